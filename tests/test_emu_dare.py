"""The Riccati kernel (libmpc_amd/csrc/dare_kernels.hip: dare_launch and dare_sda, compiled unchanged with g++) stepped through on the host by
the lock-step interpreter of tests/emu (TEST INFRASTRUCTURE, see tests/emu/hip/hip_runtime.h), against the 60-digit truths of
tests/golden/dare_truth.npz and within the bound of tests/dare_ref.py, in both forms and in both orders in which the interpreter may run the
lanes of a wavefront.  No GPU, nothing of libmpcx.so.  In one of the two orders a matrix that is read before every lane has finished writing
it (a missing dare_sync) gives other numbers; a store by a lane that owns no entry lands in the guards behind X, the gain, the flags, the
iteration counts or the kernel's LDS."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dare_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -77
FORM_ID = {"control": 0, "estimator": 1}


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("emu") / "run_dare")
    subprocess.run(["g++", "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", exe, os.path.join(EMU, "run_dare.cpp"),
                    os.path.join(EMU, "hipemu_switch.S")], check=True)

    def run(form, A, M, Q, Rm, order="forward", product=0):
        """row-major A [k, n, n], M = B [k, n, m] or C [k, m, n], Q and R [k, ., .] or 2-D for the batch -> X, gain (row-major), flags, iterations"""
        k, n = A.shape[0], A.shape[1]
        m = M.shape[2] if form == "control" else M.shape[1]
        cm = lambda a: (np.swapaxes(a, -1, -2)).ravel()
        numbers = np.concatenate([cm(A), cm(M), cm(Q), cm(Rm)])
        inp = " ".join(repr(float(v)) for v in numbers) + "\n"
        r = subprocess.run([exe, str(FORM_ID[form]), str(n), str(m), str(k), str(int(Q.ndim == 3)), str(int(Rm.ndim == 3)), str(product)],
                           input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=300)
        assert r.returncode == 0, r.stderr[:2000]
        o = json.loads(r.stdout)
        assert o["rc"] == 0

        def split(name, shape, guard):
            a = np.array(o[name])
            cnt = int(np.prod(shape))
            assert a.size == cnt + PAD and (a[cnt:] == guard).all(), name       # nothing behind the array: no lane without an entry stores anything
            return a[:cnt].reshape(shape)
        gshape = (k, n, m) if form == "control" else (k, m, n)                # column-major [m x n] / [n x m] per instance
        return (np.swapaxes(split("X", (k, n, n), GUARD), 1, 2), np.swapaxes(split("gain", gshape, GUARD), 1, 2),
                split("flags", (k,), GUARD_I).astype(int), split("iterations", (k,), GUARD_I).astype(int))
    return run


def _run_family(runner, name, form, order, shared=None):
    A, M, Q, Rm = R.inputs(name, form)
    if R.case(name)["shared"] if shared is None else shared:
        Q, Rm = Q[0], Rm[0]
    X, G, flags, its = runner(form, A, M, Q, Rm, order)
    assert (flags == 0).all() and (its >= 1).all() and (its <= R.MAX_DOUBLINGS).all(), (flags, its)
    return X, G


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("name", R.SHAPES + R.CONDITIONING)
def test_family_against_the_truth(runner, name, form, order):
    X, G = _run_family(runner, name, form, order)
    R.check_family(name, form, X, G, " (emulator, %s)" % order)


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("name", R.LIMIT)
def test_limit_family_against_the_truth(runner, name, form):
    """n = 32, m = 32 and both: one order, to bound the time"""
    X, G = _run_family(runner, name, form, "reverse" if form == "control" else "forward")
    R.check_family(name, form, X, G, " (emulator)")


@pytest.mark.parametrize("form", R.FORMS)
def test_one_q_and_r_for_the_batch(runner, form):
    """q_per_instance = r_per_instance = 0 with a batch above 1: the same bits as the per-instance call with Q and R repeated"""
    A, M, Q, Rm = R.inputs("rho_098", form)
    assert R.case("rho_098")["shared"]
    one = runner(form, A, M, Q[0], Rm[0])
    per = runner(form, A, M, Q, Rm)
    assert all(np.array_equal(a, b) for a, b in zip(one, per))


@pytest.mark.parametrize("product", [1, 2])
@pytest.mark.parametrize("name", ["shape_5_2", "shape_17_3", "shape_2_3"])
def test_both_product_forms(runner, name, product):
    """lanes over the entries and the matrix pipe, each forced, on sizes either side of the threshold between them"""
    A, M, Q, Rm = R.inputs(name, "estimator")
    X, G, flags, _ = runner("estimator", A, M, Q, Rm, "reverse", product)
    assert (flags == 0).all()
    R.check_family(name, "estimator", X, G, " (emulator, product form %d)" % product)


def test_flags_and_nan_outputs(runner):
    """a batch of good instances and three failing ones: R not positive definite -> 1; an unstable mode the output does not see
    (A = diag(1.5, 0.5), C = [0 1]) -> 3, since a squares its entries every step and overflows at the eleventh doubling, long before
    the cap; a NaN in A -> 3.  The failing instances are NaN throughout, the good ones have the bits of a call of their own."""
    A, M, Q, Rm = (np.array(a) for a in R.inputs("shape_2_1", "estimator"))
    A, M, Q, Rm = (np.concatenate([a, a], axis=0) for a in (A, M, Q, Rm))
    bad = [1, 3, 4]
    Rm[1] = -0.04
    A[3] = np.diag([1.5, 0.5]); M[3] = [[0.0, 1.0]]
    A[4, 0, 1] = np.nan
    X, G, flags, its = runner("estimator", A, M, Q, Rm)
    assert list(flags) == [0, 1, 0, 3, 3, 0], flags
    assert its[1] == 0 and 5 <= its[3] <= 12, its
    good = [0, 2, 5]
    assert np.isnan(X[bad]).all() and np.isnan(G[bad]).all()
    alone = runner("estimator", A[good], M[good], Q[good], Rm[good])
    assert np.array_equal(X[good], alone[0]) and np.array_equal(G[good], alone[1]) and np.array_equal(its[good], alone[3])


def test_grid_stride_reuses_a_block(runner):
    """4096 + 5 instances at n = 2: the tail runs in blocks 0..4 behind another instance each, and must give the bits of the same inputs in a
    call of their own"""
    rng = np.random.default_rng(5)
    k, tail = 4096 + 5, 5
    A = rng.uniform(-1.0, 1.0, size=(k, 2, 2)); C = rng.normal(size=(k, 1, 2))
    Q = np.array([[0.02, 0.005], [0.005, 0.01]]); Rm = np.array([[0.04]])
    X, G, flags, its = runner("estimator", A, C, Q, Rm)
    assert (flags == 0).all()
    small = runner("estimator", A[-tail:], C[-tail:], Q, Rm)
    assert np.array_equal(X[-tail:], small[0]) and np.array_equal(G[-tail:], small[1]) and np.array_equal(its[-tail:], small[3])
    for i in list(range(0, 4096, 211)) + list(range(4094, k)):           # and they are solutions: the restatement agrees within the bound's scale
        Xr, Kr, flag, _ = R.restate(A[i].T, C[i].T, Q, Rm)
        assert flag == 0
        assert np.abs(X[i] - Xr).max() <= R.C_BOUND * 2 * R.U * np.abs(Xr).max(), i
        assert np.abs(G[i] - Kr.T).max() <= R.C_BOUND * 2 * R.U * np.abs(Kr).max(), i
