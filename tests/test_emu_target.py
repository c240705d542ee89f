"""The target-map kernel and the target product (libmpc_amd/csrc/target_kernels.hip: target_map_launch, target_map, target_apply_launch,
target_apply, compiled unchanged with g++) stepped through on the host by the lock-step interpreter of tests/emu (TEST INFRASTRUCTURE, see
tests/emu/hip/hip_runtime.h), against the 60-digit truths of tests/golden/target_truth.npz and within the bound of tests/target_ref.py, in both
orders in which the interpreter may run the lanes of a wavefront.  No GPU, nothing of libmpcx.so.  In one of the two orders a matrix that is read
before every lane has finished writing it (a missing barrier) gives other numbers; a store by a lane that owns no entry lands in the guards behind
map_u, map_x, the flags or the kernel's LDS."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import target_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -77
LDS_LIMIT = 160 * 1024


def _cm(a):
    return np.swapaxes(a, -1, -2).ravel()


def _split(o, name, shape, guard):
    a = np.array(o[name])
    cnt = int(np.prod(shape))
    assert a.size == cnt + PAD and (a[cnt:] == guard).all(), name       # nothing behind the array: no lane without an entry stores anything
    return a[:cnt].reshape(shape)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    path = str(tmp_path_factory.mktemp("emu") / "run_target")
    subprocess.run(["g++", "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", path, os.path.join(EMU, "run_target.cpp"),
                    os.path.join(EMU, "hipemu_switch.S")], check=True)
    return path


@pytest.fixture(scope="module")
def run_map(exe):
    def run(A, B, Bd, C, Dd, order="forward", want_x=True, want_flags=True, limit=LDS_LIMIT, expect_rc=0):
        """row-major [k, ., .] matrices -> map_u [k, nu, nrhs], map_x [k, nx, nrhs] (row-major), flags"""
        k, nx, nu, ndu, ny = A.shape[0], A.shape[1], B.shape[2], Bd.shape[2], C.shape[1]
        nrhs = ny + ndu + nu
        inp = " ".join(repr(float(v)) for v in np.concatenate([_cm(A), _cm(B), _cm(Bd), _cm(C), _cm(Dd)])) + "\n"
        r = subprocess.run([exe, "map"] + [str(v) for v in (nx, nu, ndu, ny, k, int(want_x), int(want_flags), limit)], input=inp,
                           capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
        assert r.returncode == 0, r.stderr[:2000]
        o = json.loads(r.stdout)
        assert o["rc"] == expect_rc
        Tu = np.swapaxes(_split(o, "map_u", (k, nrhs, nu), GUARD), 1, 2) if expect_rc == 0 else None
        if expect_rc != 0:
            assert (np.array(o["map_u"]) == GUARD).all() and (np.array(o["map_x"]) == GUARD).all() and (np.array(o["flags"]) == GUARD_I).all()
            return None
        if want_x:
            Tx = np.swapaxes(_split(o, "map_x", (k, nrhs, nx), GUARD), 1, 2)
        else:
            assert (np.array(o["map_x"]) == GUARD).all()
            Tx = None
        if want_flags:
            flags = _split(o, "flags", (k,), GUARD_I).astype(int)
        else:
            assert (np.array(o["flags"]) == GUARD_I).all()
            flags = None
        return Tu, Tx, flags
    return run


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", R.SQUARE + R.WIDE + R.LARGE + R.SPECIAL)
def test_family_against_the_truth(run_map, name, order):
    Tu, Tx, flags = run_map(*R.model(name), order=order)
    assert (flags == 0).all(), flags
    R.check_family(name, Tu, Tx, " (emulator, %s)" % order)


def test_limit_family_against_the_truth(run_map):
    """nk = 132 rows and 152 columns, 160 512 bytes of LDS: one order, to bound the time"""
    Tu, Tx, flags = run_map(*R.model("limit"), order="reverse")
    assert (flags == 0).all()
    R.check_family("limit", Tu, Tx, " (emulator)")


def test_restatement_is_the_kernel(run_map):
    """the numpy restatement the bound's constant comes from follows the kernel closely: the two differ by far less than the bound (not by nothing:
    the compiler is free to contract the elimination's multiply and subtract, the restatement is not)"""
    for name in ("shape_3_2_1_2", "shape_5_4_2_2", "chain"):
        A, B, Bd, C, Dd = R.model(name)
        Tu, Tx, _ = run_map(A, B, Bd, C, Dd)
        c = R.case(name)
        nx, nu, ndu, ny = R.dims(name)
        for i in range(A.shape[0]):
            ru, rx, flag = R.restate(A[i], B[i], Bd[i], C[i], Dd[i])
            assert flag == 0
            scale = R.C_BOUND * (2 * nx + nu + ny) * R.U * c["cond"][i]
            assert np.abs(Tu[i] - ru).max() <= scale * np.abs(ru).max() and np.abs(Tx[i] - rx).max() <= scale * np.abs(rx).max()


def test_optional_outputs(run_map):
    """map_x = NULL and flags = NULL: nothing is stored through them, map_u has the same bits"""
    m = R.model("shape_5_4_2_2")
    full = run_map(*m)
    bare = run_map(*m, want_x=False, want_flags=False)
    assert np.array_equal(full[0], bare[0]) and bare[1] is None and bare[2] is None


def test_square_case_has_no_input_reference_term_and_wide_case_projects(run_map):
    """nu = ny: the constraints determine us, Tu = 0 to the bound's scale.  nu > ny: Tu is the orthogonal projector onto the inputs that move no
    output in steady state -- symmetric and idempotent to rounding"""
    for name in R.SQUARE:
        nx, nu, ndu, ny = R.dims(name)
        Tu = run_map(*R.model(name))[0][:, :, ny + ndu:]
        assert np.abs(Tu).max() <= R.C_BOUND * (2 * nx + nu + ny) * R.U * R.case(name)["cond"].max(), name
    for name in R.WIDE:
        nx, nu, ndu, ny = R.dims(name)
        Tu = run_map(*R.model(name))[0][:, :, ny + ndu:]
        tol = R.C_BOUND * (2 * nx + nu + ny) * R.U * R.case(name)["cond"].max() * 4
        assert np.abs(Tu - np.swapaxes(Tu, 1, 2)).max() <= tol and np.abs(Tu @ Tu - Tu).max() <= tol, name


def test_flags_and_nan_outputs(run_map):
    """a batch of good instances and three failing ones: an integrator the output does not see (column 0 of K is zero) -> 1; a reference that
    cannot be reached (B = 0: S is rank deficient; dyadic entries, so the elimination meets an exact zero) -> 1; a NaN in A -> 1.  The failing
    instances are NaN throughout, the good ones have the bits of a call of their own."""
    A, B, Bd, C, Dd = (np.concatenate([np.array(a), np.array(a)], axis=0) for a in R.model("shape_2_1_1_1"))
    bad = [1, 3, 4]
    A[1] = [[1.0, 0.0], [0.0, 0.5]]; C[1] = [[0.0, 1.0]]
    A[3] = [[0.5, 0.25], [0.0, 0.5]]; B[3] = 0.0; C[3] = [[1.0, 0.0]]
    A[4, 0, 1] = np.nan
    Tu, Tx, flags = run_map(A, B, Bd, C, Dd)
    assert list(flags) == [0, 1, 0, 1, 1, 0], flags
    good = [0, 2, 5]
    assert np.isnan(Tu[bad]).all() and np.isnan(Tx[bad]).all()
    alone = run_map(A[good], B[good], Bd[good], C[good], Dd[good])
    assert np.array_equal(Tu[good], alone[0]) and np.array_equal(Tx[good], alone[1])


def test_more_outputs_than_inputs_is_singular(run_map):
    """ny > nu: rank S < nx + ny whatever the entries.  With dyadic entries the elimination is exact and ends in a zero pivot"""
    A = np.array([[[0.5]]]); B = np.array([[[1.0]]]); Bd = np.array([[[1.0]]]); C = np.array([[[1.0], [2.0]]]); Dd = np.zeros((1, 2, 1))
    Tu, Tx, flags = run_map(A, B, Bd, C, Dd)
    assert list(flags) == [1] and np.isnan(Tu).all() and np.isnan(Tx).all()


def test_past_the_lds_limit_nothing_is_launched(run_map):
    """nk (nk + nrhs) doubles above the limit the caller read from the device: -2, and no output is touched"""
    m = R.model("shape_12_4_4_4")          # 32 x 44 doubles = 11 264 bytes
    assert run_map(*m, limit=11263, expect_rc=-2) is None
    assert run_map(*m, limit=11264)[2].tolist() == [0, 0]


def test_grid_stride_reuses_a_block(run_map):
    """4096 + 5 instances at nx = 2: the tail runs in blocks 0..4 behind another instance each, and must give the bits of the same inputs in a
    call of their own"""
    rng = np.random.default_rng(7)
    k, tail = 4096 + 5, 5
    A = rng.uniform(-0.6, 0.6, size=(k, 2, 2)); B = rng.normal(size=(k, 2, 1)); Bd = rng.normal(size=(k, 2, 1))
    C = rng.normal(size=(k, 1, 2)); Dd = rng.normal(size=(k, 1, 1))
    Tu, Tx, flags = run_map(A, B, Bd, C, Dd)
    assert (flags == 0).all()
    small = run_map(A[-tail:], B[-tail:], Bd[-tail:], C[-tail:], Dd[-tail:])
    assert np.array_equal(Tu[-tail:], small[0]) and np.array_equal(Tx[-tail:], small[1])
    nu_, nx_ = R.numpy_maps(A[::211], B[::211], Bd[::211], C[::211], Dd[::211])         # and they are solutions
    assert np.allclose(Tu[::211], nu_, rtol=1e-9, atol=1e-12) and np.allclose(Tx[::211], nx_, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("per", [0, 1])
def test_product_is_the_fma_chain(exe, per):
    """us = T [r; dhat; ubar], every row from 0 by fused multiply-adds in ascending column order: bit for bit against that chain in Python, and
    nothing stored behind us; 300 instances: more than one block of the product's threads, the last one partly idle"""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    k, nu, ndu, ny = 300, 3, 2, 2
    nrhs = ny + ndu + nu
    T = rng.normal(size=(k if per else 1, nu, nrhs)); r = rng.normal(size=(k, ny)); d = rng.normal(size=(k, ndu)); ub = rng.normal(size=(k, nu))
    inp = " ".join(repr(float(v)) for v in np.concatenate([_cm(T), r.ravel(), d.ravel(), ub.ravel()])) + "\n"
    res = subprocess.run([exe, "apply", str(nu), str(ndu), str(ny), str(k), str(per)], input=inp, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[:2000]
    o = json.loads(res.stdout)
    assert o["rc"] == 0
    us = _split(o, "us", (k, nu), GUARD)
    fma = lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c))       # exact, then rounded once to nearest-even: a fused multiply-add
    for b in range(k):
        v = np.concatenate([r[b], d[b], ub[b]])
        for i in range(nu):
            acc = 0.0
            for j in range(nrhs):
                acc = fma(float(T[b if per else 0, i, j]), float(v[j]), acc)
            assert us[b, i] == acc, (b, i)
