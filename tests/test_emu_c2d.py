"""The discretisation kernel (libmpc_amd/csrc/c2d_kernels.hip: c2d_launch and c2d_expm, compiled unchanged with g++) stepped through on the host
by the lock-step interpreter of tests/emu (TEST INFRASTRUCTURE, see tests/emu/hip/hip_runtime.h), against the 60-digit truths of
tests/golden/c2d_truth.npz and within the bound of tests/c2d_ref.py, in both orders in which the interpreter may run the lanes of a wavefront.
No GPU, nothing of libmpcx.so.  In one of the two orders a product that is copied back before every lane has finished it (a missing
c2d_sync) gives other numbers; a store by a lane that owns no entry lands in the guards behind Ad, Bd or the kernel's LDS."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import c2d_ref as R
from oracle.utils_numpy import discretization as ref_c2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
PAD, GUARD = 64, -7.25e300
FAMILIES = ["random_g1", "random_g30"] + R.TINY + ["nu0", "chain", "zero", "cs_edge", "limit_45_1"]       # limit_45_1: n = 46


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("emu") / "run_c2d")
    subprocess.run(["g++", "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", exe, os.path.join(EMU, "run_c2d.cpp"),
                    os.path.join(EMU, "hipemu_switch.S")], check=True)

    def run(A, B, Ts, per, order):
        """A [m, nx, nx], B [m, nx, nu] row-major, Ts [m] or [1] -> Ad, Bd row-major"""
        m, nx, nu = A.shape[0], A.shape[1], B.shape[2]
        numbers = np.concatenate([np.swapaxes(A, 1, 2).ravel(), np.swapaxes(B, 1, 2).ravel(), np.ravel(Ts)])
        inp = " ".join(repr(float(v)) for v in numbers) + "\n"
        r = subprocess.run([exe, str(nx), str(nu), str(m), str(int(per))], input=inp, capture_output=True, text=True,
                           env=dict(os.environ, HIPEMU_ORDER=order), timeout=120)
        assert r.returncode == 0, r.stderr[:2000]
        o = json.loads(r.stdout)
        assert o["rc"] == 0

        def split(name, shape):
            a = np.array(o[name])
            n = int(np.prod(shape))
            assert a.size == n + PAD and (a[n:] == GUARD).all(), name      # nothing behind the array: no lane without an entry stores anything
            return np.swapaxes(a[:n].reshape(shape), 1, 2)
        return split("Ad", (m, nx, nx)), split("Bd", (m, nu, nx))
    return run


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", FAMILIES)
def test_family_against_the_truth(runner, name, order):
    c = R.case(name)
    Ad, Bd = runner(c["A"], c["B"], c["Ts"], True, order)
    R.check_family(name, Ad, Bd, " (emulator, %s)" % order)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_one_sampling_time_for_the_batch(runner, order):
    """ts_per_instance = 0 with a batch above 1: the same bits as the per-instance call with Ts repeated"""
    c = R.case("random_g30")
    ts = c["Ts"][2:3]
    one = runner(c["A"], c["B"], ts, False, order)
    per = runner(c["A"], c["B"], np.repeat(ts, c["A"].shape[0]), True, order)
    assert np.array_equal(one[0], per[0]) and np.array_equal(one[1], per[1])


def test_grid_stride_reuses_a_block(runner):
    """4096 + 5 instances at n = 3: the tail runs in blocks 0..4 behind a stiff instance each (9 squarings and more; the tail needs none), and
    must give the bits of the same inputs in a call of their own"""
    rng = np.random.default_rng(77)
    m, tail = 4096 + 5, 5
    A, B, Ts = R.grid_stride_inputs(rng, m, tail)
    s = R.squarings(A, B, Ts)
    assert s[:4096].min() >= 8 and s[4096:].max() == 0
    Ad, Bd = runner(A, B, Ts, True, "forward")
    small = runner(A[4096:], B[4096:], Ts[4096:], True, "forward")
    assert np.array_equal(Ad[4096:], small[0]) and np.array_equal(Bd[4096:], small[1])
    for i in list(range(0, 4096, 97)) + list(range(4090, m)):
        ra, rb = ref_c2d(A[i], B[i], Ts[i])
        assert R.worst_ratio(A[i:i + 1], B[i:i + 1], Ts[i:i + 1], ra[None], rb[None], Ad[i:i + 1], Bd[i:i + 1]) <= 1.0, i
