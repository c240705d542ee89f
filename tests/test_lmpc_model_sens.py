"""Model sensitivities of a solved batch on the host: the truth of tests/model_sens_ref.py against central differences of the
KKT solution, the numpy restatement of the kernel's formulas against that truth on every family of the GPU tests (the figure the kernel's
tolerance derives from), the host-built Xq, and the C ABI where it can be reached without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import model_sens_ref as Mo
import sens_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _host(name):
    from libmpc_amd import LMPC
    sp = Mo.reference(name)["sp"]
    return S.configure(LMPC(*sp["dims"], device=-1), sp)


def _restate(name, b):
    R = Mo.reference(name)
    sp, res = R["sp"], R["res"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    X, Yo = Mo.rollout(sp, R["x0"][b], res["input"][b])
    return Mo.condensed_gradients(Mo.arrays(_host(name)), res["active_lower"][b], res["active_upper"][b], R["u0"][b], X, Yo, res["input"][b],
                                  np.tile(R["yref"][b][:, None], (1, ph)), sp["uref"], sp["duref"], sp.get("dmeas", np.zeros((ndu, ph))),
                                  R["seed_cmd"][b], R["seed_input"][b])


@pytest.mark.parametrize("name", Mo.FAMILIES)
def test_restatement_agrees_with_the_truth(name):
    """the kernel's formulas in numpy on the host set-up's arrays against the KKT system of the reference QP, every matrix; the worst ratio over
    the families is model_sens_ref.RESTATEMENT_WORST"""
    R = Mo.reference(name)
    a = Mo.arrays(_host(name))
    B = len(R["x0"])
    used = [b for b in range(B) if R["truth"][b] is not None]
    assert 16 <= B <= 36 and B - len(used) <= Mo.SKIP_CAP * B                  # the oracle alone stays within the cap
    worst, sizes = 0.0, []
    for b in used:
        g = _restate(name, b)
        assert not g["dependent"], b
        err = Mo.compare(R["truth"][b], g)
        assert np.isfinite(err)
        worst = max(worst, err)
        sizes.append(g["n"])
    print(f"{name}: restatement worst {worst:.2e}, working sets {min(sizes)} .. {max(sizes)} rows, nz {a['nz']}, nx ph {a['nx'] * a['ph']}, {len(used)} of {B} used")
    assert worst <= Mo.RESTATEMENT_WORST
    if name in Mo.EDGE:
        assert a["nx"] * a["ph"] == int(name[5:]) and max(sizes) >= 1            # the row-tile edge of Xq q, with active rows
    if name == "nx33":
        assert a["nx"] == 33
    if name == "ndu2":
        assert a["ndu"] == 2 and np.abs(np.diff(R["sp"]["dmeas"], axis=1)).min() > 0 and max(np.abs(R["truth"][used[0]][m]).max() for m in ("Bd", "Dd")) > 1e-4
    if name == "soft":
        assert np.count_nonzero(a["g_soft"]) > 0


@pytest.mark.parametrize("name", Mo.FAMILIES)
def test_the_data_of_the_qp_is_at_most_quadratic_in_a_model_entry(name):
    """the unit central difference of the truth is exact where the third difference of the QP's data vanishes: a sample of entries of every
    matrix"""
    R = Mo.reference(name)
    sp = R["sp"]
    rg = np.random.default_rng(3)
    for m in [m for m in Mo.MODEL if m in sp]:
        for _ in range(2):
            j, i = int(rg.integers(sp[m].shape[0])), int(rg.integers(sp[m].shape[1]))
            assert Mo.third_difference(sp, m, j, i, R["x0"][0], R["u0"][0], R["yref"][0]) <= 1e-12, (m, j, i)


@pytest.mark.parametrize("name", Mo.FAMILIES)
def test_truth_agrees_with_central_differences_of_the_kkt_solution(name):
    """p' dz / d theta by central differences (h = 1e-5) of the KKT solution on the same active set, every family; the sample is two entries
    of every model matrix on three instances.  The bound is the quotient's own error, estimated without the truth, by the rule of
    tests/test_lmpc_param_sens.py: 1e-8 plus ten times the distance between the quotients at h and at 2 h.  At least a third of the compared
    entries must exceed a hundred times their bound, so that a wrong sign, factor or stage cannot pass."""
    R = Mo.reference(name)
    sp, res = R["sp"], R["res"]
    rg = np.random.default_rng(2)
    h, worst, loosest, strong, total = 1e-5, 0.0, 0.0, 0, 0
    for b in [b for b in range(len(R["x0"])) if R["truth"][b] is not None][:3]:
        seed = R["seed_input"][b].copy()
        seed[0] += R["seed_cmd"][b]

        def quotient(m, j, i, step):
            up, dn = (Mo.perturbed_input(sp, R["x0"][b], R["u0"][b], R["yref"][b], res["active_lower"][b], res["active_upper"][b], m, j, i, s * step) for s in (1, -1))
            return (seed * (up - dn)).sum() / (2 * step)

        for m in [m for m in Mo.MODEL if m in sp]:
            for _ in range(2):
                j, i = int(rg.integers(sp[m].shape[0])), int(rg.integers(sp[m].shape[1]))
                fd, fd2 = quotient(m, j, i, h), quotient(m, j, i, 2 * h)
                bound = 1e-8 + 10.0 * abs(fd - fd2)
                g = R["truth"][b][m][j, i]
                err = abs(fd - g)
                worst, loosest = max(worst, err), max(loosest, bound)
                total += 1
                strong += abs(g) >= 100.0 * bound
                assert err <= bound, (b, m, j, i, err, bound)
    print(f"{name}: central differences, worst {worst:.2e}, loosest bound {loosest:.2e}, {strong} of {total} entries above a hundred times their bound")
    assert total >= 18 and 3 * strong >= total


def test_host_built_xq_is_the_roll_out_of_the_model():
    for name in ("full", "blocked", "xrows15", "xrows16", "xrows17", "nx33"):
        c = _host(name)
        a = Mo.arrays(c)
        ref = Mo.xq_numpy(Mo.reference(name)["sp"], a["blk"])
        assert a["Xq"].shape == ref.shape and np.abs(a["Xq"] - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
        rows16 = (a["nx"] * a["ph"] + 15) // 16 * 16
        assert len(c.debug_get("Xq")) == rows16 * a["nz"]
        assert not c.debug_get("Xq").reshape(a["nz"], rows16)[:, a["nx"] * a["ph"]:].any()          # the padding rows are zero


def test_kernel_tolerance_is_eight_times_the_restatement_figure():
    assert Mo.KERNEL_TOL == max(8.0 * Mo.RESTATEMENT_WORST, 1e-12)
    assert "`RESTATEMENT_WORST = %.1e`" % Mo.RESTATEMENT_WORST in open(os.path.join(ROOT, "DESIGN.md")).read().split("### 4.10")[1]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_declared():
    from libmpc_amd import _capi
    header = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    for n in ("mpcx_lmpc_model_sensitivity_batch", "mpcx_lmpc_model_sens_size", "mpcx_lmpc_model_sens_reserve", "mpcx_lmpc_model_sensitivity_host"):
        assert n in _capi.EXPORTS and getattr(_capi.lib(), n) is not None and n + "(" in header
    assert "int mpcx_lmpc_model_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_model_sens *s, void *stream);" in header
    assert "} mpcx_lmpc_model_sens;" in header
    import libmpc_amd
    import pympcxx
    assert all(hasattr(pympcxx.LMPC, n) for n in ("make_model_sensitivity", "launch_model_sensitivity", "modelSensitivityBatch"))
    assert callable(libmpc_amd.lmpc_cmd_model)


def test_the_ctypes_mirror_has_the_size_of_the_struct():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.ModelSens) == _capi.lib().mpcx_lmpc_model_sens_size()


def test_refusals():
    from libmpc_amd import _capi
    lib = _capi.lib()
    c = _host("full")
    words = c.info()["active_words"]
    B = 2
    al = np.zeros((B, words), np.int32); au = np.zeros((B, words), np.int32)
    x0 = np.zeros((B, c.nx)); u0 = np.zeros((B, c.nu))
    sx = np.zeros((B, c.ph + 1, c.nx)); so = np.zeros((B, c.ph + 1, c.ny)); si = np.zeros((B, c.ph + 1, c.nu))
    seed = np.zeros((B, c.nu))

    def batch(**kw):
        b = _capi.Batch()
        b.batch = B
        b.x0, b.u0 = x0.ctypes.data, u0.ctypes.data
        b.active_lower, b.active_upper = al.ctypes.data, au.ctypes.data
        b.seq_state, b.seq_output, b.seq_input = sx.ctypes.data, so.ctypes.data, si.ctypes.data
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, **kw):
        d = _capi.ModelSens()
        d.solved = None if b is None else C.cast(C.pointer(b), C.c_void_p)
        d.seed_cmd = seed.ctypes.data
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.mpcx_lmpc_model_sensitivity_batch(c._h, C.byref(d), None), lib.mpcx_last_error().decode()

    rc = lib.mpcx_lmpc_model_sensitivity_batch(c._h, None, None)
    assert rc == _capi.E_INVALID and "null" in lib.mpcx_last_error().decode()
    rc, msg = call(None)
    assert rc == _capi.E_INVALID and "solved batch" in msg
    rc, msg = call(batch(batch=-1))
    assert rc == _capi.E_INVALID and "batch" in msg
    rc, msg = call(batch(), reduce=2)
    assert rc == _capi.E_INVALID and "reduce" in msg
    rc, msg = call(batch(active_upper=None))
    assert rc == _capi.E_INVALID and "active_lower and active_upper" in msg
    rc, msg = call(batch(u0=None))
    assert rc == _capi.E_INVALID and "x0 and u0" in msg
    rc, msg = call(batch(), seed_cmd=None)
    assert rc == _capi.E_INVALID and "seed" in msg
    for missing in ("seq_state", "seq_output", "seq_input"):          # a batch solved without its sequences
        rc, msg = call(batch(**{missing: None}))
        assert rc == _capi.E_STATE and "sequences" in msg
    # a well-formed call on a host-only handle: refused as every launch is
    rc, msg = call(batch())
    assert rc == _capi.E_DEVICE and "host-only" in msg
    assert lib.mpcx_lmpc_model_sens_reserve(c._h, 16) == _capi.E_DEVICE
    assert lib.mpcx_lmpc_model_sens_reserve(c._h, -1) == _capi.E_INVALID
    assert lib.mpcx_lmpc_model_sensitivity_host(c._h, seed.ctypes.data, None, 0, None, None, None, None, None, None, None) == _capi.E_DEVICE


def _build_cpp():
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "cpp", "lmpc_model_sens_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "build", "lmpc_model_sens_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "libmpc_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + lib, "-lmpcx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_model_sensitivities_compiles_and_is_refused_before_a_solve():
    """mpc::LMPC<>::modelSensitivities() (tests/cpp/lmpc_model_sens_test.cpp), static and dynamic sizes"""
    import subprocess
    out = subprocess.run([_build_cpp(), "api"], env=dict(os.environ, MPCX_DEVICE="-1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ model-sensitivity checks passed" in out.stdout
