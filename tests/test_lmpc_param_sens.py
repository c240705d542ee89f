"""Parameter sensitivities of a solved batch on the host: the truth of tests/param_sens_ref.py against central differences of
the KKT solution, the numpy restatement of the kernel's formulas against that truth on every family of the GPU tests (the figure the kernel's
tolerance derives from), the host-built Cq, and the C ABI where it can be reached without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import param_sens_ref as P
import sens_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _host(name):
    from libmpc_amd import LMPC
    sp = P.reference(name)["sp"]
    return S.configure(LMPC(*sp["dims"], device=-1), sp)


def _restate(name, b):
    R = P.reference(name)
    sp, res = R["sp"], R["res"]
    ph = sp["dims"][4]
    return P.condensed_gradients(P.arrays(_host(name)), res["active_lower"][b], res["active_upper"][b], R["u0"][b],
                                 P.rollout(sp, R["x0"][b], res["input"][b]), res["input"][b], np.tile(R["yref"][b][:, None], (1, ph)),
                                 sp["uref"], sp["duref"], R["seed_cmd"][b], R["seed_input"][b])


@pytest.mark.parametrize("name", P.FAMILIES)
def test_restatement_agrees_with_the_truth(name):
    """the kernel's formulas in numpy on the host set-up's arrays against the KKT system of the reference QP, all five outputs; the worst ratio
    over the families is param_sens_ref.RESTATEMENT_WORST"""
    R = P.reference(name)
    a = P.arrays(_host(name))
    B = len(R["x0"])
    used = [b for b in range(B) if R["truth"][b] is not None]
    assert B - len(used) <= P.SKIP_CAP * B                  # the oracle alone stays within the cap
    worst, sizes = 0.0, []
    for b in used:
        g = _restate(name, b)
        assert not g["dependent"]
        worst = max(worst, P.compare(a, R["truth"][b], g, blocked=(name == "blocked")))
        sizes.append(g["n"])
    print(f"{name}: restatement worst {worst:.2e}, working sets {min(sizes)} .. {max(sizes)} rows, nz {a['nz']}, ny ph {a['ny'] * a['ph']}, {len(used)} of {B} used")
    assert worst <= P.RESTATEMENT_WORST
    if name in P.EDGE:
        assert a["ny"] * a["ph"] == int(name[4:]) and max(sizes) >= 2        # the row-tile edge of Cq q, with active rows
    if name == "blocked":
        assert (np.diff(a["boxrow_ptr"]) > 1).any()


@pytest.mark.parametrize("name", P.FAMILIES)
def test_truth_agrees_with_central_differences_of_the_kkt_solution(name):
    """p' dz / d theta by central differences (h = 1e-5) of the KKT solution on the same active set, every family; the sample is three entries
    of every weight matrix on three instances.  The bound is the quotient's own error, estimated without the truth: 1e-8 plus ten times the
    distance between the quotients at h and at 2 h.  Where truncation decides, that distance is three times the error at h; where the rounding
    of the two solves decides (the soft family's penalty weights: its quotients scatter by 1e-7 at h = 1e-5 and by ten times as much at
    h = 1e-6), the two quotients carry independent noise of the error's size.  At least a third of the compared entries must exceed a hundred
    times their bound, so that a wrong sign, factor or stage cannot pass."""
    R = P.reference(name)
    sp, res, tr = R["sp"], R["res"], R["tr"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    rg = np.random.default_rng(2)
    h, worst, loosest, strong, total = 1e-5, 0.0, 0.0, 0, 0
    for b in [b for b in range(len(R["x0"])) if R["truth"][b] is not None][:3]:
        seed = R["seed_input"][b].copy()
        seed[0] += R["seed_cmd"][b]

        def quotient(w, j, i, step):
            up, dn = (P.perturbed_input(tr, R["x0"][b], R["u0"][b], R["yref"][b], res["active_lower"][b], res["active_upper"][b], w, j, i, s * step) for s in (1, -1))
            return (seed * (up - dn)).sum() / (2 * step)

        for w in P.WEIGHTS:
            for _ in range(3):
                j, i = int(rg.integers(sp[w].shape[0])), int(rg.integers(ph))
                fd, fd2 = quotient(w, j, i, h), quotient(w, j, i, 2 * h)
                bound = 1e-8 + 10.0 * abs(fd - fd2)
                g = R["truth"][b][w][j, i]
                err = abs(fd - g)
                worst, loosest = max(worst, err), max(loosest, bound)
                total += 1
                strong += abs(g) >= 100.0 * bound
                assert err <= bound, (b, w, j, i, err, bound)
    print(f"{name}: central differences, worst {worst:.2e}, loosest bound {loosest:.2e}, {strong} of {total} entries above a hundred times their bound")
    assert total == 27 and 3 * strong >= total


def test_host_built_cq_is_the_roll_out_of_the_model():
    for name in ("full", "blocked", "rows15", "rows16", "rows17"):
        c = _host(name)
        a = P.arrays(c)
        ref = P.cq_numpy(P.reference(name)["sp"], a["blk"])
        assert a["Cq"].shape == ref.shape and np.abs(a["Cq"] - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
        rows16 = (a["ny"] * a["ph"] + 15) // 16 * 16
        assert len(c.debug_get("Cq")) == rows16 * a["nz"]
        assert not c.debug_get("Cq").reshape(a["nz"], rows16)[:, a["ny"] * a["ph"]:].any()          # the padding rows are zero


def test_kernel_tolerance_is_eight_times_the_restatement_figure():
    assert P.KERNEL_TOL == max(8.0 * P.RESTATEMENT_WORST, 1e-12)
    assert "`RESTATEMENT_WORST = %.1e`" % P.RESTATEMENT_WORST in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_declared():
    from libmpc_amd import _capi
    header = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    for n in ("mpcx_lmpc_param_sensitivity_batch", "mpcx_lmpc_param_sens_size", "mpcx_lmpc_param_sens_reserve", "mpcx_lmpc_param_sensitivity_host"):
        assert n in _capi.EXPORTS and getattr(_capi.lib(), n) is not None and n + "(" in header
    assert "int mpcx_lmpc_param_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_param_sens *s, void *stream);" in header
    assert "} mpcx_lmpc_param_sens;" in header
    import libmpc_amd
    import pympcxx
    assert all(hasattr(pympcxx.LMPC, n) for n in ("make_param_sensitivity", "launch_param_sensitivity", "paramSensitivityBatch"))
    assert callable(libmpc_amd.lmpc_cmd_params)


def test_the_ctypes_mirror_has_the_size_of_the_struct():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.ParamSens) == _capi.lib().mpcx_lmpc_param_sens_size()


def test_refusals():
    from libmpc_amd import _capi
    lib = _capi.lib()
    c = _host("full")
    words = c.info()["active_words"]
    B = 2
    al = np.zeros((B, words), np.int32); au = np.zeros((B, words), np.int32)
    x0 = np.zeros((B, c.nx)); u0 = np.zeros((B, c.nu)); so = np.zeros((B, c.ph + 1, c.ny)); si = np.zeros((B, c.ph + 1, c.nu))
    seed = np.zeros((B, c.nu))

    def batch(**kw):
        b = _capi.Batch()
        b.batch = B
        b.x0, b.u0 = x0.ctypes.data, u0.ctypes.data
        b.active_lower, b.active_upper = al.ctypes.data, au.ctypes.data
        b.seq_output, b.seq_input = so.ctypes.data, si.ctypes.data
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, **kw):
        d = _capi.ParamSens()
        d.solved = None if b is None else C.cast(C.pointer(b), C.c_void_p)
        d.seed_cmd = seed.ctypes.data
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.mpcx_lmpc_param_sensitivity_batch(c._h, C.byref(d), None), lib.mpcx_last_error().decode()

    rc = lib.mpcx_lmpc_param_sensitivity_batch(c._h, None, None)
    assert rc == _capi.E_INVALID and "null" in lib.mpcx_last_error().decode()
    rc, msg = call(None)
    assert rc == _capi.E_INVALID and "solved batch" in msg
    rc, msg = call(batch(batch=-1))
    assert rc == _capi.E_INVALID and "batch" in msg
    rc, msg = call(batch(), reduce=2)
    assert rc == _capi.E_INVALID and "reduce" in msg
    rc, msg = call(batch(active_upper=None))
    assert rc == _capi.E_INVALID and "active_lower and active_upper" in msg
    rc, msg = call(batch(seq_input=None))
    assert rc == _capi.E_INVALID and "seq_output and seq_input" in msg
    rc, msg = call(batch(u0=None))
    assert rc == _capi.E_INVALID and "x0 and u0" in msg
    rc, msg = call(batch(), seed_cmd=None)
    assert rc == _capi.E_INVALID and "seed" in msg
    # a well-formed call on a host-only handle: refused as every launch is
    rc, msg = call(batch())
    assert rc == _capi.E_DEVICE and "host-only" in msg
    assert lib.mpcx_lmpc_param_sens_reserve(c._h, 16) == _capi.E_DEVICE
    assert lib.mpcx_lmpc_param_sens_reserve(c._h, -1) == _capi.E_INVALID
    assert lib.mpcx_lmpc_param_sensitivity_host(c._h, seed.ctypes.data, None, 0, None, None, None, None, None, None, None) == _capi.E_DEVICE


def _build_cpp():
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "cpp", "lmpc_param_sens_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "build", "lmpc_param_sens_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "libmpc_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + lib, "-lmpcx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_parameter_sensitivities_compiles_and_is_refused_before_a_solve():
    """mpc::LMPC<>::parameterSensitivities() (tests/cpp/lmpc_param_sens_test.cpp), static and dynamic sizes"""
    import subprocess
    out = subprocess.run([_build_cpp(), "api"], env=dict(os.environ, MPCX_DEVICE="-1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ parameter-sensitivity checks passed" in out.stdout
