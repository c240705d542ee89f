"""Sensitivities of a solved batch on the host: the reference of tests/sens_ref.py against central differences of the oracle's
own solve and against the LQR identity, the numpy restatement of the kernel's formula against that reference on every family of the GPU
tests (the figure the kernel's tolerance derives from), and the C ABI where it can be reached without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rate_ref as RR
import sens_ref as S
import terminal_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def reference(name):
    return S.reference(name)


def _host(sp):
    from libmpc_amd import LMPC
    return S.configure(LMPC(*sp["dims"], device=-1), sp)


def test_reference_agrees_with_central_differences_of_the_oracle():
    """h = 1e-5, bound 1e-8 (4e-11 measured): every column on three instances, a random direction on all of them.  A perturbed solve that
    changes the active set makes the instance unusable, under the cap."""
    R = reference("full")
    sp, pb, res = R["sp"], R["pb"], R["res"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    B, h = len(R["x0"]), 1e-5
    rg = np.random.default_rng(1)
    left_out, worst = 0, 0.0

    def solve(b, d):
        r = RR.solve_one(pb, sp, R["x0"][b] + d[:nx], R["u0"][b] + d[nx:nx + nu], R["yref"][b] + d[nx + nu:])
        al = r["active_lower"].copy(); au = r["active_upper"].copy()
        al[pb.d.neq:pb.d.neq + pb.d.na] = 0; au[pb.d.neq:pb.d.neq + pb.d.na] = 0
        same = np.array_equal(al != 0, res["active_lower"][b] != 0) and np.array_equal(au != 0, res["active_upper"][b] != 0) and r["polished"] == 1
        return r["input"], same

    for b in range(B):
        if R["jac"][b] is None:
            left_out += 1
            continue
        J = R["jac"][b]["input"]
        dirs = [rg.normal(size=nx + nu + ny)]
        if b < 3:
            dirs += list(np.eye(nx + nu + ny))
        ok = True
        for d in dirs:
            (ip, sp_), (im, sm_) = solve(b, h * d), solve(b, -h * d)
            if not (sp_ and sm_):
                ok = False
                break
            worst = max(worst, np.abs((ip - im) / (2 * h) - J @ d).max())
        left_out += not ok
    print(f"central differences: worst {worst:.2e}, left out {left_out} of {B}")
    assert left_out <= S.SKIP_CAP * B
    assert worst <= 1e-8


@pytest.mark.parametrize("ph", [1, 3, 10])
def test_reference_gives_the_lqr_gain(ph):
    """with lqr_terminal_cost's P and no active row the first move is -K x0: d cmd / d x0 = -K (the tolerance of the first move in
    tests/test_lmpc_terminal.py, 1e-9 relative)"""
    sp, Q, Rm = TR.lqr_spec("stable", ph)
    nx, nu, ndu, ny, _, ch = sp["dims"]
    pb = S.builder(sp)
    none = np.zeros(pb.d.ncon, np.uint8)
    j = S.kkt_jacobian(pb, sp, np.ones(nx), np.zeros(nu), None, none, none)
    assert S.good(j)
    Kx, Ku, Ky = S.split(j["cmd"], nx, nu)
    assert np.abs(Kx + sp["K"]).max() <= 1e-9 * np.abs(sp["K"]).max()
    # ... and the restatement on the product's arrays says the same
    cj = S.condensed_jacobian(S.arrays(_host(sp)), none, none)
    assert cj["n"] == 0 and np.abs(S.split(cj["cmd"], nx, nu)[0] + sp["K"]).max() <= 1e-9 * np.abs(sp["K"]).max()


@pytest.mark.parametrize("name", S.FAMILIES)
def test_restatement_agrees_with_the_kkt_system(name):
    """the kernel's formula in numpy on the host set-up's arrays against the KKT system of the reference QP, whole input sequence; the worst
    ratio over the families is sens_ref.RESTATEMENT_WORST"""
    R = reference(name)
    sp, res = R["sp"], R["res"]
    a = S.arrays(_host(sp))
    B = len(R["x0"])
    used = [b for b in range(B) if R["jac"][b] is not None]
    assert B - len(used) <= S.SKIP_CAP * B                  # the oracle alone stays within the cap
    worst, sizes = 0.0, []
    for b in used:
        cj = S.condensed_jacobian(a, res["active_lower"][b], res["active_upper"][b])
        assert not cj["dependent"]
        ref = R["jac"][b]["input"]
        worst = max(worst, np.abs(cj["input"] - ref).max() / max(1.0, np.abs(ref).max()))
        sizes.append(cj["n"])
    print(f"{name}: restatement worst {worst:.2e}, working sets {min(sizes)} .. {max(sizes)} rows, nz {a['nz']}, {len(used)} of {B} used")
    assert worst <= S.RESTATEMENT_WORST
    if name == "smallest":
        assert max(sizes) == 0 and a["nz"] == 1
    if name in ("nz15", "nz16", "nz17"):
        assert a["nz"] == int(name[2:])
    if name == "full":
        assert min(sizes) <= 3 and max(sizes) >= 17        # both sides of the lean kernels' 16-row limit
    if name == "soft":
        assert max(sizes) > a["nz"]                        # a working set beyond nz
    if name == "linear":
        assert (res["n_linear_active"][used] > 0).sum() >= 4
    if name == "blocked":
        ptr, ref = a["boxrow_ptr"], a["boxrow_ref"]
        act = (res["active_lower"] != 0) | (res["active_upper"] != 0)
        several = sum(any(act[b][ref[ptr[e]:ptr[e + 1]]].sum() >= 2 for e in range(a["nz"])) for b in used)
        assert (np.diff(ptr) > 1).any() and several >= 3   # instances with two or more active reference rows on one variable


def test_kernel_tolerance_is_eight_times_the_restatement_figure():
    assert S.KERNEL_TOL == max(8.0 * S.RESTATEMENT_WORST, 1e-12)
    assert "%.1e" % S.RESTATEMENT_WORST in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_full_family_has_the_rows_the_gpu_tests_look_for():
    """a rate row active at step 0: that row of d cmd / d lastU is a unit vector and of d cmd / d x0 zero; an input pinned on its box: zero rows
    in all three"""
    R = reference("full")
    sp = R["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    rate0 = boxed = 0
    for j in R["jac"]:
        if j is None:
            continue
        Kx, Ku, Ky = S.split(j["cmd"], nx, nu)
        for r in range(nu):
            e = np.zeros(nu); e[r] = 1.0
            if np.abs(Kx[r]).max() <= 1e-10 and np.abs(Ky[r]).max() <= 1e-10:
                rate0 += np.abs(Ku[r] - e).max() <= 1e-10
                boxed += np.abs(Ku[r]).max() <= 1e-10
    assert rate0 >= 1 and boxed >= 1


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared():
    from libmpc_amd import _capi
    assert "mpcx_lmpc_sensitivity_batch" in _capi.EXPORTS and _capi.lib().mpcx_lmpc_sensitivity_batch is not None
    header = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    assert "int mpcx_lmpc_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_sens *s, void *stream);" in header
    assert "} mpcx_lmpc_sens;" in header and "MPCX_SENS_JACOBIAN" in header and "MPCX_SENS_VJP" in header


def test_the_ctypes_mirror_has_the_size_of_the_struct():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.Sens) == _capi.lib().mpcx_lmpc_sens_size()


def test_refusals():
    from libmpc_amd import _capi
    lib = _capi.lib()
    c = _host(RR.full_feature_spec())
    words = c.info()["active_words"]
    al = np.zeros((2, words), np.int32); au = np.zeros((2, words), np.int32)
    seed = np.zeros((2, c.nu))

    def call(d):
        return lib.mpcx_lmpc_sensitivity_batch(c._h, None if d is None else C.byref(d), None), lib.mpcx_last_error().decode()

    def desc(**kw):
        d = _capi.Sens()
        d.batch = 2
        d.active_lower, d.active_upper = al.ctypes.data, au.ctypes.data
        d.mode = _capi.SENS_JACOBIAN
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    rc, msg = call(None)
    assert rc == _capi.E_INVALID and "null" in msg
    rc, msg = call(desc(mode=7))
    assert rc == _capi.E_INVALID and "mode" in msg
    rc, msg = call(desc(active_upper=None))
    assert rc == _capi.E_INVALID and "active_lower and active_upper" in msg
    rc, msg = call(desc(mode=_capi.SENS_VJP))
    assert rc == _capi.E_INVALID and "seed" in msg
    rc, msg = call(desc(batch=-1))
    assert rc == _capi.E_INVALID and "batch" in msg
    # a well-formed call on a host-only handle: refused as every launch is
    rc, msg = call(desc(mode=_capi.SENS_VJP, seed_cmd=seed.ctypes.data))
    assert rc == _capi.E_DEVICE and "host-only" in msg
    rc, msg = call(desc())
    assert rc == _capi.E_DEVICE and "host-only" in msg


def test_debug_names_of_the_sensitivity_tests():
    c = _host(RR.full_feature_spec())
    a = S.arrays(c)
    assert a["MF1"].shape == (a["rowsF"], a["kin"]) and a["Y"].shape == (a["ldy"], a["ldy"])
    assert len(a["boxrow_ptr"]) == a["nz"] + 1 and a["boxrow_ptr"][-1] <= len(a["boxrow_ref"])
    assert len(a["blk"]) == c.ph + 1 and a["blk"][1] == 0
    # MF1's t0 rows are -Hinv f: the constant column reproduces the unconstrained optimum of the zero input
    assert np.isfinite(a["MF1"]).all()


def _build_cpp():
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "cpp", "lmpc_sens_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "build", "lmpc_sens_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "libmpc_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + lib, "-lmpcx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_sensitivities_compiles_and_is_refused_before_a_solve():
    """mpc::LMPC<>::sensitivities() (tests/cpp/lmpc_sens_test.cpp), static and dynamic sizes; pympcxx's LMPC has sensitivityBatch"""
    import subprocess
    out = subprocess.run([_build_cpp(), "api"], env=dict(os.environ, MPCX_DEVICE="-1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ sensitivity checks passed" in out.stdout
    import pympcxx
    assert hasattr(pympcxx.LMPC, "sensitivityBatch")
    from libmpc_amd import _capi
    c = _host(RR.full_feature_spec())
    assert _capi.lib().mpcx_lmpc_sensitivity_host(c._h, None, None, None, None) == _capi.E_DEVICE


@pytest.mark.gpu
def test_cpp_sensitivities_against_differences_of_optimize():
    import subprocess
    env = {k: v for k, v in os.environ.items() if k != "MPCX_DEVICE"}
    out = subprocess.run([_build_cpp(), "solve"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ sensitivity checks passed" in out.stdout
