"""Soft constraints, host side (no GPU): the two C entries and their refusals, a controller without finite weights condensing to the same
bytes, the condensed rows, Y's diagonal, g_soft and rho_g against numpy (tests/soft_ref.py), the zero-coefficient rows, the working-set
capacity, the pympcxx surface, and the yardstick itself (a bank's uniform-pattern rule needs a device: tests/test_lmpc_soft_gpu.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rate_ref as RR
import soft_ref as SR
from rate_ref import INF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["H", "Kinv", "Gr", "Gc", "Y", "lw", "uw", "rho_b", "lg0", "ug0", "rho_g", "dims", "MA0", "MA1", "Ym", "MA0p", "MA1p", "Ymp", "flags",
         "dims_maps", "g_refrow", "g_step", "g_kind", "g_comp", "g_soft", "slo", "shi", "ws_limit"]


def _host(sp, soft=True):
    from libmpc_amd import LMPC
    return SR.configure(LMPC(*sp["dims"], device=-1), sp, soft=soft)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


integrator_soft = SR.integrator_soft


def test_entries_are_exported_and_declared():
    from libmpc_amd import _capi
    lib = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    for name in ("mpcx_lmpc_set_soft_constraint_weights", "mpcx_lmpc_set_soft_constraint_weights_slice"):
        getattr(lib, name)
        assert name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    import pympcxx
    assert callable(pympcxx.LMPC.setSoftConstraintWeights)
    c = pympcxx.LMPC(2, 1, 0, 1, 4, 4, device=-1)
    assert c.setSoftConstraintWeights([1.0, 2.0], [3.0], 4.0) and not c.setSoftConstraintWeights([1.0, -2.0], [3.0], 4.0)


def test_setter_validation():
    from libmpc_amd import LMPC, _capi
    nx, nu, ndu, ny, ph, ch = 3, 2, 0, 2, 8, 3
    c = LMPC(nx, nu, ndu, ny, ph, ch, device=-1)
    lib, h = c._lib, c._h
    xw, yw = np.array([1.0, INF, 5.0]), np.array([INF, 2.0])
    assert c.setSoftConstraintWeights(xw, yw, 3.0)
    assert c.setSoftConstraintWeights(xw, yw, INF)
    assert c.setSoftConstraintWeights(None, None, None)                 # nothing changes, nothing is wrong
    assert c.setSoftConstraintWeights(xw, None, None) and c.setSoftConstraintWeights(None, yw, None) and c.setSoftConstraintWeights(None, None, 2.0)
    assert c.setSoftConstraintWeights(10.0, 20.0, 30.0)                 # a scalar: every component
    for sl, ok in (((0, ph), True), ((-1, -1), True), ((ph - 1, ph), True), ((0, ph + 1), False), ((2, 2), False), ((-1, 3), False), ((3, 2), False)):
        assert c.setSoftConstraintWeights(xw, yw, 3.0, sl) == ok, sl
    for bad in (np.nan, 0.0, -1.0, -INF):
        for k in range(nx):
            w = xw.copy(); w[k] = bad
            assert not c.setSoftConstraintWeights(w, yw, 3.0), (bad, k)
            assert not c.setSoftConstraintWeights(w, None, None, (1, 2)), (bad, k)
        for k in range(ny):
            w = yw.copy(); w[k] = bad
            assert not c.setSoftConstraintWeights(xw, w, 3.0), (bad, k)
        assert not c.setSoftConstraintWeights(xw, yw, bad), bad
        assert not c.setSoftConstraintWeights(None, None, bad, (0, 1)), bad
    one = np.array([3.0])
    assert lib.mpcx_lmpc_set_soft_constraint_weights(None, _p(xw), _p(yw), _p(one)) == _capi.E_INVALID
    assert lib.mpcx_lmpc_set_soft_constraint_weights(h, _p(xw), _p(yw), _p(one)) == 0
    assert lib.mpcx_lmpc_set_soft_constraint_weights(h, None, None, None) == 0
    assert lib.mpcx_lmpc_set_soft_constraint_weights_slice(h, _p(xw), None, None, 0, ph + 1) == _capi.E_INVALID
    with pytest.raises(ValueError):
        c.setSoftConstraintWeights(np.ones(nx + 1), yw, 1.0)


def test_a_refused_call_changes_nothing_and_an_accepted_one_invalidates_the_setup():
    sp = integrator_soft()
    c = _host(sp)
    full, refs = C.c_int(), C.c_int()
    before = {n: c.debug_get(n).copy() for n in NAMES}
    c._lib.mpcx_lmpc_debug_setup_counts(c._h, C.byref(full), C.byref(refs))
    n0 = full.value
    assert not c.setSoftConstraintWeights([INF, -10.0], None, None)
    assert not c.setSoftConstraintWeights([INF, 10.0], [0.0], None)     # one bad kind: none of the call is taken
    for n in NAMES:
        assert np.array_equal(before[n], c.debug_get(n), equal_nan=True), n
    c._lib.mpcx_lmpc_debug_setup_counts(c._h, C.byref(full), C.byref(refs))
    assert full.value == n0
    assert c.setSoftConstraintWeights([INF, 40.0], None, None)
    mg = int(c.debug_get("dims")[1])
    assert np.array_equal(c.debug_get("g_soft")[:mg], np.full(mg, 1.0 / 40.0))
    c._lib.mpcx_lmpc_debug_setup_counts(c._h, C.byref(full), C.byref(refs))
    assert full.value == n0 + 1


@pytest.mark.parametrize("dims", [(3, 2, 1, 2, 6, 3), (2, 1, 0, 1, 5, 5), (4, 2, 0, 2, 10, 9)], ids=str)
@pytest.mark.parametrize("first", [0, 1])
def test_without_finite_weights_a_controller_condenses_as_before(dims, first):
    """no call, a call with +inf, weights taken back, and weights on rows without a bound: the same bytes under every debug_get name"""
    nx, nu, ndu, ny, ph, ch = dims
    sp = RR.rate_spec(11, *dims, box=0.6, state=True, output=True, scalar=True)
    sp["first"] = first
    plain = _host(sp)
    ref = {n: plain.debug_get(n).copy() for n in NAMES}
    assert not ref["g_soft"].any() and ref["ws_limit"][0] == ref["dims"][0]
    a = _host(sp); assert a.setSoftConstraintWeights(np.full(nx, INF), np.full(ny, INF), INF)
    b = _host(SR.with_soft(sp, xw=np.full(nx, 7.0), yw=np.full(ny, 3.0), sw=5.0))
    assert b.debug_get("g_soft").any()
    assert b.setSoftConstraintWeights(np.full(nx, INF), np.full(ny, INF), INF)
    # (rate_spec bounds state component 0 alone: the other components carry a weight and no bound)
    xw = np.full(nx, 2.0); xw[0] = INF
    d = _host(sp); assert d.setSoftConstraintWeights(xw, None, None)
    cases = {"+inf": a, "taken back": b, "no bound": d}
    if first > 0:
        e = _host(sp); assert e.setSoftConstraintWeights(np.full(nx, 2.0), np.full(ny, 2.0), 2.0, (0, first))      # steps that carry no bound
        cases["unbounded steps"] = e
    for label, c in cases.items():
        for n in NAMES:
            assert np.array_equal(ref[n], c.debug_get(n), equal_nan=True), (label, n)
        assert plain.info() == c.info(), label


def _cases():
    out = []
    for tag, dims, first in (("ch<ph-1", (3, 2, 1, 2, 8, 3), 1), ("ch=ph", (3, 2, 0, 2, 8, 8), 1), ("step 0 too", (3, 2, 1, 2, 6, 6), 0)):
        out.append((tag + " all kinds", dims, first, dict(xw=[4.0, INF, INF], yw=[10.0, 100.0], sw=30.0)))
        out.append((tag + " outputs only", dims, first, dict(yw=[INF, 50.0])))
        out.append((tag + " scalar only", dims, first, dict(sw=8.0)))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_condensed_soft_rows_against_numpy(case):
    tag, dims, first, soft = case
    nx, nu, ndu, ny, ph, ch = dims
    sp = RR.rate_spec(3, *dims, box=0.6, state=True, output=True, scalar=True, rate=0.2)
    sp["first"] = first
    sp = SR.with_soft(sp, **soft)
    c, hard = _host(sp), _host(sp, soft=False)
    ref = SR.condensed(sp)
    nz, mg, ldz, ldg, ldy = (int(v) for v in c.debug_get("dims")[:5])
    assert mg == len(ref["G"]) and int(c.debug_get("dims")[9]) == ref["fixed"]
    for n, k in (("g_kind", "kind"), ("g_step", "step"), ("g_comp", "comp"), ("g_refrow", "refrow")):
        assert np.array_equal(c.debug_get(n).astype(int)[:mg], ref[k]), n
    assert np.array_equal(c.debug_get("lg0")[:mg], ref["lo"]) and np.array_equal(c.debug_get("ug0")[:mg], ref["hi"])
    gs = c.debug_get("g_soft")
    assert np.array_equal(gs[:mg], ref["g_soft"]) and not gs[mg:].any() and (gs[:mg] > 0).sum() > 0
    assert c.debug_get("ws_limit")[0] == nz + (gs > 0).sum()
    Gr = c.debug_get("Gr").reshape(ldg, ldz)
    assert np.allclose(Gr[:mg, :nz], ref["G"], rtol=1e-12, atol=1e-13)
    assert np.allclose(c.debug_get("H").reshape(ldz, ldz)[:nz, :nz], ref["H"], rtol=1e-11, atol=1e-12)
    # the dual Hessian: G Hinv G' with 1 / rho on the diagonal, and the step sizes from that diagonal
    Y = c.debug_get("Y").reshape(ldy, ldy)
    Ygg = ref["G"] @ np.linalg.solve(ref["H"], ref["G"].T) + np.diag(ref["g_soft"])
    assert np.allclose(Y[ldz:ldz + mg, ldz:ldz + mg], Ygg, rtol=1e-8, atol=1e-10)
    rho = np.clip(2.0 / np.diag(Ygg), 1e-6, 1e6)
    assert np.allclose(c.debug_get("rho_g")[:mg], rho, rtol=1e-8)
    # against the same controller with every row hard: nothing but that diagonal and the step sizes differ (and, with soft step-0 rows, those rows)
    if first > 0:
        Yh = hard.debug_get("Y").reshape(ldy, ldy)
        D = Y - Yh
        assert np.array_equal(np.diag(D)[ldz:ldz + mg] != 0, gs[:mg] > 0) and not (D - np.diag(np.diag(D))).any()
        assert np.allclose(np.diag(D)[ldz:], gs, rtol=1e-12)
        for n in NAMES:
            if n not in ("Y", "rho_g", "Kinv", "g_soft", "ws_limit", "dims"):        # (Kinv: the ADMM matrix holds G' diag(rho_g) G)
                assert np.array_equal(c.debug_get(n), hard.debug_get(n), equal_nan=True), n
        assert c.info()["m_ref"] == hard.info()["m_ref"] and c.info()["active_words"] == hard.info()["active_words"]


@pytest.mark.parametrize("reach", [True, False], ids=["B reaches the position", "B does not"])
def test_rows_without_coefficients_become_general_rows(reach):
    """soft step-0 rows and a soft later row whose coefficients vanish: general rows with Y_rr = 1 / rho and rho_g = 2 rho, their
    feasibility rows unbounded; the same rows hard: feasibility conditions, as they have always been"""
    rho = 25.0
    sp = integrator_soft(rho=rho, reach=reach)
    sp["xmin"][0] = -2.0; sp["xmax"][0] = 2.0
    sp["soft"]["xw"] = np.array([50.0, rho])
    ph = sp["dims"][4]
    c, hard = _host(sp), _host(sp, soft=False)
    nz, mg, ldz, ldg, ldy = (int(v) for v in c.debug_get("dims")[:5])
    nfix_hard = int(hard.debug_get("dims")[9])
    assert nfix_hard == (0 if reach else 1) and int(c.debug_get("dims")[9]) == 0
    assert mg == 2 * (ph + 1) and int(hard.debug_get("dims")[1]) == 2 * ph - nfix_hard
    step = c.debug_get("g_step").astype(int)[:mg]; comp = c.debug_get("g_comp").astype(int)[:mg]
    Gr = c.debug_get("Gr").reshape(ldg, ldz)[:mg, :nz]
    zero = ~Gr.any(axis=1)
    want = (step == 0) | ((step == 1) & (comp == 0) & (not reach))
    assert np.array_equal(zero, want)
    Y = c.debug_get("Y").reshape(ldy, ldy)
    w = np.where(comp == 0, 50.0, rho)
    assert np.array_equal(np.diag(Y)[ldz:ldz + mg][zero], 1.0 / w[zero])
    assert not Y[ldz:ldz + mg][zero][:, :ldz].any()
    assert np.allclose(c.debug_get("rho_g")[:mg][zero], 2.0 * w[zero], rtol=1e-14)
    assert np.array_equal(c.debug_get("g_refrow").astype(int)[:mg][step == 0], SR.SoftBuilder(sp).d.neq + np.array([0, 1]))
    # feasibility rows [x0 | lastU | y0 | scalar 0 | fixed]: the soft ones unbounded, the hard controller's as set
    assert np.array_equal(hard.debug_get("slo")[:2], [-2.0, -0.3]) and np.array_equal(hard.debug_get("shi")[:2], [2.0, 0.3])
    assert np.array_equal(c.debug_get("slo")[:2], [-INF, -INF]) and np.array_equal(c.debug_get("shi")[:2], [INF, INF])
    assert np.array_equal(c.debug_get("slo")[2:4], hard.debug_get("slo")[2:4])          # lastU and y0: as they were
    # the stacked map's offset row of a step-0 row is the state itself
    kin, nxp, nup, nyp, ione, nz16, mg16, ns, ns16, kq16, rowsA, ldy16 = c.debug_get("dims_maps").astype(int)
    M = c.debug_get("MA0").reshape(kin, rowsA).T
    rows0 = M[nz16:nz16 + mg][step == 0]
    want0 = np.zeros((2, kin)); want0[0, 0] = 1.0; want0[1, 1] = 1.0
    assert np.array_equal(rows0, want0)


def test_capacity_follows_the_soft_rows():
    """nz = 3 decision variables (ph = 40, ch = 2) and 41 soft velocity rows: working sets of up to 44 rows, the lists and the
    large-working-set slot sized for them; all of them hard: nz, as before"""
    sp = integrator_soft(ph=40, ch=2)
    c, hard = _host(sp), _host(sp, soft=False)
    nz, mg = int(c.debug_get("dims")[0]), int(c.debug_get("dims")[1])
    assert nz == 3 and mg == 41
    assert list(c.debug_get("ws_limit")) == [44.0, 44.0, 44.0 * 44.0]
    assert list(hard.debug_get("ws_limit")) == [3.0, 28.0, 9.0]
    assert c.debug_get("dims")[10] >= hard.debug_get("dims")[10]          # LDS per wavefront: the lists grow with the capacity


def test_yardstick_soft_qp_is_the_penalty_problem():
    """the slack-augmented QP against its definition: cost = plain cost + 0.5 rho sum dist^2 of the rows, the slack is the violation, and the
    case of the GPU tests: the hard QP is infeasible wherever x0's velocity is outside the bound (most of the batch), all 16 soft ones
    polish at rho = 10"""
    sp = integrator_soft(rho=10.0)
    x0, u0, _ = RR.random_batch(sp, 16, 5)
    ref = SR.solve_batch(sp, x0, u0)
    assert (ref["status"] == 0).all() and (ref["polished"] == 1).all()
    infeasible = SR.hard_infeasible(sp, x0, u0)
    assert np.array_equal(infeasible, np.abs(x0[:, 1]) > 0.3) and infeasible.sum() >= 8
    vel = ref["state"][:, :, 1]
    dist = np.maximum(np.abs(vel) - 0.3, 0.0)
    assert np.allclose(np.abs(ref["slack"]), dist, atol=1e-9)
    pbh = RR.builder({k: v for k, v in sp.items() if k != "soft"})
    for b in range(4):
        z = np.concatenate([np.concatenate([ref["state"][b, i], ref["input"][b, i - 1] if i > 0 else u0[b]]) for i in range(11)])
        du = np.diff(np.concatenate([u0[b][None], ref["input"][b, :10]]), axis=0).reshape(-1)
        z = np.concatenate([z, du])
        q, _, _ = pbh.get(x0[b], u0[b], sp["yref"], sp["uref"], sp["duref"], np.zeros((0, 10)))
        plain = 0.5 * z @ pbh.P @ z + q @ z
        assert np.isclose(ref["cost"][b], plain + 0.5 * 10.0 * (dist[b] ** 2).sum(), rtol=1e-9, atol=1e-10)
    assert ref["n_soft_active"].max() >= 5


def test_recorded_yardstick_results_are_reproduced():
    """tests/golden/soft_oracle.npz: its inputs are the cases' own, the ph = 40 case holds more active soft rows than the three decision
    variables could carry before, and its first instance solved again here gives the recorded result"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "soft_oracle.npz"))
    sp, x0, u0 = SR.large_case()
    assert np.array_equal(g["large_x0"], x0) and np.array_equal(g["large_u0"], u0) and float(g["large_rho"]) == SR.LARGE_RHO
    assert (g["large_polished"] == 1).all() and g["large_n_soft_active"].min() >= 29
    fx0, fu0, _, _ = RR.full_feature_batch(24)
    assert np.array_equal(g["full0_x0"], fx0) and np.array_equal(g["full0_u0"], fu0) and np.array_equal(g["full1_u0"], g["full0_cmd"])
    for prefix in ("full0_", "full1_"):
        assert (g[prefix + "polished"] == 1).mean() >= 0.75 and (g[prefix + "status"] == 0).all()
    r = RR.solve_one(SR.SoftBuilder(sp), sp, x0[0], u0[0])
    assert r["polished"] == g["large_polished"][0] and r["status"] == g["large_status"][0]
    assert np.allclose(r["cmd"], g["large_cmd"][0], rtol=1e-9, atol=1e-12) and np.isclose(r["cost"], g["large_cost"][0], rtol=1e-10)
    m = int(g["large_ncon"])
    assert np.array_equal(r["active_lower"], np.unpackbits(g["large_active_lower"][0], bitorder="little")[:m])
    assert np.array_equal(r["active_upper"], np.unpackbits(g["large_active_upper"][0], bitorder="little")[:m])


def test_cpp_overloads_compile_and_call_through():
    """mpc::LMPC<>::setSoftConstraintWeights: the vector forms and the pointer form that can leave a kind of row as it is (tests/cpp/lmpc_soft_test.cpp)"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "cpp", "lmpc_soft_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "build", "lmpc_soft_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "libmpc_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + lib, "-lmpcx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], env=dict(os.environ, MPCX_DEVICE="-1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ soft-constraint checks passed" in out.stdout
