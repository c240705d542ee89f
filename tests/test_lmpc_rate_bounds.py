"""Input-rate bounds, host side (no GPU): the two C entries, their refusals, the condensed rows against numpy (tests/rate_ref.py), a
controller that never calls the setter condensing as before, and the C++ overloads."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rate_ref as RR
from rate_ref import INF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["H", "Kinv", "Gr", "Gc", "Y", "lw", "uw", "rho_b", "lg0", "ug0", "rho_g", "dims", "MA0", "MA1", "Ym", "MA0p", "MA1p", "Ymp", "flags",
         "dims_maps", "g_refrow", "g_step", "g_kind", "g_comp"]


def _host(sp, rate=True):
    from libmpc_amd import LMPC
    return RR.configure(LMPC(*sp["dims"], device=-1), sp, rate=rate)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_entries_are_exported_and_declared_with_their_provenance():
    from libmpc_amd import _capi
    lib = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    for name in ("mpcx_lmpc_set_input_rate_bounds", "mpcx_lmpc_set_input_rate_bounds_slice"):
        getattr(lib, name)
        assert name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    at = hdr.index("mpcx_lmpc_set_input_rate_bounds(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert "ProblemBuilder.hpp:768-793" in comment and "no setter" in comment
    import pympcxx
    assert callable(pympcxx.LMPC.setInputRateBounds)


def test_refusals():
    from libmpc_amd import LMPC, _capi
    nx, nu, ndu, ny, ph, ch = 3, 2, 0, 2, 8, 3
    c = LMPC(nx, nu, ndu, ny, ph, ch, device=-1)
    lib, h = c._lib, c._h
    lo, hi = -np.ones((nu, ph)), np.ones((nu, ph))
    assert c.setInputRateBounds(lo, hi)
    assert c.setInputRateBounds(lo[:, 0], hi[:, 0], (0, ph))           # a prediction-horizon slice, as the delta-u weight's
    assert c.setInputRateBounds(lo[:, 0], hi[:, 0], (-1, -1))
    assert c.setInputRateBounds(lo[:, 0], hi[:, 0], (ph - 1, ph))
    assert not c.setInputRateBounds(lo[:, 0], hi[:, 0], (0, ph + 1))
    assert not c.setInputRateBounds(lo[:, 0], hi[:, 0], (2, 2))
    assert not c.setInputRateBounds(lo[:, 0], hi[:, 0], (-1, 3))
    lo_f = np.asfortranarray(lo); hi_f = np.asfortranarray(hi)
    assert lib.mpcx_lmpc_set_input_rate_bounds(h, None, _p(hi_f)) == _capi.E_INVALID
    assert lib.mpcx_lmpc_set_input_rate_bounds(h, _p(lo_f), None) == _capi.E_INVALID
    assert lib.mpcx_lmpc_set_input_rate_bounds_slice(h, None, _p(hi_f), 0, 1) == _capi.E_INVALID
    assert lib.mpcx_lmpc_set_input_rate_bounds_slice(h, _p(lo_f), None, 0, 1) == _capi.E_INVALID
    assert lib.mpcx_lmpc_set_input_rate_bounds(None, _p(lo_f), _p(hi_f)) == _capi.E_INVALID
    for col in range(ph):
        bad = lo.copy(); bad[1, col] = np.nan
        assert not c.setInputRateBounds(bad, hi), col                   # NaN anywhere
        bad = hi.copy(); bad[0, col] = np.nan
        assert not c.setInputRateBounds(lo, bad), col
        crossed = lo.copy(); crossed[1, col] = 2.0
        assert c.setInputRateBounds(crossed, hi) == (col > ch), col     # dumin > dumax: refused where the column is read
        assert c.setInputRateBounds(crossed[:, col], hi[:, col], (col, col + 1)) == (col > ch), col
    assert not c.setInputRateBounds(np.array([np.nan, 0.0]), hi[:, 0], (ph - 1, ph))
    assert c.setInputRateBounds(np.full(nu, -INF), np.full(nu, INF), (0, ph))
    assert c.setInputRateBounds(np.full(nu, 0.0), np.full(nu, 0.0), (0, 1))      # dumin == dumax is a bound


def test_a_refused_call_changes_nothing_and_an_accepted_one_invalidates_the_setup():
    sp = RR.rate_spec(5, 3, 2, 0, 2, 6, 6, box=0.6)
    c = _host(sp)
    full, refs = C.c_int(), C.c_int()
    before = {n: c.debug_get(n).copy() for n in NAMES}
    c._lib.mpcx_lmpc_debug_setup_counts(c._h, C.byref(full), C.byref(refs))
    n0 = full.value
    bad = sp["dumin"].copy(); bad[0, 0] = np.nan
    assert not c.setInputRateBounds(bad, sp["dumax"])
    for n in NAMES:
        assert np.array_equal(before[n], c.debug_get(n), equal_nan=True), n
    c._lib.mpcx_lmpc_debug_setup_counts(c._h, C.byref(full), C.byref(refs))
    assert full.value == n0
    assert c.setInputRateBounds(0.5 * sp["dumin"], 0.5 * sp["dumax"])
    mg = int(c.debug_get("dims")[1])
    assert np.array_equal(c.debug_get("lg0")[:mg], 0.5 * before["lg0"][:mg])
    c._lib.mpcx_lmpc_debug_setup_counts(c._h, C.byref(full), C.byref(refs))
    assert full.value == n0 + 1


@pytest.mark.parametrize("dims", [(3, 2, 1, 2, 6, 3), (2, 1, 0, 1, 5, 5), (4, 2, 0, 2, 10, 9)], ids=str)
def test_without_the_setter_a_controller_condenses_as_before(dims):
    """no call, a call with the default (+-inf everywhere), finite bounds taken back, and finite bounds in the columns that are not
    read (i > ch): the same bytes under every debug_get name, and no row of the new kind"""
    nx, nu, ndu, ny, ph, ch = dims
    sp = RR.rate_spec(11, *dims, box=0.6, state=True, output=True, scalar=True)
    plain = _host(sp, rate=False)
    ref = {n: plain.debug_get(n).copy() for n in NAMES}
    mg = int(ref["dims"][1])
    assert not (ref["g_kind"][:mg] == 3).any()
    # rows as counted from the spec: one state bound, ny output bounds and the scalar row per step 1..ph (none of them vanishes here)
    assert mg + int(ref["dims"][9]) == ph * (1 + ny + 1)
    inf_lo, inf_hi = np.full((nu, ph), -INF), np.full((nu, ph), INF)
    a = _host(sp, rate=False); assert a.setInputRateBounds(inf_lo, inf_hi)
    b = _host(sp, rate=True); assert b.setInputRateBounds(np.full(nu, -INF), np.full(nu, INF), (-1, -1))
    cases = {"default": a, "taken back": b}
    if ch + 1 < ph:
        lo, hi = inf_lo.copy(), inf_hi.copy()
        lo[:, ch + 1:] = -0.1; hi[:, ch + 1:] = 0.1
        d = _host(sp, rate=False); assert d.setInputRateBounds(lo, hi)
        cases["unread columns"] = d
    for label, c in cases.items():
        for n in NAMES:
            assert np.array_equal(ref[n], c.debug_get(n), equal_nan=True), (label, n)
        assert plain.info() == c.info(), label


def _variants():
    out = []
    for tag, (ph, ch) in {"ch<ph-1": (8, 3), "ch=ph-1": (8, 7), "ch=ph": (8, 8)}.items():
        out.append((tag + " full", (3, 2, 0, 2, ph, ch), "full"))
        out.append((tag + " slices", (3, 2, 0, 2, ph, ch), "slices"))
        out.append((tag + " one-sided", (3, 2, 1, 2, ph, ch), "one-sided"))
        out.append((tag + " one component", (3, 2, 0, 2, ph, ch), "component"))
    out.append(("nu=1 ph=2", (2, 1, 0, 1, 2, 2), "full"))
    return out


@pytest.mark.parametrize("case", _variants(), ids=lambda c: c[0])
def test_condensed_rate_rows_against_numpy(case):
    from libmpc_amd import LMPC
    tag, dims, how = case
    nx, nu, ndu, ny, ph, ch = dims
    sp = RR.rate_spec(3, *dims, box=0.6, state=True, output=True, scalar=True, vary=(how == "full"))
    r = np.random.default_rng(8)
    if how == "slices":
        # the bounds arrive through the slice entry: the whole horizon, then a few steps on top
        sp["dumin"] = np.tile(np.array([[-0.3], [-0.2]])[:nu], (1, ph)); sp["dumax"] = np.tile(np.array([[0.25], [0.35]])[:nu], (1, ph))
        sp["dumin"][:, 2:5] = np.array([[-0.05], [-0.07]])[:nu]; sp["dumax"][:, 2:5] = np.array([[0.06], [0.04]])[:nu]
        sp["dumin"][:, ph - 1] = -0.9; sp["dumax"][:, ph - 1] = 0.9
    elif how == "one-sided":
        sp["dumin"] = np.full((nu, ph), -INF); sp["dumax"] = r.uniform(0.05, 0.2, size=(nu, ph))
        sp["dumin"][0, 1] = -0.1; sp["dumax"][0, 1] = INF          # one row bounded below only
    elif how == "component":
        sp["dumin"][0, :] = -INF; sp["dumax"][0, :] = INF           # the second of two components only
    c = RR.configure(LMPC(*dims, device=-1), sp, rate=(how != "slices"))
    if how == "slices":
        assert c.setInputRateBounds(sp["dumin"][:, 0], sp["dumax"][:, 0], (-1, -1))
        assert c.setInputRateBounds(sp["dumin"][:, 2], sp["dumax"][:, 2], (2, 5))
        assert c.setInputRateBounds(sp["dumin"][:, ph - 1], sp["dumax"][:, ph - 1], (ph - 1, ph))
    plain = _host(sp, rate=False)

    G, lo, hi, step, comp, ref, U0 = RR.condensed_rate_rows(sp)
    nf = min(ph, ch + 1)
    assert len(G) == np.isfinite(np.where(np.isfinite(sp["dumin"]), sp["dumin"], sp["dumax"])[:, :nf]).sum()
    nz, mg, ldz, ldg = (int(v) for v in c.debug_get("dims")[:4])
    mg0 = int(plain.debug_get("dims")[1])
    assert nz == nf * nu and mg == mg0 + len(G)
    assert int(c.debug_get("dims")[9]) == int(plain.debug_get("dims")[9])               # no rate row is a fixed row
    kind = c.debug_get("g_kind").astype(int)[:mg]; gstep = c.debug_get("g_step").astype(int)[:mg]
    gcomp = c.debug_get("g_comp").astype(int)[:mg]; gref = c.debug_get("g_refrow").astype(int)[:mg]
    rate = kind == 3
    assert rate.sum() == len(G)
    # order: by step; within a step the rate rows (of delta_{step-1}) come last; the other rows are the plain controller's, in its order
    assert (np.diff(gstep) >= 0).all()
    for s in np.unique(gstep):
        k = kind[gstep == s]
        assert (np.diff((k == 3).astype(int)) >= 0).all(), s
    Gr = c.debug_get("Gr").reshape(ldg, ldz); Gc = c.debug_get("Gc").reshape(ldz, ldg)
    assert np.array_equal(Gr, Gc.T)
    assert np.array_equal(Gr[:mg][rate][:, :nz], G) and not Gr[:mg][rate][:, nz:].any()
    assert np.array_equal(gstep[rate], step) and np.array_equal(gcomp[rate], comp) and np.array_equal(gref[rate], ref)
    assert np.array_equal(c.debug_get("lg0")[:mg][rate], lo) and np.array_equal(c.debug_get("ug0")[:mg][rate], hi)
    pl_ldg, pl_ldz = (int(v) for v in plain.debug_get("dims")[[3, 2]])
    assert np.array_equal(Gr[:mg][~rate][:, :nz], plain.debug_get("Gr").reshape(pl_ldg, pl_ldz)[:mg0, :nz])
    for n in ("g_kind", "g_step", "g_comp", "g_refrow", "lg0", "ug0"):
        assert np.array_equal(c.debug_get(n)[:mg][~rate], plain.debug_get(n)[:mg0]), n
    for n in ("H", "lw", "uw", "rho_b"):
        assert np.array_equal(c.debug_get(n), plain.debug_get(n)), n
    # the reference's numbering: m_ref and the bitmap size do not change
    assert c.info()["m_ref"] == plain.info()["m_ref"] and c.info()["active_words"] == plain.info()["active_words"]
    # the stacked map: goff = -lastU[comp] for delta_0 and nothing else -- -1 in the u0 block, zero in the x0, yref and constant columns
    kin, nxp, nup, nyp, ione, nz16, mg16, ns, ns16, kq16, rowsA, ldy16 = c.debug_get("dims_maps").astype(int)
    for name in ("MA0", "MA1"):
        M = c.debug_get(name).reshape(kin, rowsA).T                      # rowsA x kin
        rows = M[nz16:nz16 + mg][rate]
        want = np.zeros((len(G), kin)); want[:, nxp:nxp + nu] = U0
        assert np.array_equal(rows, want), name
    # the dual Hessian's rate block is what it claims to be
    Y = c.debug_get("Y").reshape(ldz + ldg, ldz + ldg)
    H = c.debug_get("H").reshape(ldz, ldz)[:nz, :nz]
    Yref = Gr[:mg, :nz] @ np.linalg.solve(H, Gr[:mg, :nz].T)
    assert np.allclose(Y[ldz:ldz + mg, ldz:ldz + mg], Yref, rtol=1e-8, atol=1e-10)


def test_rows_equal_the_reference_qp_rows_condensed():
    """the same rows from the reference's A matrix: delta-u row (i, j) of ProblemBuilderRef applied to the parametrisation z = Z w of
    tests/test_host_setup.py"""
    from test_host_setup import _dense_condensed_from_oracle_builder
    for dims in [(3, 2, 0, 2, 8, 3), (4, 2, 0, 2, 10, 10)]:
        nx, nu, ndu, ny, ph, ch = dims
        sp = RR.rate_spec(21, *dims, box=0.6, vary=True)
        c = _host(sp)
        pb = RR.builder(sp)
        nz, mg, ldz, ldg = (int(v) for v in c.debug_get("dims")[:4])
        _, Z = _dense_condensed_from_oracle_builder(pb, nf=min(ph, ch + 1))
        Gr = c.debug_get("Gr").reshape(ldg, ldz)[:mg, :nz]
        rows = c.debug_get("g_refrow").astype(int)[:mg]
        assert np.allclose(Gr, (pb.A @ Z)[rows], atol=1e-12)
        rate = c.debug_get("g_kind").astype(int)[:mg] == 3
        assert np.array_equal(c.debug_get("lg0")[:mg][rate], pb.lineq[rows[rate] - pb.d.neq])
        assert np.array_equal(c.debug_get("ug0")[:mg][rate], pb.uineq[rows[rate] - pb.d.neq])


def test_the_oracle_is_bounded_by_the_rate_and_the_plain_problem_is_not():
    """the yardstick itself, on the CPU: the reference QP with finite delta-u rows keeps every move on or inside the bound, the same QP
    without them moves more than three times as far -- in one solve and along the closed loop of the GPU tests"""
    sp = RR.integrator_spec()
    pb, pb0 = RR.builder(sp), RR.builder(RR.without_rate(sp))
    x = np.zeros(2); u = np.zeros(1); x_0 = x.copy(); u_0 = u.copy()
    worst, worst0 = 0.0, 0.0
    for k in range(12):
        r = RR.solve_one(pb, sp, x, u); r0 = RR.solve_one(pb0, sp, x_0, u_0)
        # (polished_raw: a feasible polished point is all this test needs -- where the polish kept a row too many, rate_ref clears 'polished')
        assert r["status"] == 0 and r["polished_raw"] == 1 and r0["status"] == 0
        worst = max(worst, abs(r["cmd"][0] - u[0])); worst0 = max(worst0, abs(r0["cmd"][0] - u_0[0]))
        x = sp["A"] @ x + sp["B"] @ r["cmd"]; u = r["cmd"]
        x_0 = sp["A"] @ x_0 + sp["B"] @ r0["cmd"]; u_0 = r0["cmd"]
    assert worst <= 0.1 * (1 + 1e-6) and worst0 > 0.3, (worst, worst0)


def test_recorded_oracle_results_are_reproduced():
    """tests/golden/rate_bounds_oracle.npz (the 160-row case of the GPU tests): its inputs are rate_ref.large_case()'s, and its first
    instance solved again here gives the recorded result"""
    sp, x0, u0, yref = RR.large_case()
    g = np.load(os.path.join(ROOT, "tests", "golden", "rate_bounds_oracle.npz"))
    assert np.array_equal(g["x0"], x0) and np.array_equal(g["u0"], u0) and np.array_equal(g["yref"], yref)
    assert (g["polished"] == 1).mean() >= 0.9 and g["n_rate_active"].max() > 28
    r = RR.solve_one(RR.builder(sp), sp, x0[0], u0[0], yref[0])
    assert r["polished"] == g["polished"][0] and r["status"] == g["status"][0]
    assert np.allclose(r["cmd"], g["cmd"][0], rtol=1e-9, atol=1e-12) and np.isclose(r["cost"], g["cost"][0], rtol=1e-10)
    m = int(g["ncon"])
    assert np.array_equal(r["active_lower"], np.unpackbits(g["active_lower"][0], bitorder="little")[:m])
    assert np.array_equal(r["active_upper"], np.unpackbits(g["active_upper"][0], bitorder="little")[:m])


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "lmpc_rate_bounds_test.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "build", "lmpc_rate_bounds_test")


def build_cpp():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(CPP_OUT), exist_ok=True)
    lib = os.path.join(ROOT, "libmpc_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), CPP_SRC, "-o", CPP_OUT,
                           "-L" + lib, "-lmpcx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return CPP_OUT


def test_cpp_overloads_compile_and_call_through():
    exe = build_cpp()
    out = subprocess.run([exe, "api"], env=dict(os.environ, MPCX_DEVICE="-1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ rate-bound checks passed" in out.stdout
