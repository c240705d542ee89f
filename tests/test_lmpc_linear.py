"""Linear rows lo <= Fx x_i + Fu v_i <= hi without a GPU: the host condensing against an independent numpy condensing
(tests/linear_ref.py), the bytes of a controller without such rows, nc = 1 against the scalar row, refusals, row numbering, the ABI, the
offsets against the stacked maps, and the bank's condensing kernel stepped through on the host against the 60-digit truths of
tests/golden/condense_truth_linear.npz within condense_ref's bound."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import condense_ref as CR
import linear_ref as LR
import rate_ref as RR
from test_emu_condense import EMU, GUARD, PAD, _clangxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = ("H", "Kinv", "Gr", "Gc", "Y", "lw", "uw", "rho_b", "lg0", "ug0", "rho_g", "g_soft", "dims", "MA0", "MA1", "Ym", "MA0p", "MA1p", "Ymp", "flags",
         "dims_maps", "g_refrow", "g_step", "g_kind", "g_comp", "slo", "shi", "wOutput", "wU", "terminal", "ws_limit", "fixed_rows")


def _host(sp, **kw):
    from libmpc_amd import LMPC
    return LR.configure(LMPC(*sp["dims"], device=-1), sp, **kw)


def _p(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------
# the host condensing against numpy
# ---------------------------------------------------------------------------------------------
def _specs():
    out = {}
    out["smallest nc=2"] = LR.random_rows(RR.without_rate(RR.rate_spec(5, 2, 1, 0, 1, 2, 2)), 2, 3)
    out["blocked nc=3"] = LR.random_rows(RR.without_rate(RR.rate_spec(6, 3, 2, 0, 2, 8, 3)), 3, 4)
    out["ndu=1 nc=2"] = LR.random_rows(RR.without_rate(RR.rate_spec(7, 3, 2, 1, 2, 5, 5)), 2, 5)
    # a soft row: its step-0 row is a general row without coefficients
    out["soft nc=2"] = LR.random_rows(RR.without_rate(RR.rate_spec(8, 3, 1, 0, 1, 4, 4)), 2, 6, w=[INF, 30.0], onesided=False)
    return out


@pytest.mark.parametrize("name", list(_specs()))
def test_host_condensing_equals_the_numpy_condensing(name):
    sp = _specs()[name]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    c = _host(sp)
    ref = LR.condensed_linear_rows(sp)
    nz, mg, ldz, ldg = (int(v) for v in c.debug_get("dims")[:4])
    kind = c.debug_get("g_kind").astype(int)[:mg]
    sel = kind == 4
    assert sel.sum() == len(ref["lo"]) == mg                     # (these controllers have no other general rows)
    G = c.debug_get("Gr").reshape(-1, ldz)[:mg, :nz][sel]
    scale = np.abs(ref["G"]).max()
    assert np.abs(G - ref["G"]).max() <= 1e-13 * scale, np.abs(G - ref["G"]).max()
    assert np.array_equal(c.debug_get("Gc").reshape(-1, ldg)[:nz, :mg], c.debug_get("Gr").reshape(-1, ldz)[:mg, :nz].T)
    assert np.array_equal(c.debug_get("lg0")[:mg][sel], ref["lo"]) and np.array_equal(c.debug_get("ug0")[:mg][sel], ref["hi"])
    for key in ("step", "comp", "refrow"):
        assert np.array_equal(c.debug_get("g_" + key).astype(int)[:mg][sel], ref[key]), key
    assert np.array_equal(c.debug_get("g_soft")[:mg][sel], ref["g_soft"])
    # the hard rows without coefficients (step 0; behind the control horizon none here) are feasibility rows
    fixed = c.debug_get("fixed_rows").reshape(-1, 6)
    assert [tuple(r) for r in fixed] == [(4.0, float(i), float(cc), float(rr), lo, hi) for i, cc, rr, lo, hi in ref["fixed"]]
    assert int(c.debug_get("dims")[9]) == len(ref["fixed"])
    # m_ref and active_words grow by (ph + 1) nc
    d = RR.LN.LmpcDims(*sp["dims"])
    nc = sp["lin"]["Fx"].shape[0]
    assert int(c.debug_get("dims")[7]) == d.ncon + (ph + 1) * nc
    plain = _host(sp, linear=False)
    assert int(plain.debug_get("dims")[7]) == d.ncon
    assert c.info()["active_words"] == (d.ncon + (ph + 1) * nc + 31) // 32 and plain.info()["active_words"] == (d.ncon + 31) // 32
    # the offsets: coefficients of x0 and lastU in the rows of the stacked map (disturbance: the constant column, checked on the GPU)
    dm = {k: int(v) for k, v in zip(("kin", "nxp", "nup", "nyp", "ione", "nz16", "mg16", "ns", "ns16", "kq16", "rowsA", "ldy16"), c.debug_get("dims_maps"))}
    MA = c.debug_get("MA0").reshape(dm["kin"], dm["rowsA"]).T
    goff = MA[dm["nz16"]:dm["nz16"] + mg][sel]
    assert np.abs(goff[:, :nx] - ref["X0"]).max() <= 1e-13 * max(1.0, np.abs(ref["X0"]).max())
    assert np.array_equal(goff[:, dm["nxp"]:dm["nxp"] + nu], ref["U0"])
    # ... and of the feasibility rows: a hard step-0 row is Fx x0 + Fu lastU
    srow = MA[dm["nz16"] + dm["mg16"] + nx + nu + ny + 1:][:len(ref["fixed"])]
    for k, (i, cc, rr, lo, hi) in enumerate(ref["fixed"]):
        assert i == 0 and np.array_equal(srow[k, :nx], sp["lin"]["Fx"][cc]) and np.array_equal(srow[k, dm["nxp"]:dm["nxp"] + nu], sp["lin"]["Fu"][cc])
    slo, shi = c.debug_get("slo"), c.debug_get("shi")
    at = nx + nu + ny + 1
    assert np.array_equal(slo[at:at + len(fixed)], fixed[:, 4]) and np.array_equal(shi[at:at + len(fixed)], fixed[:, 5])


def test_order_among_the_other_rows():
    """behind the scalar row of their step, in front of the rate rows filed under it; the same order in the structure-only condensing (a bank's)"""
    sp = LR.random_rows(RR.full_feature_spec(), 2, 31, size=0.7, steps=range(1, 11), onesided=False)
    c = _host(sp)
    mg = int(c.debug_get("dims")[1])
    kind, step = c.debug_get("g_kind").astype(int)[:mg], c.debug_get("g_step").astype(int)[:mg]
    assert (np.diff(step) >= 0).all()
    order = {0: 0, 1: 1, 2: 2, 4: 3, 3: 4}
    for i in range(1, 11):
        ks = [order[k] for k in kind[step == i]]
        assert ks == sorted(ks) and 3 in ks and 4 in ks and (i == 1 or 2 in ks), (i, kind[step == i])      # (its state, output and scalar rows start at step 2)


# ---------------------------------------------------------------------------------------------
# a controller without linear rows condenses to the bytes it always had
# ---------------------------------------------------------------------------------------------
def test_no_rows_means_identical_bytes():
    sp = RR.full_feature_spec()
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    base = _host(sp)
    want = {n: base.debug_get(n) for n in NAMES}
    r = np.random.default_rng(2)
    Fx, Fu = r.normal(size=(3, nx)), r.normal(size=(3, nu))

    def same(c, label):
        for n in NAMES:
            got = c.debug_get(n)
            assert got.shape == want[n].shape and np.array_equal(got.view(np.uint64), want[n].view(np.uint64)), (label, n)
        assert c.info()["active_words"] == base.info()["active_words"]
    c = _host(sp)
    assert c.setLinearConstraints(None, None, None, None)
    same(c, "nc = 0")
    c = _host(sp)
    assert c.setLinearConstraints(Fx, Fu, -np.ones(3), np.ones(3))
    assert int(c.debug_get("dims")[7]) == int(want["dims"][7]) + 3 * (ph + 1)
    assert c.setLinearConstraints(None, None, None, None)
    same(c, "rows taken back")
    c = _host(sp)
    assert c.setLinearConstraints(Fx, Fu, np.full((3, ph + 1), -INF), np.full((3, ph + 1), INF))
    same(c, "all bounds infinite")
    assert c.debug_get("linear")[0] == 3.0                       # (stored all the same)


def test_nc1_is_the_scalar_row():
    """every condensed array bit-equal to the scalar-row controller's; g_kind and g_refrow differ (and m_ref with them).  Of the stacked maps the
    rows of f and of the offsets are compared: the scalar row has a feasibility slot of its own, whose row holds sX, sU in one and zeros in the other"""
    dims = (3, 2, 1, 2, 6, 6)
    base = RR.without_rate(RR.rate_spec(5, *dims))
    r = np.random.default_rng(1)
    sX, sU = r.normal(size=3), r.normal(size=2)
    for first, soft in ((1, None), (0, 25.0)):
        spa = dict(base, sX=sX, sU=sU, smin=-1.0, smax=2.0, first=first)
        if soft:
            spa = LR.SR.with_soft(spa, sw=soft)
        steps = ([0] if first == 0 else []) + list(range(first + 1, 7))
        spb = LR.with_linear(base, sX[None], sU[None], [-1.0], [2.0], w=soft, steps=steps)
        a, b = _host(spa), _host(spb)
        for n in ("H", "Kinv", "Gr", "Gc", "Y", "lw", "uw", "rho_b", "lg0", "ug0", "rho_g", "g_soft", "g_step", "g_comp", "Ym", "dims_maps", "ws_limit", "flags"):
            x, y = a.debug_get(n), b.debug_get(n)
            assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), (first, n)
        mg = int(a.debug_get("dims")[1])
        assert (a.debug_get("g_kind")[:mg] == 2).all() and (b.debug_get("g_kind")[:mg] == 4).all()
        d = RR.LN.LmpcDims(*dims)
        assert np.array_equal(a.debug_get("g_refrow")[:mg], d.neq + d.off_s + a.debug_get("g_step")[:mg])
        assert np.array_equal(b.debug_get("g_refrow")[:mg], d.ncon + b.debug_get("g_step")[:mg])
        dm = [int(v) for v in a.debug_get("dims_maps")]
        rows = dm[5] + dm[6]
        for n in ("MA0", "MA1"):
            x, y = (c.debug_get(n).reshape(dm[0], dm[10])[:, :rows] for c in (a, b))
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (first, n)


# ---------------------------------------------------------------------------------------------
# refusals: nothing is stored
# ---------------------------------------------------------------------------------------------
def test_refusals_store_nothing():
    from libmpc_amd import LMPC, _capi
    nx, nu, ndu, ny, ph, ch = 3, 2, 0, 2, 6, 3
    sp = RR.without_rate(RR.rate_spec(9, nx, nu, ndu, ny, ph, ch))
    c = RR.configure(LMPC(*sp["dims"], device=-1), sp)
    lib, h = c._lib, c._h
    r = np.random.default_rng(4)
    Fx, Fu = r.normal(size=(2, nx)), r.normal(size=(2, nu))
    lo, hi = -np.ones((2, ph + 1)), np.ones((2, ph + 1))
    assert c.setLinearConstraints(Fx, Fu, lo, hi)
    assert c.setLinearConstraintWeights([10.0, INF])
    stored = c.debug_get("linear")
    arrays = {n: c.debug_get(n) for n in NAMES}

    def untouched(label):
        assert np.array_equal(c.debug_get("linear"), stored, equal_nan=True), label
        for n in NAMES:
            assert np.array_equal(c.debug_get(n), arrays[n], equal_nan=True), (label, n)
    for what, (i, j) in (("Fx", (1, 2)), ("Fu", (0, 1)), ("lo", (1, 3)), ("hi", (0, 0))):
        for v in (np.nan,) + ((INF, -INF) if what in ("Fx", "Fu") else ()):
            args = dict(Fx=Fx.copy(), Fu=Fu.copy(), lo=lo.copy(), hi=hi.copy())
            args[what][i, j] = v
            assert not c.setLinearConstraints(args["Fx"], args["Fu"], args["lo"], args["hi"]), (what, v)
            untouched((what, v))
            assert not c.setLinearConstraints(args["Fx"], args["Fu"], args["lo"][:, 0], args["hi"][:, 0], (0, 2)) or what in ("lo", "hi") and (i, j) != (i, 0), (what, v)
            untouched((what, v, "slice"))
    bad = lo.copy(); bad[1, 4] = 2.0
    assert not c.setLinearConstraints(Fx, Fu, bad, hi)                      # lo > hi
    untouched("lo > hi")
    assert not c.setLinearConstraints(Fx, Fu, np.array([2.0, -1.0]), np.array([1.0, 1.0]), (1, 2))
    untouched("lo > hi, slice")
    cap = int(re.search(r"#define\s+MPCX_MAX_LINEAR_ROWS\s+(\d+)", open(os.path.join(ROOT, "include", "mpcx.h")).read()).group(1))
    assert cap >= 16
    big = r.normal(size=(cap + 1, nx)), r.normal(size=(cap + 1, nu))
    assert not c.setLinearConstraints(big[0], big[1], -np.ones(cap + 1), np.ones(cap + 1))
    untouched("nc above the cap")
    assert lib.mpcx_lmpc_set_linear_constraints(h, -1, None, None, None, None) == _capi.E_INVALID
    Ff, Uf, lf, hf = (np.asfortranarray(a) for a in (Fx, Fu, lo, hi))
    for k in range(4):
        ptrs = [_p(Ff), _p(Uf), _p(lf), _p(hf)]
        ptrs[k] = None
        assert lib.mpcx_lmpc_set_linear_constraints(h, 2, *ptrs) == _capi.E_INVALID
        assert lib.mpcx_lmpc_set_linear_constraints_slice(h, 2, *ptrs, 0, 1) == _capi.E_INVALID
    assert lib.mpcx_lmpc_set_linear_constraints(None, 2, _p(Ff), _p(Uf), _p(lf), _p(hf)) == _capi.E_INVALID
    untouched("null pointers")
    # a slice with another nc while other steps hold bounds; bad slices
    F3 = r.normal(size=(3, nx)), r.normal(size=(3, nu))
    assert not c.setLinearConstraints(F3[0], F3[1], -np.ones(3), np.ones(3), (ph - 1, ph))
    untouched("slice with another nc")
    for sl in ((0, ph + 1), (2, 2), (-1, 3)):
        assert not c.setLinearConstraints(Fx, Fu, lo[:, 0], hi[:, 0], sl)
        assert not c.setLinearConstraintWeights([1.0, 1.0], sl)
    assert lib.mpcx_lmpc_set_linear_constraints_slice(h, 0, None, None, None, None, 0, 1) == _capi.E_INVALID
    untouched("bad slices")
    for w in ([np.nan, 1.0], [0.0, 1.0], [1.0, -2.0]):
        assert not c.setLinearConstraintWeights(w)
    assert lib.mpcx_lmpc_set_linear_constraint_weights(h, None) == _capi.E_INVALID
    untouched("bad weights")
    # ... while the slice that covers every step may change nc, and one that covers all bounded steps too
    assert c.setLinearConstraints(F3[0], F3[1], -np.ones(3), np.ones(3), (-1, -1))
    assert c.debug_get("linear")[0] == 3.0
    assert c.setLinearConstraints(None, None, None, None)
    assert c.setLinearConstraints(Fx, Fu, lo[:, 0], hi[:, 0], (ph - 1, ph))          # the terminal set
    assert c.setLinearConstraints(F3[0], F3[1], -np.ones(3), np.ones(3), (ph - 1, ph))
    mg = int(c.debug_get("dims")[1])
    assert mg == 3 and (c.debug_get("g_step")[:mg] == ph).all() and (c.debug_get("g_kind")[:mg] == 4).all()


def test_slice_semantics_are_the_scalar_rows():
    from libmpc_amd import LMPC
    dims = (3, 2, 0, 2, 6, 6)
    base = RR.without_rate(RR.rate_spec(5, *dims))
    r = np.random.default_rng(1)
    sX, sU = r.normal(size=3), r.normal(size=2)
    for sl in ((0, 6), (-1, -1), (2, 4), (5, 6), (0, 1)):
        a = RR.configure(LMPC(*dims, device=-1), base); b = RR.configure(LMPC(*dims, device=-1), base)
        assert a.setScalarConstraint(-1.0, 2.0, sX, sU, sl) and b.setLinearConstraints(sX[None], sU[None], [-1.0], [2.0], sl)
        mg = int(a.debug_get("dims")[1])
        assert mg == int(b.debug_get("dims")[1])
        assert np.array_equal(a.debug_get("g_step"), b.debug_get("g_step")) and np.array_equal(a.debug_get("Gr"), b.debug_get("Gr"))
        # the scalar row's hard step-0 row has a slot of its own; the linear one is a fixed row
        sa, sb = a.debug_get("slo"), b.debug_get("slo")
        at = 3 + 2 + 2
        assert sa[at] == (-1.0 if sl[0] in (0, -1) else -INF) and sb[at] == -INF
        assert len(b.debug_get("fixed_rows")) == (6 if sl[0] in (0, -1) else 0)


def test_abi_exports_the_new_entries():
    from libmpc_amd import _capi
    lib = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    for name in ("mpcx_lmpc_set_linear_constraints", "mpcx_lmpc_set_linear_constraints_slice", "mpcx_lmpc_set_linear_constraint_weights",
                 "mpcx_lmpc_set_linear_constraint_weights_slice"):
        getattr(lib, name)
        assert name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    at = hdr.index("mpcx_lmpc_set_linear_constraints(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert "MPCX_MAX_LINEAR_ROWS" in comment and "lmpc_assemble_generic" in comment and "no counterpart" in comment
    import pympcxx
    assert callable(pympcxx.LMPC.setLinearConstraints) and callable(pympcxx.LMPC.setLinearConstraintWeights)


# ---------------------------------------------------------------------------------------------
# the oracle on its own: the rows bind and the plain QP violates them (the GPU tests' condition, checked where it is cheap)
# ---------------------------------------------------------------------------------------------
def test_yardstick_smallest_case():
    sp, x0, u0, yref = LR.smallest_batch(16)
    ref = LR.solve_batch(sp, x0, u0, yref)
    assert (ref["polished"] == 1).mean() >= 0.9
    vals = LR.row_values(sp, ref["state"], ref["input"], u0)
    assert LR.violation(sp, vals, rel=1e-6) <= 0.0
    assert (ref["n_linear_active"] >= 2).all()
    plain = LR.solve_batch(LR.without_linear(sp), x0, u0, yref)
    pv = LR.row_values(sp, plain["state"], plain["input"], u0)
    assert all(LR.violation(sp, pv[b:b + 1]) > 0.4 for b in range(16))


# ---------------------------------------------------------------------------------------------
# the C++ front end
# ---------------------------------------------------------------------------------------------
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "lmpc_linear_test.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "build", "lmpc_linear_test")


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
    assert "all C++ linear-row checks passed" in out.stdout


# ---------------------------------------------------------------------------------------------
# the condensing kernel stepped through on the host
# ---------------------------------------------------------------------------------------------
def test_restatement_stays_under_an_eighth_of_the_bound():
    for name in LR.FAMILIES:
        for ctl, lay, tr in LR.family(name):
            w = CR.ratios(lay, tr, LR.restate(ctl, lay))
            print("restatement %-12s %s" % (name, "  ".join("%s %5.2f" % (k, w[k]) for k in CR.ARRAYS)))
            assert max(w.values()) <= CR.C_BOUND / 8, (name, w)


@pytest.mark.parametrize("name", list(LR.FAMILIES))
def test_host_setup_against_the_truth(name):
    ctrls = LR.host_controllers(name)
    LR.check_family(name, [CR.arrays_of(c.debug_get) for c in ctrls], " (host set-up)")


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not installed")
    exe = str(tmp_path_factory.mktemp("emu_linear") / "run_condense_linear")
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", exe, os.path.join(EMU, "run_condense_linear.cpp"),
                    os.path.join(EMU, "hipemu_switch.S")], check=True)
    return exe


def _numbers(c, ctl, lay):
    """test_emu_condense._numbers with nc, Fx, Fu behind sU"""
    nx, nu, ny, ph, ch = ctl["dims"]
    nz, mg, ldz, ldg, ldy = (int(v) for v in c.debug_get("dims")[:5])
    term = c.debug_get("terminal")
    cm = lambda a: np.asarray(a, float).T.ravel()
    nc = ctl["Fx"].shape[0]
    parts = [[nx, nu, ny, ph, nz, mg, ldz, ldg, ldy, 1 | (2 if term.size else 0), 0.1, CR.SIGMA],
             cm(ctl["A"]), cm(ctl["B"]), cm(ctl["C"]), c.debug_get("wOutput"), term, c.debug_get("wU"), cm(ctl["DUW"]), ctl.get("sX", np.zeros(nx)),
             ctl.get("sU", np.zeros(nu)), [nc], cm(ctl["Fx"]), cm(ctl["Fu"]), lay["blk"]]
    parts += [c.debug_get(k) for k in ("g_kind", "g_step", "g_comp", "lw", "uw", "lg0", "ug0", "g_soft")]
    return np.concatenate([np.asarray(p, float).ravel() for p in parts])


def _run(exe, ctrls, members, order):
    inp = " ".join(repr(float(v)) for v in np.concatenate([_numbers(c, ctl, lay) for c, (ctl, lay, _) in zip(ctrls, members)])) + "\n"
    r = subprocess.run([exe, str(len(ctrls))], input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
    assert r.returncode == 0, r.stderr[:2000]
    o = json.loads(r.stdout)
    assert o["rc"] == 0
    gots = []
    for c, oc in zip(ctrls, o["controllers"]):
        nz, mg, ldz, ldg, ldy = (int(v) for v in c.debug_get("dims")[:5])
        got = {}
        for name, cnt in (("H", ldz * ldz), ("Kinv", ldz * ldz), ("Gr", ldg * ldz), ("Gc", ldz * ldg), ("Y", ldy * ldy), ("rho_b", ldz), ("rho_g", 2 * ldg)):
            a = np.array(oc[name])
            assert a.size == cnt + PAD and (a[cnt:] == GUARD).all(), name
            got[name] = a[:cnt]
        assert np.array_equal(got["rho_g"][ldg:], c.debug_get("g_soft"))
        got["rho_g"] = got["rho_g"][:ldg]
        assert oc["cond_status"] == 0 and oc["cost_direct"] == int(c.debug_get("flags")[0])
        gots.append(got)
    return gots


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", list(LR.FAMILIES))
def test_condensing_kernel_on_the_host_against_the_truth(runner, name, order):
    ctrls, fam = LR.host_controllers(name), LR.family(name)
    if name == "linear":            # four structures: a launch each (the launch takes its LDS plan from the first controller)
        gots = [_run(runner, [c], [m], order)[0] for c, m in zip(ctrls, fam)]
    else:
        gots = _run(runner, ctrls, fam, order)
    LR.check_family(name, gots, " (emulator, %s)" % order)
    for got, (ctl, lay, tr) in zip(gots, fam):
        for n, mask in CR.written(lay).items():
            assert (got[n][~mask] == (1.0 if n == "rho_g" else 0.0)).all(), (name, n)
