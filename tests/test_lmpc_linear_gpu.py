"""Linear rows lo <= Fx x_i + Fu v_i <= hi on the GPU: every solve path, the two-chunk variant, large working sets, terminal
sets, infeasibility, soft rows, warm starts, a heterogeneous bank and the closed loops against the reference QP with the rows appended
(tests/linear_ref.py), at the tolerances of test_lmpc_rate_bounds_gpu.py, which are BASELINE.json's: u* 1e-5 relative, cost 1e-7, status and
solver_status equal, active bits equal on rate_ref.compared_rows plus the new rows wherever the oracle polished.  Every batch has the oracle
polished on at least 90 % of its instances (the seeds were chosen on the CPU for that), and all polished instances are compared.  Oracle solves
that take seconds are recorded in tests/golden/linear_oracle.npz (tests/golden/make_linear_golden.py)."""
import os
import subprocess

import numpy as np
import pytest

import condense_ref as CR
import linear_ref as LR
import rate_ref as RR
from helpers import assert_matches_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, debug_force_generic, debug_use_fused) -- the five paths of test_lmpc_shapes_gpu.py
PATHS = [("default", False, None), ("two-kernel", False, 0), ("generic", True, None), ("fused", False, 1), ("group", False, 2)]
EQUAL = ("cost", "status", "solver_status", "iterations", "polish_rounds", "active_count")
INF = float("inf")


def _controller(sp, generic=False, fused=None, warm=False, linear=True, maximum_iteration=RR.MAXIT):
    from libmpc_amd import LMPC, LParameters
    c = LR.configure(LMPC(*sp["dims"], device=0), sp, maximum_iteration, linear=linear)
    if warm:
        c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration, enable_warm_start=1))
    c.debug_force_generic(generic)
    c.debug_use_fused(fused)
    return c


def _paths(sp):
    """(name, controller) of the paths this controller can take"""
    for pname, generic, fused in PATHS:
        c = _controller(sp, generic, fused)
        flags = c.debug_get("flags")
        if (pname == "fused" and int(flags[2]) != 1) or (pname == "group" and int(flags[1]) != 1):
            continue
        yield pname, c


def _gpu_refs(yref=None, dmeas=None):
    """the reference helper's [B, n, ph] per-step arrays in the front end's [B, ph, n] layout"""
    kw = {}
    if yref is not None:
        kw["yref"] = np.ascontiguousarray(yref.transpose(0, 2, 1)) if yref.ndim == 3 else yref
    if dmeas is not None:
        kw["dmeas"] = np.ascontiguousarray(dmeas.transpose(0, 2, 1))
    return kw


def _solve(c, x0, u0, **kw):
    import torch
    r = c.optimizeBatch(x0, u0, want_active=True, **kw)
    torch.cuda.synchronize()
    return r


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _check(r, ref, sp, label, idx=None):
    """cmd, cost, status, solver_status and the compared active bits of every polished instance; idx: the instances of ref that r holds"""
    if idx is not None:
        ref = {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 else v) for k, v in ref.items()}
    pol = ref["polished"] == 1
    assert pol.mean() >= 0.9, (label, pol.mean())
    try:
        assert_matches_oracle(r, ref, ref["neq"], ref["ncon"], check_active=False)
    except AssertionError as e:
        raise AssertionError((label,) + e.args) from e
    st = r.status.cpu().numpy(); sst = r.solver_status.cpu().numpy()
    assert np.array_equal(st, ref["status"]), (label, np.nonzero(st != ref["status"])[0][:8])
    assert np.array_equal(sst[pol], ref["solver_status"][pol]), label
    keep = LR.compared_rows(sp)
    m = int(ref["ncon"])
    assert r.active_lower.shape[1] == (m + 31) // 32
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == (ref["active_lower"][:, keep] != 0)).all(axis=1) & (up[:, keep] == (ref["active_upper"][:, keep] != 0)).all(axis=1)
    assert same[pol].all(), (label, int(np.argmin(same | ~pol)))
    return r.active_count.cpu().numpy()


def _rows_of(r, sp, u0):
    """[B, nc, ph + 1]: the rows' values on the returned sequences"""
    return LR.row_values(sp, r.seq_state.cpu().numpy(), r.seq_input.cpu().numpy(), u0)


# ---------------------------------------------------------------------------------------------
# 1. the smallest shape: one row on u alone, one on x and u, both active
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smallest():
    sp, x0, u0, yref = LR.smallest_batch(65)
    return sp, x0, u0, yref, LR.solve_batch(sp, x0, u0, yref), LR.solve_batch(LR.without_linear(sp), x0, u0, yref)


@pytest.mark.parametrize("B", [1, 64, 65])
def test_smallest_shape_obeys_the_rows_and_matches_the_oracle(smallest, B):
    import torch
    sp, x0, u0, yref, ref, ref_plain = smallest
    idx = np.arange(B)
    row0 = ref["ncon_ref"]
    act = ((ref["active_lower"] != 0) | (ref["active_upper"] != 0))[:, row0:].reshape(-1, 3, 2).any(axis=1)
    assert act.all()                                         # both rows are active in every instance
    c = _controller(sp)
    r = c.optimizeBatch(x0[:B], u0[:B], yref=yref[:B], want_active=True, want_sequence=True); torch.cuda.synchronize()
    _check(r, ref, sp, "B=%d" % B, idx)
    worst = LR.violation(sp, _rows_of(r, sp, u0[:B]), rel=1e-5)
    print("B=%d: largest row value beyond its bound widened by 1e-5: %.3e" % (B, worst))
    assert worst <= 0.0, worst
    # the same controller without the setter violates them by more than six times the bound, as the reference's plain QP does
    pv = LR.row_values(sp, ref_plain["state"], ref_plain["input"], u0)
    assert min(LR.violation(sp, pv[b:b + 1]) for b in range(65)) > 3.6
    pc = _controller(sp, linear=False)
    plain = pc.optimizeBatch(x0[:B], u0[:B], yref=yref[:B], want_active=True, want_sequence=True); torch.cuda.synchronize()
    got = _rows_of(plain, sp, u0[:B])
    assert min(LR.violation(sp, got[b:b + 1]) for b in range(B)) > 3.6
    _check(plain, ref_plain, LR.without_linear(sp), "plain B=%d" % B, idx)


# ---------------------------------------------------------------------------------------------
# 2. nc = 1 is the scalar row
# ---------------------------------------------------------------------------------------------
def test_nc1_equals_the_scalar_row_controller():
    import torch
    from libmpc_amd import LMPC
    dims = (3, 2, 0, 2, 6, 6)
    base = RR.without_rate(RR.rate_spec(5, *dims))
    base.update(umin=-np.ones(2), umax=np.ones(2))
    r0 = np.random.default_rng(1)
    sX, sU = r0.normal(size=3), r0.normal(size=2)
    spa = dict(base, sX=sX, sU=sU, smin=-0.4, smax=0.4, first=1)
    spb = LR.with_linear(base, sX[None], sU[None], [-0.4], [0.4], steps=range(2, 7))
    x0, u0, _ = RR.random_batch(base, 32, 3)
    d = RR.LN.LmpcDims(*dims)
    for pname, generic, fused in PATHS[:3]:
        a = RR.configure(LMPC(*dims, device=0), spa); b = LR.configure(LMPC(*dims, device=0), spb)
        for c in (a, b):
            c.debug_force_generic(generic); c.debug_use_fused(fused)
        ra, rb = _solve(a, x0, u0), _solve(b, x0, u0)
        for name in ("cmd", "cost", "iterations", "active_count", "status", "solver_status", "polish_rounds"):
            assert torch.equal(getattr(ra, name), getattr(rb, name)), (pname, name)
        for side in ("active_lower", "active_upper"):
            ba, bb = _bits(getattr(ra, side), d.ncon), _bits(getattr(rb, side), d.ncon + 7)
            assert np.array_equal(ba[:, :d.neq + d.off_s], bb[:, :d.neq + d.off_s]) and not bb[:, d.neq + d.off_s:d.ncon].any(), (pname, side)
            assert np.array_equal(ba[:, d.neq + d.off_s:], bb[:, d.ncon:]), (pname, side)         # the bit sits at the new row number
        assert _bits(ra.active_lower, d.ncon)[:, d.neq + d.off_s:].any() or _bits(ra.active_upper, d.ncon)[:, d.neq + d.off_s:].any()


# ---------------------------------------------------------------------------------------------
# 3. move blocking, ch = ph and the full-feature controller, on every path the controller can take (oracle results recorded)
# ---------------------------------------------------------------------------------------------
_CASES = {}


def _case_ref(name):
    if name not in _CASES:
        sp, x0, u0, yref, dmeas = LR.case(name)
        _CASES[name] = ((sp, x0, u0, yref, dmeas), LR.recorded(name, x0=x0, u0=u0, yref=yref, dmeas=dmeas))
    return _CASES[name]


@pytest.mark.parametrize("name", ["blocked", "ch=ph", "full"])
def test_every_path_matches_the_oracle(name):
    (sp, x0, u0, yref, dmeas), ref = _case_ref(name)
    assert (ref["n_linear_active"] > 0).sum() >= 12            # half the batch leans on a linear row
    if name == "full":
        # the five kinds of row meet in one working set, with a disturbance model
        d = RR.LN.LmpcDims(*sp["dims"])
        act = ((ref["active_lower"] != 0) | (ref["active_upper"] != 0))[:, d.neq:]
        kinds = np.stack([act[:, :d.off_y].any(axis=1), act[:, d.off_y:d.off_du].any(axis=1), act[:, d.off_du:d.off_s].any(axis=1),
                          act[:, d.off_s:d.nineq].any(axis=1), act[:, d.nineq:].any(axis=1)])
        assert kinds.all(axis=0).sum() >= 4
    ran = []
    for pname, c in _paths(sp):
        _check(_solve(c, x0, u0, **_gpu_refs(yref, dmeas)), ref, sp, "%s %s" % (name, pname))
        ran.append(pname)
    print("%s: paths %s; active linear rows per instance up to %d, working sets up to %d" % (name, ran, ref["n_linear_active"].max(), ref["n_active"].max()))
    assert {"default", "two-kernel", "generic"} <= set(ran)


# ---------------------------------------------------------------------------------------------
# 4. more than 128 general rows: the two-chunk kernel variant (oracle results recorded)
# ---------------------------------------------------------------------------------------------
def test_160_linear_rows_take_the_two_chunk_variant():
    sp, x0, u0, yref = LR.large_case()
    ref = LR.recorded("large", x0=x0, u0=u0, yref=yref)
    for pname, generic, fused in PATHS[:3]:
        c = _controller(sp, generic, fused)
        assert c.info()["kernel_variant"] == 2 and int(c.debug_get("dims")[1]) == 160
        _check(_solve(c, x0, u0, yref=yref), ref, sp, "large " + pname)
    assert ref["n_linear_active"].max() > 28                   # more rows than the in-kernel polish holds


# ---------------------------------------------------------------------------------------------
# 5. a working set of more than 16 linear rows: past the lean kernels' 16, the fallback lands on the oracle
# ---------------------------------------------------------------------------------------------
def test_a_working_set_of_more_than_16_linear_rows():
    (sp, x0, u0, yref, dmeas), ref = _case_ref("ch=ph")
    big = np.nonzero(ref["n_linear_active"] > 16)[0]
    assert len(big) >= 2 and (ref["polished"][big] == 1).all()
    for pname, c in _paths(sp):
        r = _solve(c, x0[big], u0[big], yref=yref[big])
        ac = _check(r, ref, sp, "more than 16 rows " + pname, big)
        assert (ac > 16).all(), (pname, ac)


# ---------------------------------------------------------------------------------------------
# 6. a terminal set, together with a terminal cost
# ---------------------------------------------------------------------------------------------
def test_terminal_set_with_terminal_cost():
    import torch
    from libmpc_amd import LMPC
    ph = 10
    sp = LR.terminal_spec(ph)
    L = sp["lin"]
    r0 = np.random.default_rng(3)
    x0 = np.stack([r0.uniform(-0.2, 0.2, size=8), r0.uniform(-0.1, 0.1, size=8)], axis=1); u0 = np.zeros((8, 1))
    ref = LR.solve_batch(sp, x0, u0)
    # the controller through the slice form: the last step only
    c = LR.configure(LMPC(*sp["dims"], device=0), sp, linear=False)
    assert c.setLinearConstraints(L["Fx"], L["Fu"], L["lo"][:, ph], L["hi"][:, ph], (ph - 1, ph))
    mg = int(c.debug_get("dims")[1])
    assert mg == 3 and (c.debug_get("g_step")[:mg] == ph).all() and c.debug_get("terminal").size > 0
    r = c.optimizeBatch(x0, u0, want_active=True, want_sequence=True); torch.cuda.synchronize()
    _check(r, ref, sp, "terminal set")
    val = r.seq_state.cpu().numpy()[:, ph, :] @ L["Fx"].T
    lo, hi = L["lo"][:, ph], L["hi"][:, ph]
    tol = 1e-5                                               # (every finite bound is below 1 in size)
    assert (val >= lo - tol).all() and (val <= hi + tol).all(), (val.min(axis=0), val.max(axis=0))
    # at least one face is active in every instance, by the values and by the bits at the new row numbers
    d = RR.LN.LmpcDims(*sp["dims"])
    on = (np.abs(val - lo) <= tol) | (np.abs(val - hi) <= tol)
    m = d.ncon + 3 * (ph + 1)
    bits = (_bits(r.active_lower, m) | _bits(r.active_upper, m))[:, d.ncon + 3 * ph:]
    assert on.any(axis=1).all() and (bits != 0).any(axis=1).all() and not (bits != 0)[~on].any()
    # without the set the last state misses it
    plain = LR.configure(LMPC(*sp["dims"], device=0), sp, linear=False)
    rp = plain.optimizeBatch(x0, u0, want_sequence=True); torch.cuda.synchronize()
    vp = rp.seq_state.cpu().numpy()[:, ph, :] @ L["Fx"].T
    assert ((vp < lo - 10 * tol) | (vp > hi + 10 * tol)).any(axis=1).all()


# ---------------------------------------------------------------------------------------------
# 7. infeasibility: a step-0 row violated by (x0, lastU); two rows that contradict each other
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["step-0 row", "contradiction"])
def test_infeasible_by_linear_rows(how):
    """The oracle reports primal infeasibility; the strict mode reports what the oracle does, the default mode what the reference's front end
    does with such a problem (MAX_ITERATION, a finite command; include/mpcx.h), as with the scalar row and the rate rows"""
    dims = (3, 2, 0, 2, 6, 6)
    base = RR.without_rate(RR.rate_spec(500, *dims, rate=0.1, box=0.6))
    x0, u0, _ = RR.random_batch(base, 8, 3)
    x0 = 0.3 * x0
    if how == "step-0 row":
        # |x_1 + v_1| <= 1.5 at every step, step 0 included: there the row reads x0 and lastU, which are data
        sp = LR.with_linear(base, [[1.0, 0.0, 0.0]], [[1.0, 0.0]], [-1.5], [1.5])
        bad = np.array([2, 5])
        x0[bad, 0] = 2.5
    else:
        # v_1 + v_2 <= -0.3 and v_1 + v_2 >= 0.3 at step 2: no input satisfies both, whatever the instance
        sp = LR.with_linear(base, np.zeros((2, 3)), [[1.0, 1.0], [1.0, 1.0]], [-INF, 0.3], [-0.3, INF], steps=[2])
        bad = np.arange(8)
    good = np.setdiff1d(np.arange(8), bad)
    ref = LR.solve_batch(sp, x0, u0)
    assert (ref["status"][bad] == 2).all() and (ref["is_feasible"][bad] == 0).all() and (ref["status"][good] == 0).all()
    assert (ref["solver_status"][bad] == RR.OSQP.OSQP_PRIMAL_INFEASIBLE).all() and (ref["polished"][good] == 1).all()
    c = _controller(sp)
    c.setStrictInfeasibility(True)
    r = _solve(c, x0, u0)
    assert np.array_equal(r.status.cpu().numpy(), ref["status"]) and np.array_equal(r.is_feasible.cpu().numpy(), ref["is_feasible"])
    assert np.array_equal(r.solver_status.cpu().numpy(), ref["solver_status"])
    assert np.isnan(r.cmd.cpu().numpy()[bad]).all()
    loose = _solve(_controller(sp), x0, u0)
    assert (loose.status.cpu().numpy()[bad] == 1).all() and (loose.is_feasible.cpu().numpy() == 1).all() and np.isfinite(loose.cmd.cpu().numpy()).all()
    for res in (r, loose):
        if not len(good):
            break
        cmd = res.cmd.cpu().numpy()[good]
        err = np.abs(cmd - ref["cmd"][good]).max(axis=1) / np.maximum(np.abs(ref["cmd"][good]).max(axis=1), 1e-12)
        assert err.max() <= 1e-5, err.max()
        cost = res.cost.cpu().numpy()[good]
        assert (np.abs(cost - ref["cost"][good]) / np.maximum(1.0, np.abs(ref["cost"][good]))).max() <= 1e-7
        assert (res.status.cpu().numpy()[good] == 0).all()
        assert np.array_equal(res.solver_status.cpu().numpy()[good], ref["solver_status"][good])


# ---------------------------------------------------------------------------------------------
# 8. soft linear rows against the slack QP
# ---------------------------------------------------------------------------------------------
def test_soft_linear_rows_match_the_slack_qp():
    dims = (3, 2, 0, 2, 6, 6)
    base = RR.without_rate(RR.rate_spec(500, *dims, rate=0.1, box=0.6))
    x0, u0, _ = RR.random_batch(base, 16, 3)
    x0 = 0.3 * x0
    x0[[2, 5], 0] = 2.5                                        # the step-0 row is violated by the data there
    r0 = np.random.default_rng(6)
    Fx = np.vstack([[1.0, 0.0, 0.0], r0.normal(size=3)]); Fu = np.vstack([[1.0, 0.0], r0.normal(size=2)])
    sp = LR.with_linear(base, Fx, Fu, [-1.5, -0.3], [1.5, 0.3], w=[20.0, 5.0])
    ref = LR.solve_batch(sp, x0, u0)
    assert (ref["status"] == 0).all() and (ref["polished"] == 1).mean() >= 0.9 and ref["n_linear_active"].min() >= 1
    hard = LR.solve_batch(LR.with_linear(base, Fx, Fu, [-1.5, -0.3], [1.5, 0.3]), x0[[2, 5]], u0[[2, 5]])
    assert (hard["status"] == 2).all()                         # the same rows hard: infeasible by the data
    for pname, c in _paths(sp):
        c.setStrictInfeasibility(True)                         # a soft row never makes an instance infeasible, strict mode included
        r = _solve(c, x0, u0)
        _check(r, ref, sp, "soft " + pname)
        assert (r.status.cpu().numpy() == 0).all()
    # `cost` includes the penalty: with the weights ten times as large it is larger on the violated instances
    sp10 = LR.with_linear(base, Fx, Fu, [-1.5, -0.3], [1.5, 0.3], w=[200.0, 50.0])
    r1, r10 = _solve(_controller(sp), x0, u0), _solve(_controller(sp10), x0, u0)
    assert (r10.cost.cpu().numpy()[[2, 5]] > r1.cost.cpu().numpy()[[2, 5]] + 1.0).all()


# ---------------------------------------------------------------------------------------------
# 9. warm against cold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocked", "ch=ph", "full"])
def test_warm_start_with_shift_equals_cold(name):
    import torch
    (sp, x0, u0, yref, dmeas), ref = _case_ref(name)
    kw = _gpu_refs(yref, dmeas)
    c = _controller(sp, warm=True)
    first = _solve(c, x0, u0, **kw)
    _check(first, ref, sp, name + " tick 0")
    cmd = ref["cmd"]                          # the next tick from the oracle's command (the GPU's is equal to 1e-5): the same problem on every run
    x1 = LR.next_tick(sp, x0, cmd, dmeas)
    cold = _solve(_controller(sp), x1, cmd, **kw)
    for shift in (True, False):
        warm = _solve(c, x1, cmd, warm=first, warm_shift=shift, **kw)
        a, b = warm.cmd.cpu().numpy(), cold.cmd.cpu().numpy()
        scale = np.maximum(np.abs(b).max(axis=1), 1e-12)
        assert (np.abs(a - b).max(axis=1) / scale).max() <= 1e-5, (name, shift)
        ca, cb = warm.cost.cpu().numpy(), cold.cost.cpu().numpy()
        assert (np.abs(ca - cb) / np.maximum(1.0, np.abs(cb))).max() <= 1e-7, (name, shift)
        assert torch.equal(warm.status, cold.status) and torch.equal(warm.solver_status, cold.solver_status)
        # the active sets, on the rows that are compared with the oracle's: with move blocking the rows behind the control horizon read the same
        # block of inputs at several steps, and which of two such rows carries the multiplier is not determined by the optimum
        keep = LR.compared_rows(sp)
        for side in ("active_lower", "active_upper"):
            wa, co = _bits(getattr(warm, side), len(keep)), _bits(getattr(cold, side), len(keep))
            assert np.array_equal(wa[:, keep], co[:, keep]), (name, shift, side)
            assert keep.all() <= np.array_equal(wa, co), (name, shift, side)      # (no blocking: every bit)
    # ... and the second tick is the oracle's as well
    _check(cold, LR.recorded(name + " tick 1", x0=x1, u0=cmd), sp, name + " tick 1")


# ---------------------------------------------------------------------------------------------
# 10. a bank of controllers with their own Fx, Fu and bounds
# ---------------------------------------------------------------------------------------------
def test_hetero_bank_condenses_within_the_bound_and_solves():
    import torch
    from libmpc_amd import LMPC, LMPCHetero, MpcxError
    fam = LR.family("linear_bank")
    ctrls = LR.host_controllers("linear_bank")
    host = LMPCHetero(ctrls, device=0, condense_on_host=True)
    dev = LMPCHetero(ctrls, device=0)
    assert host.debug_get(0, "flags")[1] == 0.0 and dev.debug_get(0, "flags")[1] == 1.0
    gots = [CR.arrays_of(lambda n, k=k: dev.debug_get(k, n)) for k in range(len(fam))]
    LR.check_family("linear_bank", gots, " (device)")
    for k, (ctl, lay, tr) in enumerate(fam):
        assert (ctrls[k].debug_get("g_kind") == 4).sum() == 15
        for n, mask in CR.written(lay).items():
            a, b = gots[k][n], host.debug_get(k, n)
            assert a.size == b.size == mask.size and np.array_equal(a[~mask].view(np.uint64), b[~mask].view(np.uint64)), (k, n)
    # the solves, per controller, against the yardstick
    specs = []
    for k, (ctl, lay, tr) in enumerate(fam):
        nx, nu, ny, ph, ch = ctl["dims"]
        rr = np.random.default_rng(1000 + k)                     # (condense_ref.configure's references)
        sp = dict(dims=(nx, nu, 0, ny, ph, ch), A=ctl["A"], B=ctl["B"], C=ctl["C"], OW=ctl["OW"], UW=ctl["UW"], DUW=ctl["DUW"], umin=ctl["umin"], umax=ctl["umax"],
                  xmin=ctl["xmin"], xmax=ctl["xmax"], yref=0.3 * rr.normal(size=(ny, ph)), uref=np.zeros((nu, ph)), duref=np.zeros((nu, ph)))
        specs.append(dict(sp, lin=dict(Fx=ctl["Fx"], Fu=ctl["Fu"], lo=ctl["flo"], hi=ctl["fhi"], w=None)))
    B = 21
    r0 = np.random.default_rng(17)
    x0 = 0.3 * r0.normal(size=(B, 3)); u0 = r0.uniform(-0.2, 0.2, size=(B, 2)); yref = 1.5 * r0.normal(size=(B, 2))
    model = np.arange(B) % 3
    ra = host.optimizeBatch(x0, u0, yref=yref, model=model, want_active=True); rb = dev.optimizeBatch(x0, u0, yref=yref, model=model, want_active=True)
    torch.cuda.synchronize()
    assert torch.equal(ra.status, rb.status) and torch.equal(ra.active_lower, rb.active_lower) and torch.equal(ra.active_upper, rb.active_upper)
    np.testing.assert_allclose(ra.cmd.cpu().numpy(), rb.cmd.cpu().numpy(), rtol=1e-8, atol=1e-10)
    parts = [(np.nonzero(model == k)[0], LR.solve_batch(specs[k], x0[model == k], u0[model == k], yref[model == k])) for k in range(3)]
    ref = {k: parts[0][1][k] for k in ("neq", "ncon", "ncon_ref", "nc")}
    for key, first in parts[0][1].items():
        if isinstance(first, np.ndarray):
            ref[key] = np.zeros((B,) + first.shape[1:], dtype=first.dtype)
            for idx, p in parts:
                ref[key][idx] = p[key]
    assert ref["n_linear_active"].max() >= 2
    _check(rb, ref, specs[0], "bank")
    _check(ra, ref, specs[0], "bank condensed on the host")
    # a controller with another number of linear rows, or another pattern of finite bounds, does not fit the bank
    ctl = dict(fam[1][0])
    odd = LR.configure_family(LMPC(3, 2, 0, 2, 5, 5, device=-1), dict(ctl, Fx=ctl["Fx"][:2], Fu=ctl["Fu"][:2], flo=ctl["flo"][:2], fhi=ctl["fhi"][:2]))
    with pytest.raises(MpcxError):
        LMPCHetero([ctrls[0], odd], device=0)
    flo = ctl["flo"].copy(); flo[0, 3] = -INF
    fhi = ctl["fhi"].copy(); fhi[0, 3] = INF
    with pytest.raises(MpcxError):
        LMPCHetero([ctrls[0], LR.configure_family(LMPC(3, 2, 0, 2, 5, 5, device=-1), dict(ctl, flo=flo, fhi=fhi))], device=0)


# ---------------------------------------------------------------------------------------------
# 11. closed loops: the coupled row |x_2 + 0.5 u| <= c on the double integrator
# ---------------------------------------------------------------------------------------------
def _loop_inputs(B=8):
    r = np.random.default_rng(23)
    return 0.1 * r.normal(size=(B, 2)), np.zeros((B, 1))


def _row_violation(x, u, c):
    """largest |x_2(k + 1) + 0.5 cmd_k| - c over the run: the row of step 1 of every tick, on the logged state and command"""
    return float((np.abs(x[1:, :, 1] + 0.5 * u[:, :, 0]) - c).max())


def _follow(c2, res, x_of_tick, u0, ticks, warm, label):
    import torch
    prev, u = None, torch.as_tensor(u0).cuda()
    for k in range(ticks):
        if warm:
            r = c2.optimizeBatch(x_of_tick[k], u, want_active=True, warm=prev, warm_shift=k > 0)
        else:
            r = c2.optimizeBatch(x_of_tick[k], u)
        torch.cuda.synchronize()
        assert torch.equal(res.u[k], r.cmd), (label, k, float((res.u[k] - r.cmd).abs().max()))
        for name in EQUAL:
            assert torch.equal(getattr(res, name)[k], getattr(r, name)), (label, k, name)
        prev, u = r, res.u[k]


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_closed_loop_obeys_the_row_and_equals_the_single_steps(warm):
    lim, ticks = 0.25, 40
    sp = LR.integrator_coupled(ph=10, c=lim)
    x0, u0 = _loop_inputs()
    res = _controller(sp, warm=warm).simulate(x0, u0, ticks, warm=warm)
    x, u = res.x.cpu().numpy(), res.u.cpu().numpy()
    worst = _row_violation(x, u, lim)
    print("closed loop %s: worst |x_2 + 0.5 cmd| - c = %.3e over %d ticks x %d instances" % ("warm" if warm else "cold", worst, ticks, len(x0)))
    assert worst <= lim * 1e-5, worst
    assert (res.status.cpu().numpy() == 0).all()
    assert (np.abs(x[1:, :, 1] + 0.5 * u[:, :, 0]) >= lim * (1 - 1e-5)).any()          # the bound was reached
    _follow(_controller(sp, warm=warm), res, res.x, u0, ticks, warm, "loop")
    # the same loop without the row leaves it by more than twice the bound
    plain = _controller(sp, warm=warm, linear=False).simulate(x0, u0, ticks, warm=warm)
    assert _row_violation(plain.x.cpu().numpy(), plain.u.cpu().numpy(), lim) > 2 * lim


def test_observed_loop_obeys_the_row_on_the_estimate_and_equals_the_single_steps():
    lim, ticks = 0.25, 40
    sp = LR.integrator_coupled(ph=10, c=lim)
    x0, u0 = _loop_inputs()
    c = _controller(sp, warm=True)
    L = c.kalman_gain(0.01 * np.eye(2), 0.04 * np.eye(1))
    r = np.random.default_rng(29)
    res = c.simulate(x0, u0, ticks, warm=True, observer=L, xhat0=x0 + 0.05 * r.normal(size=x0.shape), meas_noise=0.01 * r.normal(size=(ticks, len(x0), 1)))
    # the controller sees the estimate: the row holds on the state it predicts from it, A xhat_k + B cmd_k
    xh, u = res.xhat.cpu().numpy(), res.u.cpu().numpy()
    pred = xh[:-1] @ sp["A"].T + u @ sp["B"].T
    worst = float((np.abs(pred[:, :, 1] + 0.5 * u[:, :, 0]) - lim).max())
    print("observed loop: worst |x_2 + 0.5 cmd| - c on the predicted estimate = %.3e" % worst)
    assert worst <= lim * 1e-5, worst
    assert (res.status.cpu().numpy() == 0).all()
    _follow(_controller(sp, warm=True), res, res.xhat, u0, ticks, True, "observed loop")


# ---------------------------------------------------------------------------------------------
# 12. the C++ front end and pympcxx
# ---------------------------------------------------------------------------------------------
def test_cpp_and_pympcxx_first_move_equal_the_python_front_ends():
    from test_lmpc_linear import build_cpp
    exe = build_cpp()
    env = {k: v for k, v in os.environ.items() if k != "MPCX_DEVICE"}
    out = subprocess.run([exe, "solve"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ linear-row checks passed" in out.stdout
    got = {ln.split()[1]: float.fromhex(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("cmd ")}
    assert set(got) == {"static", "dynamic"}
    sp = LR.integrator_coupled(ph=10, c=0.25)
    res = _controller(sp).optimize(np.zeros(2), np.array([0.3]))
    assert res.status == 0 and got["static"] == got["dynamic"] == float(res.cmd[0]), (got, float(res.cmd[0]).hex())
    import pympcxx
    p = LR.configure(pympcxx.LMPC(*sp["dims"]), sp)
    rp = p.optimize(np.zeros(2), np.array([0.3]))
    assert rp.status == 0 and float(rp.cmd[0]) == float(res.cmd[0])
