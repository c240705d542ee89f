"""Soft constraints on the GPU: every solve path, strict infeasibility, working sets past nz rows, all three kinds of soft
row beside hard box and rate rows, the forced fallback and plain ADMM, banks, a noisy observed closed loop, the +inf no-op and the penalty's
monotonicity -- against the slack-augmented reference QP (tests/soft_ref.py) at the project's tolerances: u* 1e-5 relative, cost 1e-7,
active bits equal wherever the yardstick polished, status equal.  Instances the yardstick leaves unpolished are at most a quarter of any
batch (the seeds were chosen on the CPU for that) and are compared loosely, as helpers.assert_matches_oracle does."""
import os

import numpy as np
import pytest

import rate_ref as RR
import soft_ref as SR
from helpers import assert_matches_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
# (name, debug_force_generic, debug_use_fused) -- the five paths of test_lmpc_rate_bounds_gpu.py
PATHS = [("default", False, None), ("two-kernel", False, 0), ("generic", True, None), ("fused", False, 1), ("group", False, 2)]
EQUAL = ("cost", "status", "solver_status", "iterations", "polish_rounds", "active_count")
VMAX = 0.3


def _controller(sp, generic=False, fused=None, warm=False, soft=True, strict=False, rounds=None, polish=1, device=0, maximum_iteration=RR.MAXIT):
    from libmpc_amd import LMPC, LParameters
    from libmpc_amd._capi import check
    c = SR.configure(LMPC(*sp["dims"], device=device), sp, maximum_iteration, soft=soft)
    if warm or not polish:
        c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration, enable_warm_start=int(warm), polish=polish))
    if device >= 0:
        c.debug_force_generic(generic)
        c.debug_use_fused(fused)
    if strict:
        c.setStrictInfeasibility(True)
    if rounds is not None:
        check(c._lib.mpcx_lmpc_debug_set_rounds(c._h, rounds, 10))
    return c


def _can_take(c, pname):
    flags = c.debug_get("flags")
    return not ((pname == "fused" and int(flags[2]) != 1) or (pname == "group" and int(flags[1]) != 1))


def _solve(c, x0, u0, **kw):
    import torch
    r = c.optimizeBatch(x0, u0, want_active=True, **kw)
    torch.cuda.synchronize()
    return r


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _check(r, ref, sp, label):
    """cmd, cost and status of every instance, solver_status and the compared active bits of the polished ones"""
    pol = ref["polished"] == 1
    assert pol.mean() >= 0.75, (label, pol.mean())
    try:
        assert_matches_oracle(r, ref, ref["neq"], ref["ncon"], check_active=False)
    except AssertionError as e:
        raise AssertionError((label,) + e.args) from e
    st = r.status.cpu().numpy(); sst = r.solver_status.cpu().numpy()
    assert np.array_equal(st, ref["status"]), (label, np.nonzero(st != ref["status"])[0][:8])
    assert np.array_equal(sst[pol], ref["solver_status"][pol]), label
    keep = RR.compared_rows(sp)
    m = int(ref["ncon"])
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == (ref["active_lower"][:, keep] != 0)).all(axis=1) & (up[:, keep] == (ref["active_upper"][:, keep] != 0)).all(axis=1)
    assert same[pol].all(), (label, int(np.argmin(same | ~pol)))
    return r.active_count.cpu().numpy()


def _refs(yref=None, dmeas=None):
    kw = {}
    if yref is not None:
        kw["yref"] = np.ascontiguousarray(yref.transpose(0, 2, 1)) if yref.ndim == 3 else yref
    if dmeas is not None:
        kw["dmeas"] = np.ascontiguousarray(dmeas.transpose(0, 2, 1))
    return kw


# ---------------------------------------------------------------------------------------------
# 1. the integrator with a soft velocity bound on steps 0 .. ph: every path, strict mode too
# ---------------------------------------------------------------------------------------------
_INTEGRATOR = {}


def _integrator_case(rho):
    if rho not in _INTEGRATOR:
        sp = SR.integrator_soft(rho=rho)
        x0, u0, _ = RR.random_batch(sp, 16, 5)
        _INTEGRATOR[rho] = (sp, x0, u0, SR.solve_batch(sp, x0, u0), SR.hard_infeasible(sp, x0, u0))
    return _INTEGRATOR[rho]


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("rho", [10.0, 100.0])
def test_integrator_parity_on_every_path(rho, strict):
    sp, x0, u0, ref, infeasible = _integrator_case(rho)
    # most of the batch is infeasible with the bound hard: x0 itself is outside it
    assert infeasible.sum() >= 8 and np.array_equal(infeasible, np.abs(x0[:, 1]) > VMAX)
    assert (ref["status"] == 0).all()
    d = RR.LN.LmpcDims(*sp["dims"])
    row0 = d.neq + 1                                   # the velocity row of step 0
    assert np.array_equal((ref["active_lower"][:, row0] != 0) | (ref["active_upper"][:, row0] != 0), infeasible)
    ran = []
    for pname, generic, fused in PATHS:
        c = _controller(sp, generic, fused, strict=strict)
        if not _can_take(c, pname):
            continue
        r = _solve(c, x0, u0)
        _check(r, ref, sp, "rho=%g %s%s" % (rho, pname, " strict" if strict else ""))
        assert (r.status.cpu().numpy() == 0).all() and (r.is_feasible.cpu().numpy() == 1).all()
        ran.append(pname)
    assert {"default", "two-kernel", "generic"} <= set(ran)
    # the same controller with the rows hard: the instances whose x0 is outside are not solved (MAX_ITERATION by default, INFEASIBLE in strict mode)
    hard = _solve(_controller(sp, soft=False, strict=strict), x0, u0)
    assert np.array_equal(hard.status.cpu().numpy() != 0, infeasible)
    assert (hard.status.cpu().numpy()[infeasible] == (2 if strict else 1)).all()


# ---------------------------------------------------------------------------------------------
# 2. more active soft rows than a working set could hold before (nz = 3)
# ---------------------------------------------------------------------------------------------
def _golden(prefix):
    """a recorded yardstick result (tests/golden/make_soft_golden.py)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "soft_oracle.npz"))
    ref = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    m = int(ref["ncon"])
    ref["active_lower"] = np.unpackbits(ref["active_lower"], axis=1, bitorder="little")[:, :m]
    ref["active_upper"] = np.unpackbits(ref["active_upper"], axis=1, bitorder="little")[:, :m]
    return ref


@pytest.mark.parametrize("forced", [False, True], ids=["default path", "forced fallback"])
def test_more_active_soft_rows_than_decision_variables(forced):
    sp, x0, u0 = SR.large_case()
    ref = _golden("large_")
    assert np.array_equal(ref["x0"], x0) and np.array_equal(ref["u0"], u0) and float(ref["rho"]) == SR.LARGE_RHO
    assert np.allclose(np.abs(x0[:, 1]), 3 * VMAX, rtol=1e-15)
    assert (ref["n_soft_active"] >= 29).all() and (ref["polished"] == 1).all()
    c = _controller(sp, fused=0 if forced else None, rounds=1 if forced else None)
    assert int(c.debug_get("dims")[0]) == 3 and int(c.debug_get("ws_limit")[0]) == 44
    r = _solve(c, x0, u0)
    ac = _check(r, ref, sp, "41 soft rows" + (" forced" if forced else ""))
    # (the yardstick's n_active also counts the reference's pinned delta-u rows behind the control horizon, which move blocking has eliminated here)
    assert (ac >= ref["n_soft_active"]).all() and (ac <= ref["n_soft_active"] + 3).all() and ac.min() >= 29
    if forced:
        assert (r.iterations.cpu().numpy() > 0).all()


# ---------------------------------------------------------------------------------------------
# 3. state, output and scalar rows soft at three weights, box and rate rows hard, per-step references, per-instance disturbances
# ---------------------------------------------------------------------------------------------
_FULL = {}


def _full_case():
    if not _FULL:
        sp = SR.full_feature_soft()
        x0, u0, yref, dmeas = RR.full_feature_batch(24)
        ref = _golden("full0_")                       # (these yardstick solves take a minute: recorded)
        assert np.array_equal(ref["x0"], x0) and np.array_equal(ref["u0"], u0)
        _FULL["case"] = (sp, x0, u0, yref, dmeas, ref)
    return _FULL["case"]


def test_full_feature_controller_on_every_path():
    sp, x0, u0, yref, dmeas, ref = _full_case()
    d = RR.LN.LmpcDims(*sp["dims"])
    act = ((ref["active_lower"] != 0) | (ref["active_upper"] != 0))[:, d.neq:]
    kinds = np.stack([act[:, :d.off_y].any(axis=1), act[:, d.off_y:d.off_du].any(axis=1), act[:, d.off_du:d.off_s].any(axis=1), act[:, d.off_s:].any(axis=1)])
    assert kinds.all(axis=0).sum() >= 3 and ref["n_soft_active"].max() >= 4
    ran = []
    for pname, generic, fused in PATHS:
        c = _controller(sp, generic, fused)
        if not _can_take(c, pname):
            continue
        _check(_solve(c, x0, u0, **_refs(yref, dmeas)), ref, sp, "full " + pname)
        ran.append(pname)
    assert {"default", "two-kernel", "generic"} <= set(ran)


def test_full_feature_warm_start_equals_cold():
    import torch
    sp, x0, u0, yref, dmeas, ref = _full_case()
    kw = _refs(yref, dmeas)
    c = _controller(sp, warm=True)
    first = _solve(c, x0, u0, **kw)
    _check(first, ref, sp, "tick 0")
    ref1 = _golden("full1_")
    cmd = ref["cmd"]                          # the next tick from the yardstick's command (the GPU's is equal to 1e-5): the same problem on every run
    x1 = x0 @ sp["A"].T + cmd @ sp["B"].T + dmeas[:, :, 0] @ sp["Bd"].T
    assert np.array_equal(ref1["x0"], x1) and np.array_equal(ref1["u0"], cmd)
    cold = _solve(_controller(sp), x1, cmd, **kw)
    for shift in (True, False):
        warm = _solve(c, x1, cmd, warm=first, warm_shift=shift, **kw)
        a, b = warm.cmd.cpu().numpy(), cold.cmd.cpu().numpy()
        assert (np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-12)).max() <= 1e-5, shift
        ca, cb = warm.cost.cpu().numpy(), cold.cost.cpu().numpy()
        assert (np.abs(ca - cb) / np.maximum(1.0, np.abs(cb))).max() <= 1e-7, shift
        assert torch.equal(warm.status, cold.status) and torch.equal(warm.solver_status, cold.solver_status)
        assert torch.equal(warm.active_lower, cold.active_lower) and torch.equal(warm.active_upper, cold.active_upper), shift
    _check(cold, ref1, sp, "tick 1")


# ---------------------------------------------------------------------------------------------
# 4. the forced fallback and plain ADMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["integrator", "full"])
def test_forced_fallback_lands_on_the_yardstick(case):
    if case == "integrator":
        sp, x0, u0, ref, _ = _integrator_case(100.0); kw = {}
    else:
        sp, x0, u0, yref, dmeas, ref = _full_case(); kw = _refs(yref, dmeas)
    c = _controller(sp, fused=0, rounds=1)
    r = _solve(c, x0, u0, **kw)
    it = r.iterations.cpu().numpy()
    assert (it > 0).mean() >= 0.5, (it > 0).mean()          # one polish round is not enough for most: they went through lmpc_solve_admm
    _check(r, ref, sp, case + " forced fallback")


def test_plain_admm_with_the_prox():
    """polish = false: the z-update of a soft row is the prox of its penalty.  At the looseness of test_lmpc_gpu.test_admm_only_mode (2e-2 on
    u*), the cost -- penalty from its definition at the iterate -- to 1e-3"""
    sp, x0, u0, ref, _ = _integrator_case(10.0)
    r = _solve(_controller(sp, polish=0, maximum_iteration=1000), x0, u0)
    it = r.iterations.cpu().numpy()
    assert (r.status.cpu().numpy() == 0).all() and it.min() >= 10 and it.max() <= 1000
    err = np.abs(r.cmd.cpu().numpy() - ref["cmd"]).max(axis=1) / np.maximum(np.abs(ref["cmd"]).max(axis=1), 1e-12)
    cerr = np.abs(r.cost.cpu().numpy() - ref["cost"]) / np.maximum(1.0, np.abs(ref["cost"]))
    print("plain ADMM: worst relative error of u* %.2e, of the cost %.2e, iterations up to %d" % (err.max(), cerr.max(), it.max()))
    assert err.max() < 2e-2 and cerr.max() < 1e-3


def test_cost_from_its_definition_carries_the_penalty():
    """A regularised Hessian: lmpc_solve leaves the cost to lmpc_cost_mfma (the penalty rides in the record's constant), the generic path and
    the bank's path add 0.5 sum g_soft lambda^2 themselves.  What is checked is the cost (and u*) of every instance the GPU verified and the
    yardstick polished, at the project's tolerances -- without the penalty the cost is off by up to 2.4.  Not checked: that every instance
    is solved.  On this controller (no input weights, a singular Hessian) 4 of 16 instances stay at MAX_ITERATION with an ADMM iterate:
    their polish does not verify and ADMM does not reach its residual test in 4000 iterations; the cause is not established (DESIGN.md 3.2,
    "not covered, and open").  The count is pinned below."""
    import torch
    from libmpc_amd import LMPCHetero
    specs = [SR.singular_soft(rho=w) for w in (100.0, 200.0)]
    x0, u0, _ = RR.random_batch(specs[0], 16, 5)
    x0 *= 0.3                                     # excursions of the size of the bound
    refs = [SR.solve_batch(sp, x0, u0) for sp in specs]
    assert refs[0]["n_soft_active"].max() >= 5 and (np.abs(x0[:, 1]) > VMAX).sum() >= 4
    assert (0.5 * 100.0 * (np.maximum(np.abs(x0[:, 1]) - VMAX, 0.0) ** 2)).max() > 1.0

    def compare(r, ref, idx, label, most_unsolved):
        ok = (r.status.cpu().numpy()[idx] == 0) & (r.active_count.cpu().numpy()[idx] > 0) & (ref["polished"][idx] == 1) & (ref["status"][idx] == 0)
        cost = r.cost.cpu().numpy()[idx]; cmd = r.cmd.cpu().numpy()[idx]
        cerr = np.abs(cost - ref["cost"][idx]) / np.maximum(1.0, np.abs(ref["cost"][idx]))
        err = np.abs(cmd - ref["cmd"][idx]).max(axis=1) / np.maximum(np.abs(ref["cmd"][idx]).max(axis=1), 1e-12)
        unsolved = int((r.status.cpu().numpy()[idx] != 0).sum())
        print("%s: %d of %d instances unsolved; %d verified and polished by the yardstick: cost to %.2e, u* to %.2e" % (label, unsolved, len(idx), ok.sum(), cerr[ok].max(), err[ok].max()))
        assert ok.sum() >= len(idx) // 2 and cerr[ok].max() <= 1e-7 and err[ok].max() <= 1e-5, label
        # the count of unsolved instances as measured when this was written: more of them is a regression (fewer is welcome)
        assert unsolved <= most_unsolved, (label, unsolved)
        assert (r.status.cpu().numpy()[idx] <= 1).all() and (r.is_feasible.cpu().numpy()[idx] == 1).all(), label      # SUCCESS or MAX_ITERATION, flagged
        return ok
    sp, ref = specs[0], refs[0]
    every = np.arange(16)
    for label, kw in (("default", {}), ("two-kernel", dict(fused=0)), ("generic", dict(generic=True))):
        c = _controller(sp, **kw)
        assert int(c.debug_get("flags")[0]) == 1 and int(c.debug_get("dims")[11]) == 1
        ok = compare(_solve(c, x0, u0), ref, every, "singular " + label, 4)
        assert (ref["n_soft_active"][ok] > 0).sum() >= 8          # the compared instances carry a penalty
    hosts = [_controller(q, device=-1) for q in specs]
    model = every % 2
    for on_host in (True, False):
        r = LMPCHetero(hosts, device=0, condense_on_host=on_host).optimizeBatch(x0, u0, model=model, want_active=True)
        torch.cuda.synchronize()
        for k in range(2):
            compare(r, refs[k], np.nonzero(model == k)[0], "bank (host %s) controller %d" % (on_host, k), (2, 3)[k])


# ---------------------------------------------------------------------------------------------
# 5. banks
# ---------------------------------------------------------------------------------------------
BANK_RHO = (5.0, 10.0, 40.0, 100.0)


def test_bank_of_four_weights_equals_four_single_handles():
    """LMPCBank groups by controller: every instance bit for bit what its own controller returns.  LMPCHetero: the device's condensing
    against the host's array by array (g_soft and the diagonal included), the two banks against each other and against the yardstick."""
    import torch
    from libmpc_amd import LMPCBank, LMPCHetero
    specs = [SR.integrator_soft(rho=w) for w in BANK_RHO]
    B = 24
    x0, u0, _ = RR.random_batch(specs[0], B, 5)
    model = np.arange(B) % 4
    ctrls = [_controller(sp) for sp in specs]
    r = LMPCBank(ctrls).optimizeBatch(x0, u0, model); torch.cuda.synchronize()
    for k in range(4):
        idx = np.nonzero(model == k)[0]
        one = _controller(specs[k]).optimizeBatch(x0[idx], u0[idx]); torch.cuda.synchronize()
        sel = torch.as_tensor(idx, device=r.cmd.device)
        for name in ("cmd", "cost", "status", "solver_status", "is_feasible", "iterations"):
            assert torch.equal(getattr(r, name)[sel], getattr(one, name)), (k, name)
    assert (r.status == 0).all()
    hosts = [_controller(sp, device=-1) for sp in specs]
    host = LMPCHetero(hosts, device=0, condense_on_host=True)
    dev = LMPCHetero(hosts, device=0)
    assert host.debug_get(0, "flags")[1] == 0.0 and dev.debug_get(0, "flags")[1] == 1.0
    for k in range(4):
        for name, tol in (("H", 1e-12), ("Gr", 1e-12), ("Gc", 1e-12), ("Y", 1e-9), ("rho_b", 1e-9), ("rho_g", 1e-9), ("Kinv", 1e-8)):
            a, b = host.debug_get(k, name), dev.debug_get(k, name)
            assert np.abs(a - b).max() <= tol * max(np.abs(a).max(), 1e-300), (k, name)
        gs = dev.debug_get(k, "g_soft")
        assert np.array_equal(gs, hosts[k].debug_get("g_soft")) and np.array_equal(gs, host.debug_get(k, "g_soft")) and gs.max() == 1.0 / BANK_RHO[k]
        # the step-0 row has no coefficients: its diagonal entry is 1 / rho exactly, on the device as on the host
        ldz, ldy = int(hosts[k].debug_get("dims")[2]), int(hosts[k].debug_get("dims")[4])
        assert dev.debug_get(k, "Y").reshape(ldy, ldy)[ldz, ldz] == 1.0 / BANK_RHO[k] == hosts[k].debug_get("Y").reshape(ldy, ldy)[ldz, ldz]
    ra = host.optimizeBatch(x0, u0, model=model, want_active=True); rb = dev.optimizeBatch(x0, u0, model=model, want_active=True)
    torch.cuda.synchronize()
    assert torch.equal(ra.status, rb.status) and torch.equal(ra.active_lower, rb.active_lower) and torch.equal(ra.active_upper, rb.active_upper)
    np.testing.assert_allclose(ra.cmd.cpu().numpy(), rb.cmd.cpu().numpy(), rtol=1e-8, atol=1e-10)
    parts = [(np.nonzero(model == k)[0], SR.solve_batch(specs[k], x0[model == k], u0[model == k])) for k in range(4)]
    ref = {"neq": parts[0][1]["neq"], "ncon": parts[0][1]["ncon"]}
    for key, first in parts[0][1].items():
        if isinstance(first, np.ndarray) and first.ndim >= 1 and len(first) == len(parts[0][0]) and key != "soft_rows":
            ref[key] = np.zeros((B,) + first.shape[1:], dtype=first.dtype)
            for idx, p in parts:
                ref[key][idx] = p[key]
    _check(rb, ref, specs[0], "bank")
    _check(ra, ref, specs[0], "bank condensed on the host")
    np.testing.assert_allclose(r.cmd.cpu().numpy(), rb.cmd.cpu().numpy(), rtol=1e-9, atol=1e-11)


def test_bank_takes_one_pattern_of_soft_rows():
    """(a GPU test although the rule is decided on the host: mpcx_lmpc_hetero_create_ex refuses a call without a device -- "no such HIP device" --
    before it looks at its controllers, so the rule cannot be reached on a machine without one)"""
    from libmpc_amd import LMPCHetero, MpcxError
    a = _controller(SR.integrator_soft(rho=10.0), device=-1)
    odd = _controller(SR.integrator_soft(rho=10.0), device=-1, soft=False)      # its step-0 row is a feasibility row: another number of general rows
    with pytest.raises(MpcxError) as e:
        LMPCHetero([a, odd], device=0)
    assert "differs from controller 0" in str(e.value)
    # the same rows in both, fewer of them soft in the second
    sp1 = dict(SR.integrator_soft(rho=10.0), first=1)
    full, part = _controller(sp1, device=-1), _controller(sp1, device=-1, soft=False)
    assert part.setSoftConstraintWeights([INF, 10.0], None, None, (3, 10))
    assert full.debug_get("dims")[1] == part.debug_get("dims")[1] and (full.debug_get("g_soft") > 0).sum() > (part.debug_get("g_soft") > 0).sum() > 0
    for on_host in (False, True):
        with pytest.raises(MpcxError) as e:
            LMPCHetero([full, part], device=0, condense_on_host=on_host)
        assert "which constraint rows are soft" in str(e.value)
    # different weights on one pattern are what a bank is for
    LMPCHetero([full, _controller(dict(SR.integrator_soft(rho=77.0), first=1), device=-1)], device=0)


# ---------------------------------------------------------------------------------------------
# 6. a noisy observed closed loop
# ---------------------------------------------------------------------------------------------
def test_noisy_observed_loop_stays_solvable_and_equals_the_single_steps():
    import torch
    ticks, B = 30, 8
    sp = SR.integrator_soft(rho=100.0)
    r0 = np.random.default_rng(23)
    x0 = 0.1 * r0.normal(size=(B, 2)); u0 = np.zeros((B, 1))
    rn = np.random.default_rng(29)
    kw = dict(xhat0=x0 + 0.05 * rn.normal(size=x0.shape), meas_noise=0.05 * rn.normal(size=(ticks, B, 1)), noise=0.02 * rn.normal(size=(ticks, B, 2)))
    c = _controller(sp, warm=True)
    L = c.kalman_gain(0.01 * np.eye(2), 0.04 * np.eye(1))
    res = c.simulate(x0, u0, ticks, warm=True, observer=L, **kw)
    assert (res.status.cpu().numpy() == 0).all()
    xhat = res.xhat.cpu().numpy()[:ticks]                                  # what the solve of tick k read as x0
    outside = np.abs(xhat[:, :, 1]) > VMAX * (1 + 1e-6)
    print("observed loop: %d of %d solves started outside the velocity bound, by up to %.3e" % (outside.sum(), outside.size, (np.abs(xhat[:, :, 1]) - VMAX).max()))
    assert outside.sum() >= 5
    # every tick is the single-step call on the logged inputs
    c2 = _controller(sp, warm=True)
    prev, u = None, torch.as_tensor(u0).cuda()
    for k in range(ticks):
        r = c2.optimizeBatch(res.xhat[k], u, want_active=True, warm=prev, warm_shift=k > 0)
        torch.cuda.synchronize()
        assert torch.equal(res.u[k], r.cmd), (k, float((res.u[k] - r.cmd).abs().max()))
        for name in EQUAL:
            assert torch.equal(getattr(res, name)[k], getattr(r, name)), (k, name)
        prev, u = r, res.u[k]
    # the same loop with the bound hard loses ticks: that is what the soft rows are for
    hard = _controller(sp, warm=True, soft=False).simulate(x0, u0, ticks, warm=True, observer=L, **kw)
    assert (hard.status.cpu().numpy() != 0).any()


# ---------------------------------------------------------------------------------------------
# 7. +inf is no call; the violation shrinks as the weight grows
# ---------------------------------------------------------------------------------------------
def test_infinite_weight_is_no_call():
    import torch
    sp = dict(SR.integrator_soft(), first=1)                              # (hard from step 1: every instance is solvable)
    x0, u0, _ = RR.random_batch(sp, 16, 5)
    x0[:, 1] *= 0.2
    plain = _solve(_controller(sp, soft=False), x0, u0, want_sequence=True)
    c = _controller(sp, soft=False)
    assert c.setSoftConstraintWeights([INF, INF], [INF], INF)
    back = _controller(sp)
    assert back.setSoftConstraintWeights([INF, INF], None, None)
    for label, ctl in (("+inf", c), ("taken back", back)):
        r = _solve(ctl, x0, u0, want_sequence=True)
        for name in ("cmd", "cost", "status", "solver_status", "iterations", "polish_rounds", "active_count", "active_lower", "active_upper", "seq_state", "seq_input"):
            assert torch.equal(getattr(r, name), getattr(plain, name)), (label, name)
    assert (plain.status == 0).all() and int(plain.active_count.max()) > 0


def test_violation_does_not_grow_with_the_weight():
    """per instance, along rho = 1, 10, 100, 1e3: the largest violation of the velocity bound over the horizon does not grow, and neither
    does the sum of squared violations (the penalty method's own monotonicity; both to 1e-9, the solutions being exact to round-off)"""
    sp0 = SR.integrator_soft()
    x0, u0, _ = RR.random_batch(sp0, 16, 5)
    worst, total = [], []
    for rho in (1.0, 10.0, 100.0, 1e3):
        r = _solve(_controller(SR.integrator_soft(rho=rho)), x0, u0, want_sequence=True)
        assert (r.status.cpu().numpy() == 0).all(), rho
        v = np.maximum(np.abs(r.seq_state.cpu().numpy()[:, :, 1]) - VMAX, 0.0)
        worst.append(v.max(axis=1)); total.append((v[:, 1:] ** 2).sum(axis=1))
    worst, total = np.array(worst), np.array(total)
    print("largest violation along rho: %s; sum of squares past step 0: %s" % (worst.max(axis=1), total.max(axis=1)))
    assert (np.diff(worst, axis=0) <= 1e-9).all() and (np.diff(total, axis=0) <= 1e-9).all()
    assert (total[0] > 0).any() and (total[-1] < total[0]).any()
