"""The terminal cost on the GPU at the project's tolerances -- u* 1e-5 relative, cost 1e-7, active bits equal wherever the
yardstick polished, status equal:

  1. the LQR identity: with P the Riccati solution the first move is -K x0 and the cost 0.5 x0' P x0 on every solve path, whatever ph;
  2. constrained parity with the reference QP plus the terminal block (tests/terminal_ref.py): the integrator under an input box and a rate
     bound, the full-feature controller with a P that is no Riccati solution, xT and Tx, on the MFMA per-instance route and the generic one,
     warm equal to cold;
  3. the bank's condensing on the device against the host's arrays, k = nx across an MFMA k-step and a tile edge, nz on both sides of 16, the
     scratch-block form; four controllers with four different P as LMPCHetero and LMPCBank against each controller alone;
  4. closed loops: the unconstrained loop is x+ = (A - B K) x, every tick is the single-step call bit for bit, also where Tx comes from
     target_map(want_x=True) in an offset-free target loop; a captured graph replays the plain launch;
  5. a controller that set the term and took it back is the controller that never called the setter, bit for bit."""
import dataclasses
import os

import numpy as np
import pytest

import rate_ref as RR
import terminal_ref as TR
from test_lmpc_loop_gpu import _follow
from test_lmpc_offset_free_gpu import _disturbed, _host_gain, _random_of
from test_lmpc_soft_gpu import PATHS, _can_take, _check, _refs, _solve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT = ("cmd", "cost", "status", "solver_status", "is_feasible", "iterations", "polish_rounds", "active_count", "active_lower", "active_upper")
# ... and the fallback forced by a cap on the polish rounds of the two-kernel path: one round where constraints are active, none where none is
# (an unconstrained instance verifies in its first round and would leave the fallback nothing to serve)
ALL_PATHS = PATHS + [("forced fallback", False, 0)]


def _controller(sp, generic=False, fused=None, warm=False, rounds=None, terminal=True, device=0, maximum_iteration=RR.MAXIT):
    from libmpc_amd import LMPC, LParameters
    from libmpc_amd._capi import check
    c = TR.configure(LMPC(*sp["dims"], device=device), sp, maximum_iteration, terminal=terminal)
    if warm:
        c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration, enable_warm_start=1))
    if device >= 0:
        c.debug_force_generic(generic)
        c.debug_use_fused(fused)
    if rounds is not None:
        check(c._lib.mpcx_lmpc_debug_set_rounds(c._h, rounds, 10))
    return c


def _on_every_path(sp, run, label, forced_rounds=1):
    """run(c, label) on every path the controller can take; returns {path: instances lmpc_solve_admm served}"""
    ran = {}
    for pname, generic, fused in ALL_PATHS:
        c = _controller(sp, generic, fused, rounds=forced_rounds if pname == "forced fallback" else None)
        if not _can_take(c, pname):
            continue
        run(c, "%s %s" % (label, pname))              # (the first solve of the handle: nothing served before it)
        ran[pname] = int(c.debug_get("fallback")[0])
    print("%s: fallback served %s" % (label, ran))
    assert {"default", "two-kernel", "generic", "forced fallback"} <= set(ran), ran
    assert ran["forced fallback"] > 0, ran          # the cap did send instances through the fallback kernel
    return ran


def _golden(prefix):
    """a recorded yardstick result (tests/golden/make_terminal_golden.py)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "terminal_oracle.npz"))
    ref = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    m = int(ref["ncon"])
    ref["active_lower"] = np.unpackbits(ref["active_lower"], axis=1, bitorder="little")[:, :m]
    ref["active_upper"] = np.unpackbits(ref["active_upper"], axis=1, bitorder="little")[:, :m]
    return ref


# ---------------------------------------------------------------------------------------------
# 1. the LQR identity
# ---------------------------------------------------------------------------------------------
LQR_CASES = [("integrator", 3), ("integrator", 10), ("stable", 5), ("unstable", 2)]
_FIRST_MOVES = {}


@pytest.mark.parametrize("name,ph", LQR_CASES)
def test_lqr_identity_on_every_solve_path(name, ph):
    sp, Q, R = TR.lqr_spec(name, ph)
    nx, nu = sp["dims"][:2]
    P, K = sp["P"], sp["K"]
    if name == "integrator":
        # the weight from the device's Riccati kernel through the controller's own helper: user column 0 carries the stage weights
        Pd, Kd = _controller(sp, terminal=False).lqr_terminal_cost(step=0)
        print("lqr_terminal_cost against numpy: P %.2e, K %.2e (relative)" % (np.abs(Pd - P).max() / np.abs(P).max(), np.abs(Kd - K).max() / np.abs(K).max()))
        sp = TR.with_terminal(sp, Pd)
    x0 = np.random.default_rng(5).normal(size=(16, nx)); u0 = np.zeros((16, nu))
    cmd = -x0 @ K.T
    cost = 0.5 * np.einsum("bi,ij,bj->b", x0, P, x0)

    def run(c, label):
        r = _solve(c, x0, u0)
        got, gc = r.cmd.cpu().numpy(), r.cost.cpu().numpy()
        err = np.abs(got - cmd).max(axis=1) / np.maximum(np.abs(cmd).max(axis=1), 1e-12)
        cerr = np.abs(gc - cost) / np.maximum(1.0, np.abs(cost))
        print("%s: cmd %.2e, cost %.2e" % (label, err.max(), cerr.max()))
        assert (r.status.cpu().numpy() == 0).all(), label
        assert err.max() <= 1e-5 and cerr.max() <= 1e-7, (label, err.max(), cerr.max())
        _FIRST_MOVES.setdefault((name, ph), got)
    ran = _on_every_path(sp, run, "%s ph=%d" % (name, ph), forced_rounds=0)
    # these controllers are small enough for every form: the fused mat-vec and the one-workgroup form did run, and without a polish round
    # every instance went through the fallback kernel
    assert {"fused", "group"} <= set(ran) and ran["forced fallback"] == 16, ran
    # without the term the horizon is finite and the first move another one, by more than ten times the tolerance above
    r = _solve(_controller(sp, terminal=False), x0, u0)
    assert (np.abs(r.cmd.cpu().numpy() - cmd).max(axis=1) / np.abs(cmd).max(axis=1)).max() > 10 * 1e-5


def test_the_first_move_does_not_depend_on_the_horizon():
    for ph in (3, 10):
        if ("integrator", ph) not in _FIRST_MOVES:
            sp, _, _ = TR.lqr_spec("integrator", ph)
            x0 = np.random.default_rng(5).normal(size=(16, 2))
            _FIRST_MOVES[("integrator", ph)] = _solve(_controller(sp), x0, np.zeros((16, 1))).cmd.cpu().numpy()
    a, b = _FIRST_MOVES[("integrator", 3)], _FIRST_MOVES[("integrator", 10)]
    assert (np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max() <= 1e-5


# ---------------------------------------------------------------------------------------------
# 2. constrained parity with the yardstick
# ---------------------------------------------------------------------------------------------
def test_integrator_under_box_and_rate_bounds_on_every_path():
    sp = TR.integrator_constrained()
    x0, u0, _ = RR.random_batch(sp, 16, 5)
    ref = TR.solve_batch(sp, x0, u0)
    act = ((ref["active_lower"] != 0) | (ref["active_upper"] != 0))[:, ref["neq"]:].sum(axis=1)
    assert (ref["status"] == 0).all() and act.min() >= 5          # the bounds are in reach: this is not the unconstrained problem
    _on_every_path(sp, lambda c, label: _check(_solve(c, x0, u0), ref, sp, label), "integrator")
    # ... and the term moves the solution: the same controller without it is off the yardstick
    r = _solve(_controller(sp, terminal=False), x0, u0)
    assert np.abs(r.cost.cpu().numpy() - ref["cost"]).max() > 1e-3


_FULL = {}


def _full_case():
    if not _FULL:
        sp = TR.full_feature_terminal()
        x0, u0, yconst, ystep, dmeas = TR.full_feature_batch(24)
        refc, refs, refs1 = _golden("fullc_"), _golden("fulls_"), _golden("fulls1_")
        assert np.array_equal(refc["x0"], x0) and np.array_equal(refs["x0"], x0) and np.array_equal(refs["u0"], u0)
        _FULL["case"] = (sp, x0, u0, yconst, ystep, dmeas, refc, refs, refs1)
    return _FULL["case"]


def test_full_feature_controller_with_a_constant_reference_per_instance_on_every_path():
    """P random positive semidefinite of rank 3, xT and Tx non-zero, Bd and Dd present; yref [B, ny]: the MFMA routes' per-instance map"""
    sp, x0, u0, yconst, ystep, dmeas, refc, refs, refs1 = _full_case()
    d = RR.LN.LmpcDims(*sp["dims"])
    act = ((refc["active_lower"] != 0) | (refc["active_upper"] != 0))[:, d.neq:]
    assert act.any(axis=1).sum() >= 12
    _on_every_path(sp, lambda c, label: _check(_solve(c, x0, u0, yref=yconst), refc, sp, label), "full, constant yref")


def test_full_feature_controller_with_per_step_references_and_disturbances_per_instance():
    """the generic route: the terminal target follows the last reference column and the instance's own exogenous input"""
    sp, x0, u0, yconst, ystep, dmeas, refc, refs, refs1 = _full_case()
    kw = _refs(ystep, dmeas)
    _check(_solve(_controller(sp), x0, u0, **kw), refs, sp, "full, per-step yref")
    _check(_solve(_controller(sp, fused=0, rounds=1), x0, u0, **kw), refs, sp, "full, per-step yref, forced fallback")
    # Td is read: with the controller's own disturbance in place of the instances' the answers move
    other = _solve(_controller(sp), x0, u0, yref=kw["yref"])
    assert np.abs(other.cmd.cpu().numpy() - refs["cmd"]).max() > 1e-3


def test_full_feature_warm_start_equals_cold():
    import torch
    sp, x0, u0, yconst, ystep, dmeas, refc, refs, refs1 = _full_case()
    kw = _refs(ystep, dmeas)
    c = _controller(sp, warm=True)
    first = _solve(c, x0, u0, **kw)
    _check(first, refs, sp, "tick 0")
    cmd = refs["cmd"]
    x1 = x0 @ sp["A"].T + cmd @ sp["B"].T + dmeas[:, :, 0] @ sp["Bd"].T
    assert np.array_equal(refs1["x0"], x1) and np.array_equal(refs1["u0"], cmd)
    cold = _solve(_controller(sp), x1, cmd, **kw)
    for shift in (True, False):
        warm = _solve(c, x1, cmd, warm=first, warm_shift=shift, **kw)
        a, b = warm.cmd.cpu().numpy(), cold.cmd.cpu().numpy()
        assert (np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-12)).max() <= 1e-5, shift
        ca, cb = warm.cost.cpu().numpy(), cold.cost.cpu().numpy()
        assert (np.abs(ca - cb) / np.maximum(1.0, np.abs(cb))).max() <= 1e-7, shift
        assert torch.equal(warm.status, cold.status) and torch.equal(warm.solver_status, cold.solver_status)
        assert torch.equal(warm.active_lower, cold.active_lower) and torch.equal(warm.active_upper, cold.active_upper), shift
    _check(cold, refs1, sp, "tick 1")


# ---------------------------------------------------------------------------------------------
# 3. condensing on the device
# ---------------------------------------------------------------------------------------------
def _large_spec(seed):
    sp = RR.rate_spec(seed, *RR.LARGE_DIMS, rate=0.1)
    r = np.random.default_rng(seed + 7)
    F = r.normal(size=(2, 2))
    return TR.with_terminal(sp, F @ F.T, xT=0.1 * r.normal(size=2), Tx=0.2 * r.normal(size=(2, 1)))


# (nx, ny, nu, ph, ch): nx = 15, 16, 17 with ny = 3 -- k = nx ends inside a k-step, on a tile edge, one past it; nz = 15, 17, 18 and 10 (move blocking)
CONDENSE = {"nx15 nz15": (15, 3, 3, 5, 5), "nx16 nz17": (16, 3, 1, 17, 17), "nx17 nz18": (17, 3, 2, 9, 9), "nx17 nz10 blocked": (17, 3, 2, 9, 4),
            "nz160 scratch form": None}


@pytest.mark.parametrize("case", list(CONDENSE))
def test_device_condensing_matches_the_host_set_up(case):
    import torch
    from libmpc_amd import LMPCHetero
    big = CONDENSE[case] is None
    K = 2 if big else 4
    specs = [_large_spec(401 + k) for k in range(K)] if big else [TR.condense_spec(*CONDENSE[case], seed=900 + 10 * k) for k in range(K)]
    hosts = [_controller(sp, device=-1) for sp in specs]
    nx, nu = specs[0]["dims"][:2]
    nz = int(hosts[0].debug_get("dims")[0])
    assert nz == (160 if big else int(case.split("nz")[1].split()[0]))
    host = LMPCHetero(hosts, device=0, condense_on_host=True)
    dev = LMPCHetero(hosts, device=0)
    assert host.debug_get(0, "flags")[1] == 0.0 and dev.debug_get(0, "flags")[1] == 1.0
    # (the tolerances of tests/test_lmpc_hetero.py; its scratch-form case, 200 variables, takes the inverses two orders looser, and so does this one)
    loose = 100.0 if big else 1.0
    for k in range(K):
        for name, tol in (("H", 1e-12), ("Gr", 1e-12), ("Gc", 1e-12), ("Y", 1e-9 * loose), ("rho_b", 1e-9 * loose), ("rho_g", 1e-9 * loose), ("Kinv", 1e-8 * loose)):
            a, b = host.debug_get(k, name), dev.debug_get(k, name)
            scale = max(np.abs(a).max(), 1e-300)
            print("%s controller %d %s: %.2e" % (case, k, name, np.abs(a - b).max() / scale))
            assert np.abs(a - b).max() <= tol * scale, (k, name, np.abs(a - b).max() / scale)
        # the term is in what was compared: the host's Hessian without it is another matrix
        ldz = int(hosts[k].debug_get("dims")[2])
        H0 = _controller(specs[k], device=-1, terminal=False).debug_get("H")
        assert np.abs(H0 - dev.debug_get(k, "H")).max() > 1e-6 * np.abs(H0).max() and H0.size == ldz * ldz
    r = np.random.default_rng(17)
    x0 = 0.3 * r.normal(size=(K, nx)); u0 = r.uniform(-0.2, 0.2, size=(K, nu))
    ra = host.optimizeBatch(x0, u0, want_active=True); rb = dev.optimizeBatch(x0, u0, want_active=True)
    torch.cuda.synchronize()
    assert torch.equal(ra.status, rb.status) and torch.equal(ra.active_lower, rb.active_lower) and torch.equal(ra.active_upper, rb.active_upper)
    np.testing.assert_allclose(ra.cmd.cpu().numpy(), rb.cmd.cpu().numpy(), rtol=1e-8 * loose, atol=1e-10 * loose)
    np.testing.assert_allclose(ra.cost.cpu().numpy(), rb.cost.cpu().numpy(), rtol=1e-8 * loose, atol=1e-8 * loose)


def test_bank_of_four_terminal_weights_equals_four_single_handles():
    import torch
    from libmpc_amd import LMPCBank, LMPCHetero
    base = TR.integrator_constrained()
    # (Weights of this size: with 2.5 times larger ones, eigenvalues near 40 on this plant, two of the 24 instances end as MAX_ITERATION where the
    # yardstick solves them.  The same QP written with output weights alone, no terminal cost, ends the same way to the bit -- the solver's open
    # question of DESIGN.md 3.2, not this term's; DESIGN.md 3.3 has the figures)
    rg = np.random.default_rng(41)
    specs = [base]
    for k in range(3):
        F = rg.normal(size=(2, 2))
        specs.append(TR.with_terminal(base, (k + 1) * 2.0 * F @ F.T, xT=0.1 * rg.normal(size=2), Tx=0.2 * rg.normal(size=(2, 1))))
    B = 24
    x0, u0, _ = RR.random_batch(base, B, 5)
    model = np.arange(B) % 4
    r = LMPCBank([_controller(sp) for sp in specs]).optimizeBatch(x0, u0, model); torch.cuda.synchronize()
    alone = {}
    for k in range(4):
        idx = np.nonzero(model == k)[0]
        one = _controller(specs[k]).optimizeBatch(x0[idx], u0[idx]); torch.cuda.synchronize()
        sel = torch.as_tensor(idx, device=r.cmd.device)
        for name in ("cmd", "cost", "status", "solver_status", "is_feasible", "iterations"):
            assert torch.equal(getattr(r, name)[sel], getattr(one, name)), (k, name)
        alone[k] = (idx, one)
    assert (r.status == 0).all()
    assert not np.allclose(r.cmd.cpu().numpy()[model == 0], r.cmd.cpu().numpy()[model == 3])      # (four weights, four answers)
    hosts = [_controller(sp, device=-1) for sp in specs]
    dev = LMPCHetero(hosts, device=0)
    assert dev.debug_get(0, "flags")[1] == 1.0
    rb = dev.optimizeBatch(x0, u0, model=model); torch.cuda.synchronize()
    assert torch.equal(rb.status, r.status)
    cmd, cost = r.cmd.cpu().numpy(), r.cost.cpu().numpy()
    err = np.abs(rb.cmd.cpu().numpy() - cmd).max(axis=1) / np.maximum(np.abs(cmd).max(axis=1), 1e-12)
    assert err.max() <= 1e-5 and (np.abs(rb.cost.cpu().numpy() - cost) / np.maximum(1.0, np.abs(cost))).max() <= 1e-7
    # ... and each against its own yardstick
    for k in range(4):
        idx, one = alone[k]
        _check(_solve(_controller(specs[k]), x0[idx], u0[idx]), TR.solve_batch(specs[k], x0[idx], u0[idx]), specs[k], "controller %d alone" % k)


def test_bank_takes_the_term_in_every_controller_or_in_none():
    """(a GPU test although the rule is decided on the host: mpcx_lmpc_hetero_create_ex asks for a device before it looks at its controllers)"""
    from libmpc_amd import LMPCHetero, MpcxError
    sp = TR.integrator_constrained()
    a, b = _controller(sp, device=-1), _controller(sp, device=-1, terminal=False)
    for pair in ((a, b), (b, a)):
        for on_host in (False, True):
            with pytest.raises(MpcxError) as e:
                LMPCHetero(list(pair), device=0, condense_on_host=on_host)
            assert "whether it has a terminal cost" in str(e.value)
    LMPCHetero([a, _controller(TR.with_terminal(sp, 3.0 * sp["P"]), device=-1)], device=0)
    # one batched Riccati call for a bank's weights
    het = LMPCHetero([b, _controller(sp, device=-1, terminal=False)], device=0)
    X, K = het.lqr_terminal_costs(step=0)
    assert tuple(X.shape) == (2, 2, 2) and tuple(K.shape) == (2, 1, 2)
    # (tests/test_dare_gpu.py holds the kernel to 1e-10; the numpy value iteration it is compared with here stops at 1e-13 steps, good to some 1e-9)
    assert np.abs(X[0].cpu().numpy() - sp["P"]).max() <= 1e-7 * np.abs(sp["P"]).max()


# ---------------------------------------------------------------------------------------------
# 4. closed loops and graph capture
# ---------------------------------------------------------------------------------------------
def test_unconstrained_loop_is_the_lqr_loop_and_every_tick_the_single_step_call():
    import torch
    ticks, B = 30, 8
    sp, Q, R = TR.lqr_spec("integrator", 10)
    A, Bm, K = sp["A"], sp["B"], sp["K"]
    nx, nu = 2, 1
    x0 = np.random.default_rng(61).normal(size=(B, nx)); u0 = np.zeros((B, nu))
    res = _controller(sp).simulate(x0, u0, ticks, warm=False)
    assert (res.status.cpu().numpy() == 0).all()
    x, u = res.x.cpu().numpy(), res.u.cpu().numpy()
    # x_{k+1} = (A - B K) x_k.  Each tick's command is -K x_k of the loop's own state within the u* tolerance: |du_k|_2 <= sqrt(nu) 1e-5 |u_k|_inf,
    # and the deviation e_k from the nominal trajectory obeys e_{k+1} = (A - B K) e_k + B du_k, so
    # |e_{k+1}|_2 <= |A - B K|_2 |e_k|_2 + |B|_2 |du_k|_2, compounded over the ticks (rounding of the plant step is ten orders below)
    Acl = A - Bm @ K
    na, nb = np.linalg.norm(Acl, 2), np.linalg.norm(Bm, 2)
    nom = x0.copy()
    bound = np.zeros(B)
    for k in range(ticks):
        assert (np.linalg.norm(x[k] - nom, axis=1) <= bound + 1e-13).all(), (k, np.linalg.norm(x[k] - nom, axis=1).max(), bound.max())
        bound = na * bound + nb * np.sqrt(nu) * 1e-5 * np.abs(u[k]).max(axis=1)
        nom = nom @ Acl.T
    assert (np.linalg.norm(x[ticks] - nom, axis=1) <= bound + 1e-13).all()
    assert np.abs(x[ticks]).max() < np.abs(x0).max()                # (it is the stabilising loop)
    _follow(_controller(sp), res, u0, ticks, "lqr loop")
    # the same step replayed as a captured graph
    c = _controller(sp)
    batch, out, keep = c.make_batch(x0, u0)
    side = torch.cuda.Stream(device=0)
    g = c.make_graph(batch, side)
    c.launch_graph(g, side); side.synchronize()
    assert torch.equal(out.cmd, res.u[0]) and torch.equal(out.cost, res.cost[0])
    c.destroy_graph(g)


def test_constrained_warm_loop_equals_the_single_steps():
    sp = TR.integrator_constrained()
    x0, u0, _ = RR.random_batch(sp, 8, 5)
    ticks = 12
    res = _controller(sp, warm=True).simulate(x0, u0, ticks, warm=True)
    assert (res.status.cpu().numpy() == 0).all() and int(res.active_count.max()) > 0
    _follow(_controller(sp, warm=True), res, u0, ticks, "constrained warm loop", warm=True)


def test_offset_free_target_loop_whose_terminal_target_follows_the_estimate():
    """Tx = the first ny + ndu columns of map_x: x_T = Tx [r; dhat_k] is the steady state the loop's own targets belong to, and it moves with the
    disturbance estimate through the solve's per-instance exogenous input -- no new plumbing.  Every tick is the single-step call bit for bit."""
    import torch
    make, inputs, model = _random_of(nx=3, nu=2, ndu=1, ny=2)
    nx, nu, ndu, ny = 3, 2, 1, 2
    B, ticks = 22, 7
    x0, u0, _ = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 85)
    rng = np.random.default_rng(86)
    yref = 0.3 * rng.normal(size=(B, ny))
    ubar = np.zeros((B, nu))
    L = _host_gain(model)
    F = rng.normal(size=(nx, nx))
    P = 4.0 * F @ F.T

    def build():
        c = make()
        Tu, Txm = c.target_map(want_x=True)
        assert Txm.shape == (nx, ny + ndu + nu)
        assert c.setTerminalCost(P, None, Txm[:, :ny + ndu])
        return c, Tu
    c, T = build()
    kw = dict(warm=False, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, yref=yref, uref=ubar)
    res = c.simulate(x0, u0, ticks, target=T, **kw)
    assert not torch.equal(res.dhat[1], res.dhat[0])
    _follow(build()[0], dataclasses.replace(res, x=res.xhat), u0, ticks, "target loop", refs_of_tick=lambda k: dict(dmeas=res.dhat[k], uref=res.us[k]), yref=yref)
    plain = make().simulate(x0, u0, ticks, target=T, **kw)
    assert not torch.equal(plain.u, res.u)


# ---------------------------------------------------------------------------------------------
# 5. no call is the parent
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
def test_set_and_taken_back_is_never_set(generic):
    import torch
    sp, x0, u0, yconst, ystep, dmeas, refc, refs, refs1 = _full_case()
    kw = _refs(ystep, dmeas) if generic else dict(yref=yconst)
    never = _solve(_controller(sp, terminal=False), x0, u0, want_sequence=True, **kw)
    back = _controller(sp)
    assert back.setTerminalCost(None)
    null = _controller(sp, terminal=False)
    assert null.setTerminalCost(None)
    for label, c in (("taken back", back), ("null", null)):
        r = _solve(c, x0, u0, want_sequence=True, **kw)
        for name in RESULT + ("seq_state", "seq_input", "seq_output"):
            assert torch.equal(getattr(r, name), getattr(never, name)), (label, name)
    with_term = _solve(_controller(sp), x0, u0, **kw)
    assert not torch.equal(with_term.cmd, never.cmd)
