"""Input-rate bounds on the GPU: every solve path, warm starts, infeasibility, a heterogeneous bank and the closed loops against the
reference QP with finite delta-u rows (tests/rate_ref.py), at the tolerances of BASELINE.json: u* 1e-5 relative, cost 1e-7, active bits
equal wherever the oracle polished, status and solver_status equal.  Every batch has the oracle polished on at least 90 % of its
instances (the seeds were chosen on the CPU for that), and all polished instances are compared."""
import os
import subprocess

import numpy as np
import pytest

import rate_ref as RR
from helpers import assert_matches_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, debug_force_generic, debug_use_fused) -- the five paths of test_lmpc_shapes_gpu.py
PATHS = [("default", False, None), ("two-kernel", False, 0), ("generic", True, None), ("fused", False, 1), ("group", False, 2)]
EQUAL = ("cost", "status", "solver_status", "iterations", "polish_rounds", "active_count")


def _controller(sp, generic=False, fused=None, warm=False, rate=True, maximum_iteration=RR.MAXIT):
    from libmpc_amd import LMPC, LParameters
    c = RR.configure(LMPC(*sp["dims"], device=0), sp, maximum_iteration, rate=rate)
    if warm:
        c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration, enable_warm_start=1))
    c.debug_force_generic(generic)
    c.debug_use_fused(fused)
    return c


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
    keep = RR.compared_rows(sp)
    m = int(ref["ncon"])
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == (ref["active_lower"][:, keep] != 0)).all(axis=1) & (up[:, keep] == (ref["active_upper"][:, keep] != 0)).all(axis=1)
    assert same[pol].all(), (label, int(np.argmin(same | ~pol)))
    return r.active_count.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# 1. the smallest shape: delta_0 (one entry and the -lastU offset) and delta_1 (two entries)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smallest():
    sp = RR.rate_spec(102, 2, 1, 0, 1, 2, 2, rate=0.1)
    x0, u0, _ = RR.random_batch(sp, 65, 7)                 # lastU random and non-zero
    r = np.random.default_rng(8)
    yref = r.choice([-1.0, 1.0], size=(65, 1)) * r.uniform(3.0, 5.0, size=(65, 1))      # a reference far away: every instance pulls hard
    assert (np.abs(u0) > 1e-3).all()
    return sp, x0, u0, yref, RR.solve_batch(sp, x0, u0, yref), RR.solve_batch(RR.without_rate(sp), x0, u0, yref)


@pytest.mark.parametrize("B", [1, 64, 65])
def test_smallest_shape_obeys_the_rate_and_matches_the_oracle(smallest, B):
    sp, x0, u0, yref, ref, ref_plain = smallest
    rate = 0.1
    idx = np.arange(B)
    r = _solve(_controller(sp), x0[:B], u0[:B], yref=yref[:B])
    _check(r, ref, sp, "B=%d" % B, idx)
    move = np.abs(r.cmd.cpu().numpy() - u0[:B]).max(axis=1)
    print("B=%d: largest first move %.17g (rate %.3g)" % (B, move.max(), rate))
    assert (move <= rate * (1 + 1e-5)).all(), move.max()
    assert (ref["n_rate_active"][:B] == 2).all()
    # the same controller without the setter moves more than three times as far, as the reference's plain QP does
    assert (np.abs(ref_plain["cmd"] - u0).max(axis=1) > 3 * rate).all()
    plain = _solve(_controller(sp, rate=False), x0[:B], u0[:B], yref=yref[:B])
    move0 = np.abs(plain.cmd.cpu().numpy() - u0[:B]).max(axis=1)
    assert (move0 > 3 * rate).all(), move0.min()
    _check(plain, ref_plain, RR.without_rate(sp), "plain B=%d" % B, idx)


# ---------------------------------------------------------------------------------------------
# 2, 3, 6. move blocking, ch = ph - 1, ch = ph and the full-feature controller, on every path
# ---------------------------------------------------------------------------------------------
def _case(name):
    if name == "full":
        sp = RR.full_feature_spec()
        x0, u0, yref, dmeas = RR.full_feature_batch(24)
        return sp, x0, u0, yref, dmeas
    dims = {"blocked": (3, 2, 0, 2, 8, 3), "ch=ph-1": (4, 2, 0, 2, 10, 9), "ch=ph": (4, 2, 0, 2, 10, 10)}[name]
    sp = RR.rate_spec(200, *dims, rate=0.1, vary=True)
    x0, u0, _ = RR.random_batch(sp, 24, 9)
    return sp, x0, u0, None, None


_CASES = {}


def _case_ref(name):
    """(case, oracle results), computed once per module run"""
    if name not in _CASES:
        sp, x0, u0, yref, dmeas = _case(name)
        _CASES[name] = ((sp, x0, u0, yref, dmeas), RR.solve_batch(sp, x0, u0, yref, dmeas))
    return _CASES[name]


@pytest.mark.parametrize("name", ["blocked", "ch=ph-1", "ch=ph", "full"])
def test_every_path_matches_the_oracle(name):
    (sp, x0, u0, yref, dmeas), ref = _case_ref(name)
    assert ref["n_rate_active"].max() >= 4
    if name == "full":
        # the four kinds of row meet in one working set, with a disturbance model
        d = RR.LN.LmpcDims(*sp["dims"])
        act = ((ref["active_lower"] != 0) | (ref["active_upper"] != 0))[:, d.neq:]
        kinds = np.stack([act[:, :d.off_y].any(axis=1), act[:, d.off_y:d.off_du].any(axis=1), act[:, d.off_du:d.off_s].any(axis=1), act[:, d.off_s:].any(axis=1)])
        assert kinds.all(axis=0).sum() >= 4
    ran = []
    for pname, generic, fused in PATHS:
        c = _controller(sp, generic, fused)
        flags = c.debug_get("flags")
        if (pname == "fused" and int(flags[2]) != 1) or (pname == "group" and int(flags[1]) != 1):
            continue                                   # this controller cannot take that path
        _check(_solve(c, x0, u0, **_gpu_refs(yref, dmeas)), ref, sp, "%s %s" % (name, pname))
        ran.append(pname)
    print("%s: paths %s; active rate rows per instance up to %d, working sets up to %d" % (name, ran, ref["n_rate_active"].max(), ref["n_active"].max()))
    assert {"default", "two-kernel", "generic"} <= set(ran)


# ---------------------------------------------------------------------------------------------
# 4. more than 128 general rows: the two-chunk kernel variant (oracle results recorded)
# ---------------------------------------------------------------------------------------------
def test_160_rate_rows_take_the_two_chunk_variant():
    sp, x0, u0, yref = RR.large_case()
    g = np.load(os.path.join(ROOT, "tests", "golden", "rate_bounds_oracle.npz"))
    assert np.array_equal(g["x0"], x0) and np.array_equal(g["u0"], u0) and np.array_equal(g["yref"], yref)
    ref = {k: g[k] for k in g.files}
    m = int(ref["ncon"])
    ref["active_lower"] = np.unpackbits(g["active_lower"], axis=1, bitorder="little")[:, :m]
    ref["active_upper"] = np.unpackbits(g["active_upper"], axis=1, bitorder="little")[:, :m]
    for pname, generic, fused in PATHS[:3]:
        c = _controller(sp, generic, fused)
        assert c.info()["kernel_variant"] == 2 and int(c.debug_get("dims")[1]) == 160
        r = _solve(c, x0, u0, yref=yref)
        ac = _check(r, ref, sp, "large " + pname)
        assert np.abs(r.cmd.cpu().numpy() - u0).max() <= 0.1 * (1 + 1e-5)
    assert ac.max() > 28 and ref["n_rate_active"].max() > 28


# ---------------------------------------------------------------------------------------------
# 5. 24 active rate rows: past the lean kernels' 16, the fallback lands on the oracle
# ---------------------------------------------------------------------------------------------
def test_a_working_set_of_24_rate_rows():
    sp = RR.integrator_spec(ph=24, rate=0.05, yref=3.0, box=None)
    r0 = np.random.default_rng(5)
    x0 = 0.05 * r0.normal(size=(8, 2)); u0 = 0.02 * r0.normal(size=(8, 1))
    ref = RR.solve_batch(sp, x0, u0)
    assert (ref["n_rate_active"] == 24).all() and (ref["polished"] == 1).all()
    for pname, generic, fused in PATHS:
        c = _controller(sp, generic, fused)
        flags = c.debug_get("flags")
        if (pname == "fused" and int(flags[2]) != 1) or (pname == "group" and int(flags[1]) != 1):
            continue
        r = _solve(c, x0, u0)
        ac = _check(r, ref, sp, "24 rows " + pname)
        assert (ac == 24).all(), (pname, ac)
        assert np.abs(r.cmd.cpu().numpy() - u0).max() <= 0.05 * (1 + 1e-5)


# ---------------------------------------------------------------------------------------------
# 7. warm against cold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocked", "ch=ph-1", "ch=ph", "full"])
def test_warm_start_with_shift_equals_cold(name):
    import torch
    (sp, x0, u0, yref, dmeas), ref = _case_ref(name)
    kw = _gpu_refs(yref, dmeas)
    c = _controller(sp, warm=True)
    first = _solve(c, x0, u0, **kw)
    _check(first, ref, sp, name + " tick 0")
    cmd = ref["cmd"]                          # the next tick from the oracle's command (the GPU's is equal to 1e-5): the same problem on every run
    d0 = (sp["dmeas"][:, 0][None, :] if dmeas is None else dmeas[:, :, 0]) if "Bd" in sp else np.zeros((len(x0), 0))
    x1 = x0 @ sp["A"].T + cmd @ sp["B"].T + (d0 @ sp["Bd"].T if "Bd" in sp else 0.0)
    cold = _solve(_controller(sp), x1, cmd, **kw)
    for shift in (True, False):
        warm = _solve(c, x1, cmd, warm=first, warm_shift=shift, **kw)
        a, b = warm.cmd.cpu().numpy(), cold.cmd.cpu().numpy()
        scale = np.maximum(np.abs(b).max(axis=1), 1e-12)
        assert (np.abs(a - b).max(axis=1) / scale).max() <= 1e-5, (name, shift)
        ca, cb = warm.cost.cpu().numpy(), cold.cost.cpu().numpy()
        assert (np.abs(ca - cb) / np.maximum(1.0, np.abs(cb))).max() <= 1e-7, (name, shift)
        assert torch.equal(warm.status, cold.status) and torch.equal(warm.solver_status, cold.solver_status)
        assert torch.equal(warm.active_lower, cold.active_lower) and torch.equal(warm.active_upper, cold.active_upper), (name, shift)
    # ... and the second tick is the oracle's as well
    _check(cold, RR.solve_batch(sp, x1, cmd, yref, dmeas), sp, name + " tick 1")


# ---------------------------------------------------------------------------------------------
# 8. infeasible by the rate
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_from", [0, 1], ids=["box on lastU too", "box from step 1"])
def test_infeasible_by_rate(box_from):
    """lastU = umax + 10 rate: the first move cannot come back inside the input box.  box_from = 0 is the case as the reference's own
    setter leaves it (the box's first column also bounds lastU itself); with box_from = 1 lastU is free and the rate row alone makes
    the instance infeasible.  The oracle reports primal infeasibility; the strict mode reports what the oracle does, the default mode
    what the reference's front end does with such a problem (MAX_ITERATION, a finite command; include/mpcx.h).  The neighbours in the
    batch are the oracle's."""
    rate, box = 0.1, 0.6
    sp = RR.rate_spec(500, 3, 2, 0, 2, 6, 6, rate=rate, box=box)
    sp["box_first"] = box_from
    x0, u0, _ = RR.random_batch(sp, 8, 3)
    bad = [2, 5]
    u0[bad, 0] = box + 10 * rate
    ref = RR.solve_batch(sp, x0, u0)
    good = np.setdiff1d(np.arange(8), bad)
    assert (ref["status"][bad] == 2).all() and (ref["is_feasible"][bad] == 0).all() and (ref["status"][good] == 0).all()
    assert (ref["solver_status"][bad] == RR.OSQP.OSQP_PRIMAL_INFEASIBLE).all() and (ref["polished"][good] == 1).all()
    c = _controller(sp)
    c.setStrictInfeasibility(True)
    r = _solve(c, x0, u0)
    assert np.array_equal(r.status.cpu().numpy(), ref["status"]) and np.array_equal(r.is_feasible.cpu().numpy(), ref["is_feasible"])
    assert np.isnan(r.cmd.cpu().numpy()[bad]).all()
    loose = _solve(_controller(sp), x0, u0)
    assert (loose.status.cpu().numpy()[bad] == 1).all() and (loose.is_feasible.cpu().numpy() == 1).all() and np.isfinite(loose.cmd.cpu().numpy()).all()
    for res in (r, loose):
        cmd = res.cmd.cpu().numpy()[good]
        err = np.abs(cmd - ref["cmd"][good]).max(axis=1) / np.maximum(np.abs(ref["cmd"][good]).max(axis=1), 1e-12)
        assert err.max() <= 1e-5, err.max()
        cost = res.cost.cpu().numpy()[good]
        assert (np.abs(cost - ref["cost"][good]) / np.maximum(1.0, np.abs(ref["cost"][good]))).max() <= 1e-7
        assert (res.status.cpu().numpy()[good] == 0).all()


# ---------------------------------------------------------------------------------------------
# 9. a bank of controllers with different rate bounds
# ---------------------------------------------------------------------------------------------
def test_hetero_bank_with_per_controller_rate_bounds():
    import torch
    from libmpc_amd import LMPC, LMPCHetero
    dims = (3, 2, 0, 2, 8, 8)
    specs = []
    for k in range(3):
        sp = RR.rate_spec(600 + k, *dims, rate=0.08 + 0.04 * k, vary=True, box=0.8)
        specs.append(sp)
    ctrls = [RR.configure(LMPC(*dims, device=-1), sp) for sp in specs]
    host = LMPCHetero(ctrls, device=0, condense_on_host=True)
    dev = LMPCHetero(ctrls, device=0)
    assert host.debug_get(0, "flags")[1] == 0.0 and dev.debug_get(0, "flags")[1] == 1.0
    for k in range(3):
        assert (ctrls[k].debug_get("g_kind") == 3).sum() > 0
        for name, tol in (("H", 1e-12), ("Gr", 1e-12), ("Gc", 1e-12), ("Y", 1e-9), ("rho_b", 1e-9), ("rho_g", 1e-9), ("Kinv", 1e-8)):
            a, b = host.debug_get(k, name), dev.debug_get(k, name)
            scale = max(np.abs(a).max(), 1e-300)
            assert np.abs(a - b).max() <= tol * scale, (k, name, np.abs(a - b).max() / scale)
        # the rate rows hold nothing but +-1: the device writes them exactly
        mg, ldz = int(ctrls[k].debug_get("dims")[1]), int(ctrls[k].debug_get("dims")[2])
        rows = ctrls[k].debug_get("g_kind").astype(int)[:mg] == 3
        assert np.array_equal(dev.debug_get(k, "Gr").reshape(-1, ldz)[:mg][rows], ctrls[k].debug_get("Gr").reshape(-1, ldz)[:mg][rows])
    B = 22
    x0, u0, _ = RR.random_batch(specs[0], B, 17)
    model = np.arange(B) % 3
    ra = host.optimizeBatch(x0, u0, model=model, want_active=True); rb = dev.optimizeBatch(x0, u0, model=model, want_active=True)
    torch.cuda.synchronize()
    assert torch.equal(ra.status, rb.status) and torch.equal(ra.active_lower, rb.active_lower) and torch.equal(ra.active_upper, rb.active_upper)
    np.testing.assert_allclose(ra.cmd.cpu().numpy(), rb.cmd.cpu().numpy(), rtol=1e-8, atol=1e-10)
    parts = [(np.nonzero(model == k)[0], RR.solve_batch(specs[k], x0[model == k], u0[model == k])) for k in range(3)]
    ref = {"neq": parts[0][1]["neq"], "ncon": parts[0][1]["ncon"]}
    for key, first in parts[0][1].items():
        if isinstance(first, np.ndarray):
            ref[key] = np.zeros((B,) + first.shape[1:], dtype=first.dtype)
            for idx, p in parts:
                ref[key][idx] = p[key]
    assert ref["n_rate_active"].min() >= 1
    _check(rb, ref, specs[0], "bank")
    _check(ra, ref, specs[0], "bank condensed on the host")
    # a controller with another pattern of finite rate bounds does not fit the bank, as with the other bounds
    from libmpc_amd import MpcxError
    odd = dict(specs[1], dumin=specs[1]["dumin"].copy(), dumax=specs[1]["dumax"].copy())
    odd["dumin"][0, :] = -np.inf; odd["dumax"][0, :] = np.inf
    with pytest.raises(MpcxError):
        LMPCHetero([ctrls[0], RR.configure(LMPC(*dims, device=-1), odd)], device=0)


# ---------------------------------------------------------------------------------------------
# 10. closed loops
# ---------------------------------------------------------------------------------------------
def _loop_inputs(B=8):
    r = np.random.default_rng(23)
    return 0.1 * r.normal(size=(B, 2)), np.zeros((B, 1))


def _rate_violation(u, u0, rate):
    """largest |cmd_k - cmd_{k-1}| - rate over the run, cmd_{-1} = lastU"""
    seq = np.concatenate([u0[None], u], axis=0)
    return float((np.abs(np.diff(seq, axis=0)) - rate).max())


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
def test_closed_loop_obeys_the_rate_and_equals_the_single_steps(warm):
    rate, ticks = 0.1, 40
    sp = RR.integrator_spec(ph=10, rate=rate, box=1.0, yref=1.0)
    x0, u0 = _loop_inputs()
    res = _controller(sp, warm=warm).simulate(x0, u0, ticks, warm=warm)
    u = res.u.cpu().numpy()
    worst = _rate_violation(u, u0, rate)
    print("closed loop %s: worst |cmd_k - cmd_(k-1)| - rate = %.3e over %d ticks x %d instances; largest |cmd| %.6f" % ("warm" if warm else "cold", worst, ticks, len(x0), np.abs(u).max()))
    assert worst <= rate * 1e-5, worst
    assert (res.status.cpu().numpy() == 0).all() and np.abs(u).max() <= 1.0 + 1e-9
    assert (np.abs(np.diff(np.concatenate([u0[None], u]), axis=0)) >= rate * (1 - 1e-5)).any()       # the bound was reached
    _follow(_controller(sp, warm=warm), res, res.x, u0, ticks, warm, "loop")
    # the same loop without the rate bounds moves more than 3 rate in one tick (as the oracle's does: test_lmpc_rate_bounds.py)
    plain = _controller(sp, warm=warm, rate=False).simulate(x0, u0, ticks, warm=warm)
    assert _rate_violation(plain.u.cpu().numpy(), u0, rate) + rate > 3 * rate


def test_observed_loop_obeys_the_rate_and_equals_the_single_steps_on_the_estimate():
    rate, ticks = 0.1, 40
    sp = RR.integrator_spec(ph=10, rate=rate, box=1.0, yref=1.0)
    x0, u0 = _loop_inputs()
    c = _controller(sp, warm=True)
    L = c.kalman_gain(0.01 * np.eye(2), 0.04 * np.eye(1))
    r = np.random.default_rng(29)
    res = c.simulate(x0, u0, ticks, warm=True, observer=L, xhat0=x0 + 0.05 * r.normal(size=x0.shape), meas_noise=0.01 * r.normal(size=(ticks, len(x0), 1)))
    worst = _rate_violation(res.u.cpu().numpy(), u0, rate)
    print("observed loop: worst |cmd_k - cmd_(k-1)| - rate = %.3e" % worst)
    assert worst <= rate * 1e-5, worst
    _follow(_controller(sp, warm=True), res, res.xhat, u0, ticks, True, "observed loop")


# ---------------------------------------------------------------------------------------------
# 11. the C++ front end
# ---------------------------------------------------------------------------------------------
def test_cpp_first_move_equals_the_python_front_ends():
    from test_lmpc_rate_bounds import build_cpp
    exe = build_cpp()
    env = {k: v for k, v in os.environ.items() if k != "MPCX_DEVICE"}
    out = subprocess.run([exe, "solve"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ rate-bound checks passed" in out.stdout
    got = {ln.split()[1]: float.fromhex(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("cmd ")}
    assert set(got) == {"static", "dynamic"}
    sp = RR.integrator_spec(ph=10, rate=0.1, box=1.0, yref=1.0)
    sp["dumin"][0, 9] = -np.inf                        # the program's last call: the last step bounded above only
    res = _controller(sp).optimize(np.zeros(2), np.array([0.3]))
    assert res.status == 0 and got["static"] == got["dynamic"] == float(res.cmd[0]), (got, float(res.cmd[0]).hex())
