"""-m gpu: the NLMPC closed loop with output feedback (mpcx_nlmpc_loop_create_observed, mpcx_nlmpc_ekf_step_batch; NLMPC.ekf_step and
make_loop / simulate with ekf=).

Shapes (those of test_nlmpc_loop_gpu.py, trimmed; the batches span at least two blocks of the filter's kernel with the last one partial):
  vdp   Van der Pol, ph 10 / ch 5, B 23 (10 instances per block), 5 ticks, Cm = [0 1]
  ugv   UGV, ph 12 / ch 4, B 13 (6 per block), 5 ticks, the two positions are measured
  osc6  six oscillators, ph 10 / ch 5, B 5 (2 per block), 3 ticks, the q_i are measured
  osc8  eight oscillators, ph 10 / ch 5, B 3 (one instance per wavefront), 2 ticks, the q_i are measured
The filter step is held to nlmpc_ekf_ref.py within its tolerances; an observed loop is held to the calls it replaces BIT FOR BIT."""
import ctypes as C

import numpy as np
import pytest

import nlmpc_ekf_ref as E
import nlmpc_plant_ref as P

pytestmark = pytest.mark.gpu

SHAPES = {"vdp": dict(model="vanderpol", ph=10, ch=5, Ts=0.1, B=23, ticks=5, max_iter=200, hard=1),
          "ugv": dict(model="ugv", ph=12, ch=4, Ts=0.1, B=13, ticks=5, max_iter=150, hard=0),
          "osc6": dict(model="osc6", ph=10, ch=5, Ts=0.1, B=5, ticks=3, max_iter=None, hard=1),
          "osc8": dict(model="osc8", ph=10, ch=5, Ts=0.1, B=3, ticks=2, max_iter=None, hard=1)}
CASE_OF = {"vanderpol": "vdp", "ugv": "ugv", "osc6": "osc6", "osc8": "osc8"}
LOGS = ("cost", "status", "solver_status", "is_feasible", "iterations")
FIELDS = ("x", "u") + LOGS + ("xhat", "y", "P", "ekf_flags")


def _controller(case):
    from libmpc_amd.nlmpc import NLMPC, NLParameters, VANDERPOL, UGV, OSCILLATORS6, OSCILLATORS8
    s = SHAPES[case]
    c = NLMPC(dict(vanderpol=VANDERPOL, ugv=UGV, osc6=OSCILLATORS6, osc8=OSCILLATORS8)[s["model"]], s["ph"], s["ch"], s["Ts"])
    kw = dict(hard_constraints=s["hard"])
    if s["max_iter"] is not None:
        kw["maximum_iteration"] = s["max_iter"]
    c.setOptimizerParameters(NLParameters(**kw))
    return c


def _start(case, seed=0):
    """x0 [B, nx], u0 [B, nu] (numpy), seeded: the starts of test_nlmpc_loop_gpu.py"""
    s = SHAPES[case]
    rng = np.random.default_rng(100 + seed)
    B = s["B"]
    if case == "vdp":
        x0 = rng.uniform(-1.0, 1.0, size=(B, 2)); x0[0] = [0.0, 1.0]
        return x0, np.zeros((B, 1))
    if case == "ugv":
        x0 = np.zeros((B, 4)); x0[:, :2] = rng.uniform(-0.5, 0.5, size=(B, 2))
        return x0, np.zeros((B, 2))
    n = E.DIMS[s["model"]][0]
    x0 = rng.uniform(-0.1, 0.1, size=(B, n)); x0[:, 0] += 1.0
    return x0, np.zeros((B, n // 2))


def _ugv_params(seed, spread=0.05):
    rng = np.random.default_rng(200 + seed)
    base = np.tile(np.array(P.DEFAULT_PARAMS["ugv"]), (SHAPES["ugv"]["B"], 1))
    p = base * (1.0 + rng.uniform(-spread, spread, size=base.shape))
    p[:, 8] = base[:, 8]
    return p


def _ekf(case, q=1e-4, r=1e-2, p0=1e-2, full=False):
    from libmpc_amd.nlmpc import NLEkf
    model = SHAPES[case]["model"]
    nx = E.DIMS[model][0]
    Cm = None if full else E.meas_matrix(model)
    ny = nx if full else Cm.shape[0]
    return NLEkf(Q=q * np.eye(nx), R=r * np.eye(ny), P0=p0 * np.eye(nx), C=Cm)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _snapshot(res):
    return {k: getattr(res, k).clone() for k in FIELDS}


_RUNS = {}


def _loop_run(case, warm, variant=""):
    """one observed closed-loop run per (case, warm, variant), shared by the tests that look at it: (controller, inputs, filter, result)"""
    import torch
    key = (case, warm, variant)
    if key not in _RUNS:
        s = SHAPES[case]
        c = _controller(case)
        x0, u0 = _start(case)
        ekf = _ekf(case)
        kw = {}
        if variant == "plant":
            kw["params"] = _ugv_params(1); kw["plant_params"] = _ugv_params(2, 0.1)
            kw["plant_params"][:, 8] = np.random.default_rng(7).choice([0.08, 0.1, 0.12], size=x0.shape[0])
        elif variant == "noise":
            rng = np.random.default_rng(9)
            ny = ekf.R.shape[0]
            kw["noise"] = rng.normal(scale=1e-2, size=(s["ticks"],) + x0.shape)
            kw["meas_noise"] = rng.normal(scale=3e-2, size=(s["ticks"], s["B"], ny))
            kw["xhat0"] = x0 + rng.normal(scale=3e-2, size=x0.shape)
        res = c.simulate(_t(x0), _t(u0), s["ticks"], warm=warm, ekf=ekf, log_P=True, **{k: _t(v) for k, v in kw.items()})
        torch.cuda.synchronize()
        _RUNS[key] = (c, dict(x0=x0, u0=u0, **kw), ekf, res)
    return _RUNS[key]


# ---- 4. the filter step against numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,substeps,variant", E.cases())
def test_ekf_step_against_numpy(model, substeps, variant):
    """every tick of the reference's own run of the case (nlmpc_ekf_ref.inputs: the inputs its tolerances were measured on): substeps 1 and 4 on Van
    der Pol, per-instance params in the `plant` variants, ny < nx everywhere but in `full`, where Cm is None"""
    import torch
    from libmpc_amd.nlmpc import NLEkf
    case = CASE_OF[model]
    c = _controller(case)
    d = E.inputs(model, variant)
    pc = d["ctrl"] if d["params"] is None else d["params"]
    _, xh, Pk, ys, _ = E.run(model, substeps, d, SHAPES[case]["Ts"])
    ekf = NLEkf(Q=d["Q"], R=d["R"], P0=d["P0"], C=d["Cm"])
    prm = _t(d["params"]) if c.n_params else None                  # (Van der Pol has no parameters to give per instance)
    tol_x, tol_P = E.TOL[model]
    worst = [0.0, 0.0]
    for k in range(E.TICKS):
        got = c.ekf_step(_t(xh[k]), _t(Pk[k]), _t(d["cmd"][k]), _t(ys[k]), ekf, params=prm, substeps=substeps)
        torch.cuda.synchronize()
        want = E.ekf_step(model, xh[k], Pk[k], d["cmd"][k], ys[k], pc, SHAPES[case]["Ts"], substeps, d["Cm"], d["Q"], d["R"])
        gx, gP = got[0].cpu().numpy(), got[1].cpu().numpy()
        ex, eP = E.rel_x(gx, want[0]), E.rel_P(gP, want[1])
        worst = [max(worst[0], ex / tol_x), max(worst[1], eP / tol_P)]
        print("ekf step %s substeps %d %s tick %d: xhat %.3e (tolerance %.2e), P %.3e (tolerance %.2e)" % (model, substeps, variant, k, ex, tol_x, eP, tol_P))
        assert ex <= tol_x and eP <= tol_P, (k, ex, tol_x, eP, tol_P)
        assert np.array_equal(gP, np.swapaxes(gP, 1, 2))                    # symmetric, bit for bit
        assert not got[2].cpu().numpy().any() and not want[2].any()
    # in place: the same bits
    xt, Pt = _t(xh[0]), _t(Pk[0])
    a = c.ekf_step(_t(xh[0]), _t(Pk[0]), _t(d["cmd"][0]), _t(ys[0]), ekf, params=prm, substeps=substeps)
    b = c.ekf_step(xt, Pt, _t(d["cmd"][0]), _t(ys[0]), ekf, params=prm, substeps=substeps, out=(xt, Pt))
    torch.cuda.synchronize()
    assert b[0].data_ptr() == xt.data_ptr() and _same(a[0], xt) and _same(a[1], Pt)


# ---- 5. certainty equivalence, exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["vdp", "ugv", "osc6", "osc8"])
def test_without_noise_and_mismatch_the_estimate_is_the_truth(case):
    """no process noise, no measurement noise, the plant's parameters the controller's, no xhat0: every lane's Phi is one call site, so the
    prediction and the truth are the same bits, the innovation is exactly 0 and the estimate never leaves the truth; the loop then IS the
    unobserved loop"""
    import torch
    c, inp, ekf, res = _loop_run(case, False)
    s = SHAPES[case]
    assert _same(res.xhat, res.x)
    assert not res.ekf_flags.cpu().numpy().any()
    plain = _controller(case).simulate(_t(inp["x0"]), _t(inp["u0"]), s["ticks"], warm=False)
    torch.cuda.synchronize()
    assert plain.xhat is None and plain.y is None and plain.P is None and plain.ekf_flags is None
    for name in ("x", "u") + LOGS:
        assert _same(getattr(res, name), getattr(plain, name)), (case, name)
    ok = (res.status != 3).float().mean().item()
    assert ok > 0.9, ok


# ---- 6. an observed loop is the calls it replaces, tick by tick ----------------------------------------------------------------------------
def _check_y(inp, ekf, res, k, nx):
    Cm = np.eye(nx) if ekf.C is None else ekf.C
    xn = res.x[k + 1].cpu().numpy()
    v = inp["meas_noise"][k] if "meas_noise" in inp else None
    want = xn @ Cm.T + (0.0 if v is None else v)
    bound = (nx + 1) * P.U * (np.abs(xn) @ np.abs(Cm).T + (0.0 if v is None else np.abs(v)))
    assert (np.abs(res.y[k].cpu().numpy() - want) <= bound).all(), k


@pytest.mark.parametrize("case,variant", [("vdp", ""), ("ugv", ""), ("osc6", ""), ("ugv", "plant"), ("vdp", "noise")])
def test_cold_observed_loop_equals_the_single_step_calls(case, variant):
    import torch
    c, inp, ekf, res = _loop_run(case, False, variant)
    s = SHAPES[case]
    assert _same(res.x[0], _t(inp["x0"])) and _same(res.xhat[0], _t(inp.get("xhat0", inp["x0"])))
    assert _same(res.P[0], _t(np.tile(ekf.P0, (s["B"], 1, 1))))
    pc = _t(inp.get("params"))
    pp = _t(inp.get("plant_params", inp.get("params")))
    for k in range(s["ticks"]):
        uk = _t(inp["u0"]) if k == 0 else res.u[k - 1]
        r = c.optimizeBatch(res.xhat[k], uk, params=pc)                        # the solve reads the estimate
        xn = c.plant_step(res.x[k], res.u[k], params=pp, noise=None if "noise" not in inp else _t(inp["noise"][k]))
        xh, Pn, fl = c.ekf_step(res.xhat[k], res.P[k], res.u[k], res.y[k], ekf, params=pc)
        torch.cuda.synchronize()
        assert _same(r["cmd"], res.u[k]), (case, variant, k)
        for name in LOGS:
            assert _same(r[name], getattr(res, name)[k]), (case, variant, k, name)
        assert _same(xn, res.x[k + 1]), (case, variant, k)
        assert _same(xh, res.xhat[k + 1]) and _same(Pn, res.P[k + 1]), (case, variant, k)
        assert not fl.cpu().numpy().any()
        _check_y(inp, ekf, res, k, c.nx)
    assert not res.ekf_flags.cpu().numpy().any()
    if variant:
        assert not _same(res.xhat, res.x)                                   # (the estimate is a thing of its own here)
    ok = (res.status != 3).float().mean().item()
    assert ok > 0.9, ok


def test_warm_observed_loop_equals_the_chained_calls():
    import torch
    case = "ugv"
    _, inp, ekf, res = _loop_run(case, True, "noise")
    s = SHAPES[case]
    c = _controller(case)                                          # a second handle of the same controller
    x, xh, u, z = _t(inp["x0"]), _t(inp["xhat0"]), _t(inp["u0"]), None
    Pk = _t(np.tile(ekf.P0, (s["B"], 1, 1)))
    for k in range(s["ticks"]):
        r = c.optimizeBatch(xh, u, z_warm=z, warm_curvature=True)
        xn = c.plant_step(x, r["cmd"], noise=_t(inp["noise"][k]))
        xhn, Pn, _ = c.ekf_step(xh, Pk, r["cmd"], res.y[k], ekf)
        torch.cuda.synchronize()
        assert _same(r["cmd"], res.u[k]), k
        for name in LOGS:
            assert _same(r[name], getattr(res, name)[k]), (k, name)
        assert _same(xn, res.x[k + 1]) and _same(xhn, res.xhat[k + 1]) and _same(Pn, res.P[k + 1]), k
        _check_y(inp, ekf, res, k, c.nx)
        x, xh, Pk, u, z = xn, xhn, Pn, r["cmd"], r["z"]


# ---- 7. the skipped update -----------------------------------------------------------------------------------------------------------------
def test_a_failed_cholesky_skips_the_update_and_sets_the_flag():
    import torch
    case = "vdp"
    s = SHAPES[case]
    c = _controller(case)
    x0, u0 = _start(case)
    rng = np.random.default_rng(3)
    xhat0 = x0 + rng.normal(scale=3e-2, size=x0.shape)
    v = rng.normal(scale=3e-2, size=(s["ticks"], s["B"], 1))
    res = c.simulate(_t(x0), _t(u0), s["ticks"], warm=False, ekf=_ekf(case, 0.0, 0.0, 0.0), xhat0=_t(xhat0), meas_noise=_t(v), log_P=True)
    torch.cuda.synchronize()
    assert (res.ekf_flags.cpu().numpy() == 1).all()
    assert (res.P.cpu().numpy() == 0).all()
    for name in ("x", "xhat", "y", "u", "cost"):
        assert torch.isfinite(getattr(res, name)).all(), name
    for k in range(s["ticks"]):
        assert _same(c.plant_step(res.xhat[k], res.u[k]), res.xhat[k + 1]), k          # the prediction and nothing else
    # the flags are cleared by every run: a loop with R > 0 on a flag tensor that stands at 1
    loop = c.make_loop(_t(x0), _t(u0), s["ticks"], warm=False, ekf=_ekf(case, 0.0, 1e-2, 0.0), xhat0=_t(xhat0), meas_noise=_t(v))
    try:
        loop.result.ekf_flags.fill_(1)
        c.run_loop(loop); torch.cuda.synchronize()
        assert not loop.result.ekf_flags.cpu().numpy().any()
        assert loop.result.P is None
    finally:
        c.destroy_loop(loop)


# ---- 8. housekeeping -----------------------------------------------------------------------------------------------------------------------
def test_runs_repeat_follow_refilled_inputs_and_stop_at_the_end():
    import torch
    from libmpc_amd import _capi
    lib = _capi.lib()
    case = "vdp"
    s = SHAPES[case]
    c, inp, ekf, shared = _loop_run(case, False, "noise")
    c = _controller(case)
    kw = {k: _t(inp[k]) for k in ("noise", "meas_noise", "xhat0")}
    loop = c.make_loop(_t(inp["x0"]), _t(inp["u0"]), s["ticks"], warm=False, ekf=ekf, log_P=True, **kw)
    try:
        c.run_loop(loop); torch.cuda.synchronize()
        first = _snapshot(loop.result)
        assert all(_same(first[k], getattr(shared, k)) for k in first)             # ... and so does another handle's loop
        c.run_loop(loop); torch.cuda.synchronize()
        second = _snapshot(loop.result)
        assert all(_same(first[k], second[k]) for k in first)
        # one more replay behind the end: the counter stands at `ticks`, nothing is written
        cur = torch.cuda.current_stream()
        assert lib.mpcx_nlmpc_loop_debug_replay(loop.handle, C.c_void_p(cur.cuda_stream)) == _capi.OK
        tick = C.c_int(-1)
        assert lib.mpcx_nlmpc_loop_debug_tick(loop.handle, C.byref(tick)) == _capi.OK and tick.value == s["ticks"]
        assert all(_same(second[k], getattr(loop.result, k)) for k in second)
        # another initial estimate and other measurement noise, refilled in place
        rng = np.random.default_rng(77)
        xh1 = inp["x0"] + rng.normal(scale=3e-2, size=inp["x0"].shape)
        v1 = rng.normal(scale=3e-2, size=inp["meas_noise"].shape)
        loop.keep[6].copy_(_t(xh1)); loop.keep[7].copy_(_t(v1))
        c.run_loop(loop); torch.cuda.synchronize()
        third = _snapshot(loop.result)
        assert _same(third["xhat"][0], _t(xh1)) and not _same(third["y"], first["y"]) and not _same(third["xhat"], first["xhat"])
        fresh = _controller(case).simulate(_t(inp["x0"]), _t(inp["u0"]), s["ticks"], warm=False, ekf=ekf, log_P=True, noise=kw["noise"],
                                           meas_noise=_t(v1), xhat0=_t(xh1))
        assert all(_same(third[k], getattr(fresh, k)) for k in third)
    finally:
        c.destroy_loop(loop)


def test_a_setter_on_the_controller_invalidates_an_observed_loop():
    import torch
    from libmpc_amd import MpcxError, _capi
    case = "vdp"
    s = SHAPES[case]
    c = _controller(case)
    x0, u0 = _start(case)
    loop = c.make_loop(_t(x0), _t(u0), s["ticks"], warm=True, ekf=_ekf(case))
    try:
        c.run_loop(loop); torch.cuda.synchronize()
        before = {k: getattr(loop.result, k).clone() for k in ("x", "u", "xhat", "y")}
        assert c.setInputBounds([-0.4], [0.4])
        with pytest.raises(MpcxError) as e:
            c.run_loop(loop)
        assert e.value.code == _capi.E_STATE and "new loop" in str(e.value)
        torch.cuda.synchronize()
        assert all(_same(before[k], getattr(loop.result, k)) for k in before)      # refused before anything ran
    finally:
        c.destroy_loop(loop)


def _raw_create(c, spoil):
    import torch
    from libmpc_amd import _capi
    B, T, nx, nu = 7, 2, c.nx, c.nu
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device="cuda")
    keep = [z(B, nx), z(B, nu), z(T + 1, B, nx), z(T, B, nu), z(T + 1, B, nx), z(T, B, nx)]
    d = _capi.NlmpcLoopDesc()
    d.batch, d.ticks, d.substeps, d.warm = B, T, 1, 1
    d.x0, d.u0, d.traj_x, d.traj_u = (t.data_ptr() for t in keep[:4])
    ny = spoil.get("ny", 1)
    mats = dict(Cm=np.asfortranarray(np.eye(nx)[:max(1, min(ny, nx))]), Q=np.asfortranarray(1e-4 * np.eye(nx)), R=np.asfortranarray(1e-2 * np.eye(max(ny, 1))),
                P0=np.asfortranarray(1e-2 * np.eye(nx)))
    for k in ("Cm", "Q", "R", "P0"):
        if k in spoil:
            mats[k] = spoil[k]
    e = _capi.NlmpcEkfDesc()
    e.ny = ny
    e.Cm, e.Q, e.R, e.P0 = (None if mats[k] is None else mats[k].ctypes.data for k in ("Cm", "Q", "R", "P0"))
    e.traj_xhat, e.traj_y = keep[4].data_ptr(), keep[5].data_ptr()
    st = torch.cuda.Stream()
    out = C.c_void_p()
    lib = _capi.lib()
    rc = lib.mpcx_nlmpc_loop_create_observed(c._h, C.byref(d), C.byref(e), C.c_void_p(st.cuda_stream), C.byref(out))
    msg = lib.mpcx_last_error().decode()
    torch.cuda.synchronize()
    if out.value:
        lib.mpcx_nlmpc_loop_destroy(out)
    return rc, msg, bool(out.value)


def _nan(n):
    a = np.asfortranarray(1e-2 * np.eye(n)); a[0, 0] = np.nan
    return a


BAD = {"ny above nx": dict(ny=3), "Cm null with ny below nx": dict(Cm=None), "Q not finite": dict(Q=_nan(2)), "R not finite": dict(R=np.array([[np.inf]])),
       "P0 not finite": dict(P0=_nan(2)), "Cm not finite": dict(Cm=np.array([[np.nan, 1.0]]))}


@pytest.mark.parametrize("name", sorted(BAD))
def test_an_invalid_filter_is_refused_with_a_message(name):
    from libmpc_amd import _capi
    c = _controller("vdp")
    rc, msg, made = _raw_create(c, BAD[name])
    assert rc == _capi.E_INVALID and msg and not made, (name, rc, msg)


def test_a_good_raw_descriptor_is_accepted_and_python_refuses_what_belongs_to_a_filter():
    from libmpc_amd import _capi
    c = _controller("vdp")
    assert _raw_create(c, {})[0] == _capi.OK                       # the descriptor the cases above spoil is a good one
    x0, u0 = _start("vdp")
    with pytest.raises(ValueError):
        c.make_loop(_t(x0), _t(u0), 2, meas_noise=_t(np.zeros((2, x0.shape[0], 1))))
    with pytest.raises(ValueError):
        c.make_loop(_t(x0), _t(u0), 2, log_P=True)


def test_hook_models_are_refused_as_unsupported():
    import torch
    from libmpc_amd import MpcxError, _capi
    from libmpc_amd.nlmpc import NLMPC
    usr = NLMPC.from_sources(2, 1, 2, 10, 5, 11, 0, 0.1,
                             state_fn="dx(0) = ((1.0 - (x(1) * x(1))) * x(0)) - x(1) + u(0); dx(1) = x(0);",
                             objective_fn="return x.array().square().sum() + u.array().square().sum();",
                             ineq_fn="for (int i = 0; i < ineq_c; i++) { in_con(i) = u(i, 0) - 0.5; }")
    rc, msg, made = _raw_create(usr, {})
    assert rc == _capi.E_UNSUPPORTED and "hook models come later" in msg and not made, (rc, msg)
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device="cuda")
    with pytest.raises(MpcxError) as e:
        usr.ekf_step(z(4, 2), z(4, 2, 2), z(4, 1), z(4, 1), _ekf("vdp"))
    assert e.value.code == _capi.E_UNSUPPORTED and "hook models come later" in str(e.value)
