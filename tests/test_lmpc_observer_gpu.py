"""Closed loops with output feedback (LMPC / LMPCHetero .simulate / make_loop with observer=, mpcx_lmpc_loop_create_observed): the solve of tick k
reads an estimate, the advance kernel measures y = C x + Dd d + v, steps the plant and the predictor-form observer.

Yardsticks, those of tests/test_lmpc_loop_gpu.py and tests/test_lmpc_loop_fleet_gpu.py, whose controllers and helpers are used as they are:
the unobserved loop (bit for bit where the summation-order contract makes the two agree), the single-step call on the logged estimate (bit for
bit), and float64 numpy on the logged inputs within operation-count bounds.  u = 2^-53 below; a chain of n fused multiply-adds from 0 has a
componentwise error of at most n u sum|c||v| (1 + O(u)), an add u times its result, and numpy's own product of the same terms no more.

Shapes: the three controllers of test_lmpc_loop_gpu.py (nx = 12, 4, 3 with ny = 12, 4, 2) plus `wide` (nx = 2, ny = 3: more output rows than
lanes of an instance, 32 instances per wavefront) and `five` (nx = 5, ny = 2: 12 instances, 4 idle lanes, ny divides neither); B = 1, 22 and
100 are a partial tile, a tile boundary and several tiles with a partial last one."""
import dataclasses
import functools

import numpy as np
import pytest

from helpers import configure_random, random_lmpc_spec
from test_lmpc_loop_gpu import CONTROLLERS, EQUAL, _assert_plant, _follow, _np
from test_lmpc_loop_fleet_gpu import _assert_plants, _bank_case, _copies, _scaled

pytestmark = pytest.mark.gpu

FIELDS = ("x", "u") + EQUAL
EPS = 2.0 ** -52


def _random_of(**kw):
    from libmpc_amd import LMPC
    sp = random_lmpc_spec(3, **kw)
    nx, nu = sp["dims"][0], sp["dims"][1]

    def inputs(B):
        r = np.random.default_rng(B)
        return r.uniform(-0.5, 0.5, size=(B, nx)), r.uniform(-0.4, 0.4, size=(B, nu)), {}
    return (lambda: configure_random(LMPC(*sp["dims"], device=0), sp)), inputs, (sp["A"], sp["B"], sp["Bd"], sp["dmeas"][:, 0])


ALL = dict(CONTROLLERS, wide=lambda: _random_of(nx=2, ny=3), five=lambda: _random_of(nx=5))


def _gain(c):
    return c.kalman_gain(0.01 * np.eye(c.nx), 0.04 * np.eye(c.ny))


def _mv(M, v):
    """M_b v_b for [B, r, c] matrices and [B, c] vectors"""
    return np.einsum("bij,bj->bi", M, v)


def _batchwise(M, B):
    M = np.asarray(M, dtype=np.float64)
    return _copies(M, B) if M.ndim == 2 else M


def _assert_measurement(res, Cm, Dd, d_of_tick, v, label):
    """y_k against float64 numpy C x + Dd d + v on the logged true state.  The kernel's chain of nx + ndu fused multiply-adds and one add:
    (nx + ndu + 1) u mag; numpy's products and two adds no more; together (nx + ndu + 1) 2^-52 mag, and 2 x 2^-52 mag for the terms of second
    order: (nx + ndu + 3) 2^-52 (|C||x| + |Dd||d| + |v|)"""
    x, y = _np(res.x), _np(res.y)
    B = x.shape[1]
    Cm, Dd = _batchwise(Cm, B), _batchwise(Dd, B)
    nx, ndu = Cm.shape[2], Dd.shape[2]
    for k in range(y.shape[0]):
        d = np.broadcast_to(d_of_tick(k), (B, ndu))
        vk = v[k] if v is not None else np.zeros_like(y[k])
        want = _mv(Cm, x[k]) + _mv(Dd, d) + vk
        bound = (nx + ndu + 3) * EPS * (_mv(np.abs(Cm), np.abs(x[k])) + _mv(np.abs(Dd), np.abs(d)) + np.abs(vk))
        err = np.abs(y[k] - want)
        print("%s tick %d: measurement error max %.3e, worst ratio to the bound %.3f" % (label, k, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, k, float(err.max()))


def _estimator_bound(A, Bm, Bd, Cm, Dd, L, xh, u, d, e):
    """componentwise bound on |xhat_{k+1} - numpy|, numpy being A xhat + B u + Bd d + L e with e = y - (C xhat + Dd d) from the logged y.
    The kernel's yhat is a chain of nx + ndu fused multiply-adds, numpy's two products and an add: they differ by at most
    dyh = (nx + ndu + 2) 2^-52 (|C||xhat| + |Dd||d|); each subtraction from y adds u |e|, so the two innovations differ by at most
    dyh + 2^-52 |e| (the bound below allows 2 dyh).  The kernel's row is a chain of nx + nu + ndu + ny fused multiply-adds, numpy's four
    products and three adds no more: (nx + nu + ndu + ny + 2) 2^-52 (|A||xhat| + |B||u| + |Bd||d| + |L||e|)"""
    nx, nu, ndu, ny = A.shape[2], Bm.shape[2], Bd.shape[2], Cm.shape[1]
    dyh = (nx + ndu + 2) * EPS * (_mv(np.abs(Cm), np.abs(xh)) + _mv(np.abs(Dd), np.abs(d)))
    mag = _mv(np.abs(A), np.abs(xh)) + _mv(np.abs(Bm), np.abs(u)) + _mv(np.abs(Bd), np.abs(d)) + _mv(np.abs(L), np.abs(e))
    return (nx + nu + ndu + ny + 2) * EPS * mag + _mv(np.abs(L), 2 * dyh + EPS * np.abs(e))


def _assert_estimator(res, A, Bm, Bd, Cm, Dd, L, d_of_tick, label):
    xh, u, y = _np(res.xhat), _np(res.u), _np(res.y)
    B = xh.shape[1]
    A, Bm, Bd, Cm, Dd, L = (_batchwise(M, B) for M in (A, Bm, Bd, Cm, Dd, L))
    for k in range(u.shape[0]):
        d = np.broadcast_to(d_of_tick(k), (B, Bd.shape[2]))
        e = y[k] - (_mv(Cm, xh[k]) + _mv(Dd, d))
        want = _mv(A, xh[k]) + _mv(Bm, u[k]) + _mv(Bd, d) + _mv(L, e)
        bound = _estimator_bound(A, Bm, Bd, Cm, Dd, L, xh[k], u[k], d, e)
        err = np.abs(xh[k + 1] - want)
        print("%s tick %d: estimator error max %.3e, worst ratio to the bound %.3f" % (label, k, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, k, float(err.max()))


# ---------------------------------------------------------------------------------------------
# 1. certainty equivalence, exact: the test of the summation-order contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 22, 100])
@pytest.mark.parametrize("name", sorted(ALL))
def test_an_observer_that_starts_at_the_state_reproduces_the_unobserved_loop_bit_for_bit(name, B):
    """No xhat0, no sensor noise: e_0 is an exact 0 and the estimator's row is the plant's chain of fused multiply-adds followed by ny terms
    L x 0, so on the controller's own plant -- the default, or plants= copies of it -- xhat stays x bitwise and every field equals the
    unobserved loop's.  With process noise w_k the plant adds w_k behind that chain and the estimator does not, so equality cannot go
    beyond tick 0 (the solve of tick 1 reads xhat_1 = x_1 - w_0); what is exact then: tick 0's solve, x_1, and xhat_1 = the x_1 of the run
    without noise."""
    import torch
    make, inputs, (A, Bm, Bd, _) = ALL[name]()
    ticks = 5
    x0, u0, refs = inputs(B)
    c = make()
    L = _gain(c)
    quiet = c.simulate(x0, u0, ticks, **refs)
    assert quiet.xhat is None and quiet.y is None
    assert int((quiet.status == 0).sum()) > 0
    plants = (_copies(A, B), _copies(Bm, B), _copies(Bd, B))
    for label, kw in (("own plant", {}), ("plants=", dict(plants=plants))):
        obs = c.simulate(x0, u0, ticks, observer=L, **kw, **refs)
        for f in FIELDS:
            a, b = getattr(obs, f), getattr(quiet, f)
            assert torch.equal(a, b), (name, B, label, f, int((a != b).sum()))
        assert torch.equal(obs.xhat, obs.x), (name, B, label, int((obs.xhat != obs.x).sum()))
        assert tuple(obs.y.shape) == (ticks, B, c.ny)
    noise = 0.05 * np.random.default_rng(5).normal(size=(ticks, B, c.nx))
    noisy = c.simulate(x0, u0, ticks, noise=noise, **refs)
    for label, kw in (("own plant", {}), ("plants=", dict(plants=plants))):
        obs = c.simulate(x0, u0, ticks, observer=L, noise=noise, **kw, **refs)
        assert torch.equal(obs.x[:2], noisy.x[:2]) and torch.equal(obs.u[0], noisy.u[0]), (name, B, label)
        for f in EQUAL:
            assert torch.equal(getattr(obs, f)[0], getattr(noisy, f)[0]), (name, B, label, f)
        assert torch.equal(obs.xhat[0], obs.x[0]) and torch.equal(obs.xhat[1], quiet.x[1]), (name, B, label)


# ---------------------------------------------------------------------------------------------
# 2. every tick against the single-step call on the logged estimate, bit for bit
# ---------------------------------------------------------------------------------------------
def _disturbed(c, B, ticks, seed):
    """xhat0 - x0, sensor noise, process noise"""
    r = np.random.default_rng(seed)
    return 0.05 * r.normal(size=(B, c.nx)), 0.02 * r.normal(size=(ticks, B, c.ny)), 0.02 * r.normal(size=(ticks, B, c.nx))


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", sorted(ALL))
def test_ticks_of_an_observed_loop_equal_the_single_step_call_on_the_estimate(name, warm):
    import torch
    make, inputs, _ = ALL[name]()
    B, ticks = (100 if name == "quadrotor" else 22), 7
    x0, u0, refs = inputs(B)
    c = make()
    dx, v, w = _disturbed(c, B, ticks, 31)
    res = c.simulate(x0, u0, ticks, warm=warm, observer=_gain(c), xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    assert np.array_equal(_np(res.x[0]), x0) and np.array_equal(_np(res.xhat[0]), x0 + dx)
    assert not torch.equal(res.xhat, res.x)
    _follow(make(), dataclasses.replace(res, x=res.xhat), u0, ticks, "%s observed %s" % (name, "warm" if warm else "cold"), warm=warm, **refs)


@functools.lru_cache(maxsize=None)
def _bank_outputs(name):
    """per controller of _bank(name): C, Dd and the Kalman gain, [K, ...]"""
    from libmpc_amd import LMPC
    from libmpc_amd.workloads import quadrotor_variant
    if name.startswith("random"):
        ctrls = [configure_random(LMPC(*sp["dims"], device=-1), sp) for sp in (random_lmpc_spec(100 + k) for k in range(22 if name == "random22" else 7))]
    else:
        ctrls = [quadrotor_variant(k, 10, device=-1) for k in range(8)]
    return tuple(np.stack(m) for m in zip(*[(np.array(c._C), np.array(c._Dd), _gain(c)) for c in ctrls]))


def _bank_observed_case(name):
    het, mats, B, x0, u0, refs = _bank_case(name)
    idx = refs["model"] if "model" in refs else np.arange(B)
    Cm, Dd, L = (m[idx] for m in _bank_outputs(name))
    return het, mats, (Cm, Dd, L), B, x0, u0, refs


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", ["random7_mixed", "quadrotor8"])
def test_ticks_of_an_observed_bank_loop_equal_the_banks_single_step_call_on_the_estimate(name, warm):
    het, _, (_, _, L), B, x0, u0, refs = _bank_observed_case(name)
    ticks = 7
    dx, v, w = _disturbed(het, B, ticks, 32)
    res = het.simulate(x0, u0, ticks, warm=warm, observer=L, xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    assert np.array_equal(_np(res.xhat[0]), x0 + dx)
    _follow(het, dataclasses.replace(res, x=res.xhat), u0, ticks, "%s observed %s" % (name, "warm" if warm else "cold"), warm=warm, **refs)
    with pytest.raises(ValueError):
        het.simulate(x0, u0, ticks, observer=L[0], **refs)


# ---------------------------------------------------------------------------------------------
# 3. the three linear steps against float64 numpy on the logged inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gains", ["one", "per_instance"])
@pytest.mark.parametrize("name", sorted(ALL))
def test_measurement_plant_and_estimator_steps_against_numpy(name, gains):
    make, inputs, (A, Bm, Bd, d0) = ALL[name]()
    B, ticks = 100, 5
    x0, u0, refs = inputs(B)
    c = make()
    dx, v, w = _disturbed(c, B, ticks, 33)
    L = _gain(c)
    if gains == "per_instance":
        L = _scaled(L, B, np.random.default_rng(34))
    plant = (1.02 * A, None, None)              # the plant is not the estimator's model
    res = c.simulate(x0, u0, ticks, plant=plant, observer=L, xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    label = "%s %s" % (name, gains)
    _assert_measurement(res, c._C, c._Dd, lambda k: d0, v, label)
    _assert_plant(res, plant[0], Bm, Bd, lambda k: d0, w, label)
    _assert_estimator(res, A, Bm, Bd, c._C, c._Dd, L, lambda k: d0, label)


def test_the_steps_of_an_observed_bank_with_a_plant_per_instance_against_numpy():
    het, (A, Bm, Bd, d0), (Cm, Dd, L), B, x0, u0, refs = _bank_observed_case("random7_mixed")
    ticks = 5
    rng = np.random.default_rng(35)
    dx, v, w = _disturbed(het, B, ticks, 36)
    P = tuple(_scaled(m[0], B, rng) for m in (A, Bm, Bd))           # variations of controller 0's model: no instance's estimator has its plant
    res = het.simulate(x0, u0, ticks, plants=P, observer=L, xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    _assert_measurement(res, Cm, Dd, lambda k: d0, v, "bank")
    _assert_plants(res, *P, lambda k: d0, w, "bank")
    _assert_estimator(res, A, Bm, Bd, Cm, Dd, L, lambda k: d0, "bank")
    # and each instance's own controller as its plant, the measurement without noise
    res = het.simulate(x0, u0, ticks, observer=L, xhat0=x0 + dx, **refs)
    _assert_measurement(res, Cm, Dd, lambda k: d0, None, "bank own plants")
    _assert_plants(res, A, Bm, Bd, lambda k: d0, None, "bank own plants")
    _assert_estimator(res, A, Bm, Bd, Cm, Dd, L, lambda k: d0, "bank own plants")


# ---------------------------------------------------------------------------------------------
# 4. the estimate converges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL))
def test_the_estimation_error_follows_the_observers_error_dynamics(name):
    """Perfect model, no noise, xhat0 = x0 + delta: both states get the same command, so x_k - xhat_k = F^k (-delta) with F = A - L C.
    With F = V diag(lam) V^-1: ||F^k delta|| <= cond(V) rho^k ||delta||.  Round-off: the logged difference obeys E_{k+1} = F E_k + r_k with
    |r_k| at most the plant step's bound, the estimator step's and |L| times the measurement's (section 3; the estimator's is against the
    logged y, whose own error enters through L), so its distance from numpy's F^k (-delta) is bounded by
    D_{k+1} = |F| D_k + r_k + (nx + 2) 2^-52 |F||F^k delta| (the last term: numpy's own product), plus 2^-52 |x - xhat| for the subtraction
    that forms the difference here."""
    make, inputs, (A, Bm, Bd, d0) = ALL[name]()
    B, ticks = 22, 7
    x0, u0, refs = inputs(B)
    c = make()
    L = _gain(c)
    Cm, Dd = np.array(c._C), np.array(c._Dd)
    delta = 0.1 * np.random.default_rng(41).normal(size=(B, c.nx))
    res = c.simulate(x0, u0, ticks, observer=L, xhat0=x0 + delta, **refs)
    x, xh, u, y = _np(res.x), _np(res.xhat), _np(res.u), _np(res.y)
    F = A - L @ Cm
    lam, V = np.linalg.eig(F)
    rho, condV = np.abs(lam).max(), np.linalg.cond(V)
    assert rho < 1.0
    nx, nu, ndu = c.nx, c.nu, c.ndu
    model = tuple(_copies(M, B) for M in (A, Bm, Bd, Cm, Dd, L))
    d = np.broadcast_to(d0, (B, ndu))
    want, D = x[0] - xh[0], np.zeros((B, nx))
    for k in range(ticks + 1):
        got = x[k] - xh[k]
        err = np.abs(got - want)
        norm, limit = np.linalg.norm(got, axis=1), condV * rho ** k * np.linalg.norm(delta, axis=1) + np.linalg.norm(D, axis=1)
        print("%s tick %d: ||x - xhat|| max %.3e (limit %.3e, rho %.3f, cond V %.1f), distance from F^k e_0 max %.3e, worst ratio to its bound %.3f"
              % (name, k, norm.max(), limit.max(), rho, condV, err.max(), (err / np.maximum(D, 1e-300)).max() if k else 0.0))
        assert (err <= D + EPS * np.abs(got)).all(), (name, k, float(err.max()))
        assert (norm <= limit).all(), (name, k, float(norm.max()))
        if k == ticks:
            break
        e = y[k] - (xh[k] @ Cm.T + d @ Dd.T)
        r_x = (nx + nu + ndu + 2) * EPS * (np.abs(x[k]) @ np.abs(A).T + np.abs(u[k]) @ np.abs(Bm).T + np.abs(d) @ np.abs(Bd).T)
        r_h = _estimator_bound(*model, xh[k], u[k], d, e)
        r_y = ((nx + ndu + 3) * EPS * (np.abs(x[k]) @ np.abs(Cm).T + np.abs(d) @ np.abs(Dd).T)) @ np.abs(L).T
        D = D @ np.abs(F).T + r_x + r_h + r_y + (nx + 2) * EPS * (np.abs(want) @ np.abs(F).T)
        want = want @ F.T


# ---------------------------------------------------------------------------------------------
# 5. re-run, replay past the end, refills in place, invalidation
# ---------------------------------------------------------------------------------------------
def test_observed_rerun_replay_past_the_end_refills_and_invalidation():
    import ctypes as C
    import torch
    from libmpc_amd import LMPC, MpcxError, _capi
    make, inputs, (A, Bm, Bd, d0) = CONTROLLERS["quadrotor"]()
    B, ticks = 100, 4
    x0, u0, refs = inputs(B)
    c = make()
    dx, v, w = _disturbed(c, B, ticks, 51)
    L = _copies(_gain(c), B)
    loop = c.make_loop(x0, u0, ticks, observer=L, xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    fields = FIELDS + ("xhat", "y")
    try:
        runs = []
        for _ in range(2):
            res = c.run_loop(loop)
            torch.cuda.synchronize()
            runs.append({k: getattr(res, k).clone() for k in fields})
        for k in fields:
            assert torch.equal(runs[0][k], runs[1][k]), k
        assert int((runs[0]["status"] == 0).sum()) > 0

        # one replay more than `ticks`: the counter stands at `ticks` and nothing is written, the estimates and measurements included
        lib = _capi.lib()
        tick = C.c_int(-1)
        _capi.check(lib.mpcx_lmpc_loop_debug_tick(loop.handle, C.byref(tick)))
        assert tick.value == ticks
        for k in fields:
            getattr(loop.result, k).add_(1.0 if getattr(loop.result, k).is_floating_point() else 1)
        torch.cuda.synchronize()
        _capi.check(lib.mpcx_lmpc_loop_debug_replay(loop.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        _capi.check(lib.mpcx_lmpc_loop_debug_tick(loop.handle, C.byref(tick)))
        assert tick.value == ticks
        for k in fields:
            assert torch.equal(getattr(loop.result, k), runs[0][k] + 1), k

        # xhat0 refilled in place: the next run starts its estimate there
        assert loop.xhat0 is not None and loop.meas_noise is not None and loop.gains is not None
        new = torch.as_tensor(x0 - dx).cuda()
        loop.xhat0.copy_(new)
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        assert torch.equal(res.xhat[0], new) and torch.equal(res.x[0], runs[0]["x"][0])
        assert not torch.equal(res.xhat[1], runs[0]["xhat"][1])
        # the sensor noise refilled: the measurements are C x + Dd d alone
        loop.meas_noise.zero_()
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        _assert_measurement(res, c._C, c._Dd, lambda k: d0, None, "refilled meas_noise")
        _assert_estimator(res, A, Bm, Bd, c._C, c._Dd, L, lambda k: d0, "refilled meas_noise")
        # the gains refilled: other gains estimate otherwise, and within the bound of their own step
        L2 = 0.5 * L
        before = res.xhat.clone()
        loop.gains.copy_(LMPC.pack_gains(torch.as_tensor(L2).cuda()))
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        assert not torch.equal(res.xhat, before)
        _assert_estimator(res, A, Bm, Bd, c._C, c._Dd, L2, lambda k: d0, "refilled gains")

        # a setter invalidates the loop
        c.setReferences(np.zeros(12), np.zeros(4), np.zeros(4), (0, c.ph))
        with pytest.raises(MpcxError) as e:
            c.run_loop(loop)
        assert e.value.code == _capi.E_STATE
    finally:
        c.destroy_loop(loop)
    c.destroy_loop(loop)          # idempotent
