"""Offset-free loops (LMPC / LMPCHetero .simulate / make_loop with disturbance_observer=, mpcx_lmpc_loop_create_offset_free): the estimator carries
[xhat; dhat], the solve of tick k reads xhat_k, u_{k-1} and dhat_k, and dmeas= is the true disturbance that acts on the plant and the measurement.

Yardsticks: the observed loop of tests/test_lmpc_observer_gpu.py (bit for bit with Ld = 0 and dhat_0 = delta: the summation-order contract), the
single-step call on the logged estimates (bit for bit), float64 numpy (tests/lmpc_offset_free_ref.py) within its operation-count bounds, a host loop
of the CPU oracle's solves and that numpy tick for the tracking error, and the 60-digit Riccati solutions of tests/golden for the gains.

Shapes (nx, nu, ndu, ny): (1,1,1,1) at B = 1, 64, 65 -- a full tile of 64 instances and one over; (3,2,1,2) at B = 22 -- 21 per wavefront; (2,2,3,3)
at B = 33 -- more rows of dhat than lanes of an instance, 32 per wavefront and one over; (5,2,2,2) at B = 13 -- 12 per wavefront, 4 idle lanes, two
tiles; the quadrotor 12/4/4/12 with Bd = B, Dd = 0 at B = 6 -- 5 per wavefront; (33,2,2,3) with ph = 3, ch = 2 at B = 3 -- one instance per
wavefront, 31 idle lanes; (32,2,2,3) at B = 5 -- two instances fill the 64 lanes exactly, two full tiles and a half; (64,2,2,3) at B = 3 -- every
lane a state row, the largest nx a controller accepts."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import lmpc_offset_free_ref as ref
from helpers import OracleFrontEnd, configure_random, random_lmpc_spec
from test_lmpc_loop_gpu import EQUAL, _follow, _np
from test_lmpc_loop_fleet_gpu import _bank_case, _scaled
from test_lmpc_observer_gpu import _bank_outputs

pytestmark = pytest.mark.gpu

FIELDS = ("x", "u") + EQUAL + ("xhat", "y")


# ---------------------------------------------------------------------------------------------
# controllers: name -> (make a controller, inputs(B) -> x0, u0, keyword references, model (A, B, Bd, C, Dd))
# ---------------------------------------------------------------------------------------------
def _random_of(**kw):
    from libmpc_amd import LMPC
    sp = random_lmpc_spec(3, **kw)
    nx, nu = sp["dims"][0], sp["dims"][1]

    def inputs(B):
        r = np.random.default_rng(B)
        return min(1.0, (3.0 / nx) ** 0.5) * r.uniform(-0.5, 0.5, size=(B, nx)), r.uniform(-0.4, 0.4, size=(B, nu)), {}      # (outputs of the size nx = 3 has)
    return (lambda device=0: configure_random(LMPC(*sp["dims"], device=device), sp)), inputs, tuple(sp[k] for k in ("A", "B", "Bd", "C", "Dd"))


def _quadrotor():
    from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc, quadrotor_matrices
    A, Bm, Cm = quadrotor_matrices()
    Dd = np.zeros((12, 4))

    def make(device=0):
        c = quadrotor_lmpc(10, device=device)
        assert c.setDisturbances(Bm, Dd)
        return c

    def inputs(B):
        x0, u0, yref = quadrotor_batch(B)
        return x0, u0, dict(yref=yref)
    return make, inputs, (A, Bm, Bm.copy(), Cm, Dd)


SHAPES = {
    "n1": lambda: _random_of(nx=1, nu=1, ndu=1, ny=1),
    "n3": lambda: _random_of(nx=3, nu=2, ndu=1, ny=2),
    "n2_d3": lambda: _random_of(nx=2, nu=2, ndu=3, ny=3),
    "n5": lambda: _random_of(nx=5, nu=2, ndu=2, ny=2),
    "quadrotor": _quadrotor,
    "n33": lambda: _random_of(nx=33, nu=2, ndu=2, ny=3, ph=3, ch=2),
    "n32": lambda: _random_of(nx=32, nu=2, ndu=2, ny=3, ph=3, ch=2),
    "n64": lambda: _random_of(nx=64, nu=2, ndu=2, ny=3, ph=3, ch=2),
}
CASES = [("n1", 1), ("n1", 64), ("n1", 65), ("n3", 22), ("n2_d3", 33), ("n5", 13), ("quadrotor", 6), ("n33", 3), ("n32", 5), ("n64", 3)]
SINGLE_STEP_B = {"quadrotor": 6, "n33": 6, "n32": 5, "n64": 3}      # (every other shape: 22)
CASE_IDS = ["%s-B%d" % c for c in CASES]


def _augmented(model):
    A, _, Bd, Cm, Dd = model
    nx, ndu = Bd.shape
    return np.block([[A, Bd], [np.zeros((ndu, nx)), np.eye(ndu)]]), np.hstack([Cm, Dd])


def _host_gain(model, qd=0.05):
    """[Lx; Ld] of the augmented pair by scipy on the host: the arithmetic tests need a gain, not the device's (n = 35 is past its limit)"""
    from scipy.linalg import solve_discrete_are
    Aa, Ca = _augmented(model)
    nx, ndu = model[2].shape
    ny = Ca.shape[0]
    Q = np.diag([0.01] * nx + [qd] * ndu)
    P = solve_discrete_are(Aa.T, Ca.T, Q, 0.04 * np.eye(ny))
    return Aa @ P @ Ca.T @ np.linalg.inv(Ca @ P @ Ca.T + 0.04 * np.eye(ny))


def _state_gain(model):
    """a state observer's gain for the equivalence test, where any gain serves"""
    from scipy.linalg import solve_discrete_are
    A, _, _, Cm, _ = model
    ny = Cm.shape[0]
    P = solve_discrete_are(A.T, Cm.T, 0.01 * np.eye(A.shape[0]), 0.04 * np.eye(ny))
    return A @ P @ Cm.T @ np.linalg.inv(Cm @ P @ Cm.T + 0.04 * np.eye(ny))


def _disturbed(nx, ndu, ny, B, ticks, seed):
    """xhat0 - x0, dhat0, delta (per instance), sensor noise, process noise"""
    r = np.random.default_rng(seed)
    return (0.05 * r.normal(size=(B, nx)), 0.1 * r.normal(size=(B, ndu)), 0.2 * r.normal(size=(B, ndu)), 0.02 * r.normal(size=(ticks, B, ny)),
            0.02 * r.normal(size=(ticks, B, nx)))


def _with_zero_rows(Lx, ndu):
    """[Lx; 0]: [.., nx + ndu, ny]"""
    return np.concatenate([Lx, np.zeros(Lx.shape[:-2] + (ndu, Lx.shape[-1]))], axis=-2)


# ---------------------------------------------------------------------------------------------
# 1. with Ld = 0 and dhat_0 = delta the loop is the observed loop given delta as its per-instance dmeas, bit for bit
# ---------------------------------------------------------------------------------------------
def _assert_equals_the_observed_loop(sim, nx, ndu, B, ticks, Lx, delta, label, **kw):
    import torch
    obs = sim(observer=Lx, dmeas=delta, **kw)
    off = sim(disturbance_observer=_with_zero_rows(np.asarray(Lx), ndu), dhat0=delta, dmeas=delta, **kw)
    print("%s: %d of %d solves end with status 0" % (label, int((obs.status == 0).sum()), obs.status.numel()))
    for f in FIELDS:
        a, b = getattr(off, f), getattr(obs, f)
        assert torch.equal(a, b), (label, f, int((a != b).sum()))
    assert obs.dhat is None and tuple(off.dhat.shape) == (ticks + 1, B, ndu)
    want = torch.as_tensor(delta).cuda().expand(ticks + 1, B, ndu)
    assert torch.equal(off.dhat.view(torch.int64), want.contiguous().view(torch.int64)), label


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_without_a_disturbance_gain_the_loop_is_the_observed_loop_bit_for_bit(case, warm):
    name, B = case
    make, inputs, model = SHAPES[name]()
    A, Bm, Bd, Cm, Dd = model
    nx, ndu, ny, ticks = A.shape[0], Bd.shape[1], Cm.shape[0], 5
    x0, u0, refs = inputs(B)
    dx, _, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 61)
    c = make()
    Lx = _state_gain(model)
    rng = np.random.default_rng(62)

    def sim(**kw):
        return c.simulate(x0, u0, ticks, warm=warm, xhat0=x0 + dx, meas_noise=v, noise=w, **kw, **refs)
    # one gain on the controller's own plant; a gain per instance on a plant per instance
    _assert_equals_the_observed_loop(sim, nx, ndu, B, ticks, Lx, delta, "%s B=%d one gain" % case)
    plants = tuple(_scaled(M, B, rng) for M in (A, Bm, Bd))
    _assert_equals_the_observed_loop(sim, nx, ndu, B, ticks, _scaled(Lx, B, rng), delta, "%s B=%d gains" % case, plants=plants)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_a_bank_without_disturbance_gains_is_its_observed_loop_bit_for_bit(warm):
    het, _, B, x0, u0, refs = _bank_case("random7_mixed")
    Lx = _bank_outputs("random7_mixed")[2][refs["model"]]
    ticks = 5
    dx, _, delta, v, w = _disturbed(het.nx, het.ndu, het.ny, B, ticks, 63)

    def sim(**kw):
        return het.simulate(x0, u0, ticks, warm=warm, xhat0=x0 + dx, meas_noise=v, noise=w, **kw, **refs)
    _assert_equals_the_observed_loop(sim, het.nx, het.ndu, B, ticks, Lx, delta, "bank")


# ---------------------------------------------------------------------------------------------
# 2. every tick against the single-step call on the logged estimates, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", ["n1", "n3", "n2_d3", "n5", "quadrotor", "n33", "n32", "n64"])
def test_ticks_equal_the_single_step_call_on_the_estimates(name, warm):
    import torch
    make, inputs, model = SHAPES[name]()
    nx, ndu, ny = model[0].shape[0], model[2].shape[1], model[3].shape[0]
    B, ticks = SINGLE_STEP_B.get(name, 22), 7
    x0, u0, refs = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 64)
    L = _host_gain(model)
    res = make().simulate(x0, u0, ticks, warm=warm, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, **refs)
    assert np.array_equal(_np(res.x[0]), x0) and np.array_equal(_np(res.xhat[0]), x0 + dx) and np.array_equal(_np(res.dhat[0]), dh0)
    assert not torch.equal(res.dhat[1], res.dhat[0])
    _follow(make(), dataclasses.replace(res, x=res.xhat), u0, ticks, "%s offset-free %s" % (name, "warm" if warm else "cold"), warm=warm,
            refs_of_tick=lambda k: dict(dmeas=res.dhat[k]), **refs)


@functools.lru_cache(maxsize=None)
def _bank_models(name):
    """per controller of _bank(name): (A, B, Bd, C, Dd) [K, ...] and the augmented gain"""
    assert name.startswith("random7")
    specs = [random_lmpc_spec(100 + k) for k in range(7)]
    mats = tuple(np.stack([sp[n] for sp in specs]) for n in ("A", "B", "Bd", "C", "Dd"))
    return mats, np.stack([_host_gain(tuple(sp[n] for n in ("A", "B", "Bd", "C", "Dd"))) for sp in specs])


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_ticks_of_a_banks_loop_equal_the_banks_single_step_call_on_the_estimates(warm):
    het, _, B, x0, u0, refs = _bank_case("random7_mixed")
    _, gains = _bank_models("random7_mixed")
    ticks = 7
    dx, dh0, delta, v, w = _disturbed(het.nx, het.ndu, het.ny, B, ticks, 65)
    res = het.simulate(x0, u0, ticks, warm=warm, disturbance_observer=gains[refs["model"]], xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v,
                       noise=w, **refs)
    assert np.array_equal(_np(res.dhat[0]), dh0)
    _follow(het, dataclasses.replace(res, x=res.xhat), u0, ticks, "bank offset-free %s" % ("warm" if warm else "cold"), warm=warm,
            refs_of_tick=lambda k: dict(dmeas=res.dhat[k]), **refs)
    with pytest.raises(ValueError):
        het.simulate(x0, u0, ticks, disturbance_observer=gains[0], **refs)


# ---------------------------------------------------------------------------------------------
# 3. the five linear steps against float64 numpy on the logged inputs
# ---------------------------------------------------------------------------------------------
WORST = {}


def _assert_steps(res, plant_mats, model, L, delta_of_tick, v, w, label):
    """y_k, x_k+1, xhat_k+1 and dhat_k+1 of every tick from the logged x_k, xhat_k, dhat_k, u_k (and the logged y_k for the estimator's two)"""
    x, xh, dh, u, y = (_np(getattr(res, f)) for f in ("x", "xhat", "dhat", "u", "y"))
    B, nx = x.shape[1], x.shape[2]
    Ap, Bp, Bdp = (ref.batchwise(M, B) for M in plant_mats)
    A, Bm, Bd, Cm, Dd = (ref.batchwise(M, B) for M in model)
    Lx, Ld = (ref.batchwise(M, B) for M in ref.split_gain(L, nx))
    worst = dict(y=0.0, x=0.0, xhat=0.0, dhat=0.0)
    for k in range(u.shape[0]):
        d = np.broadcast_to(delta_of_tick(k), dh[k].shape)
        vk, wk = (None if v is None else v[k]), (None if w is None else w[k])
        e = ref.innovation(Cm, Dd, xh[k], dh[k], y[k])
        for q, got, want, bound in (
                ("y", y[k], ref.measure(Cm, Dd, x[k], d, vk), ref.measure_bound(Cm, Dd, x[k], d, vk)),
                ("x", x[k + 1], ref.plant(Ap, Bp, Bdp, x[k], u[k], d, wk), ref.plant_bound(Ap, Bp, Bdp, x[k], u[k], d, wk)),
                ("xhat", xh[k + 1], ref.estimate(A, Bm, Bd, Lx, xh[k], u[k], dh[k], e), ref.estimate_bound(A, Bm, Bd, Cm, Dd, Lx, xh[k], u[k], dh[k], e)),
                ("dhat", dh[k + 1], ref.disturbance(Ld, dh[k], e), ref.disturbance_bound(Cm, Dd, Ld, xh[k], dh[k], e))):
            err = np.abs(got - want)
            worst[q] = max(worst[q], float((err / np.maximum(bound, 1e-300)).max()))
            assert np.isfinite(got).all() and (err <= bound).all(), (label, k, q, float(err.max()))
    print("%s: worst ratio of an error to its bound: y %.3f, x %.3f, xhat %.3f, dhat %.3f" % (label, worst["y"], worst["x"], worst["xhat"], worst["dhat"]))
    for q in worst:
        WORST[q] = max(WORST.get(q, 0.0), worst[q])
    print("so far, over every case: " + ", ".join("%s %.3f" % (q, WORST[q]) for q in ("y", "x", "xhat", "dhat")))


@pytest.mark.parametrize("gains", ["one", "per_instance"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_steps_against_numpy(case, gains):
    name, B = case
    make, inputs, model = SHAPES[name]()
    A, Bm, Bd, Cm, Dd = model
    nx, ndu, ny, ticks = A.shape[0], Bd.shape[1], Cm.shape[0], 5
    x0, u0, refs = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 66)
    L = _host_gain(model)
    if gains == "per_instance":
        L = _scaled(L, B, np.random.default_rng(67))
    plant = (1.02 * A, None, None)              # the plant is not the estimator's model
    res = make().simulate(x0, u0, ticks, plant=plant, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, **refs)
    _assert_steps(res, (1.02 * A, Bm, Bd), model, L, lambda k: delta, v, w, "%s B=%d %s" % (name, B, gains))


@pytest.mark.parametrize("name", ["n3", "n2_d3", "quadrotor"])
def test_the_steps_with_a_preview_disturbance_against_numpy(name):
    """delta_k is row k of a [B, ticks + ph, ndu] array, read by the plant and the measurement directly: the solve no longer sees it"""
    make, inputs, model = SHAPES[name]()
    A, Bm, Bd, Cm, Dd = model
    nx, ndu, ny, B, ticks = A.shape[0], Bd.shape[1], Cm.shape[0], 13, 5
    x0, u0, refs = inputs(B)
    dx, dh0, _, v, w = _disturbed(nx, ndu, ny, B, ticks, 68)
    c = make()
    delta = 0.2 * np.random.default_rng(69).normal(size=(B, ticks + c.ph, ndu))
    L = _host_gain(model)
    res = c.simulate(x0, u0, ticks, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, preview=True, meas_noise=v, noise=w, **refs)
    _assert_steps(res, (A, Bm, Bd), model, L, lambda k: delta[:, k], v, w, "%s preview" % name)
    _follow(make(), dataclasses.replace(res, x=res.xhat), u0, ticks, "%s preview" % name, warm=True, refs_of_tick=lambda k: dict(dmeas=res.dhat[k]), **refs)


def test_the_steps_of_a_bank_with_a_plant_per_instance_against_numpy():
    het, (A, Bm, Bd, d0), B, x0, u0, refs = _bank_case("random7_mixed")
    mats, gains = _bank_models("random7_mixed")
    model = tuple(M[refs["model"]] for M in mats)
    L = gains[refs["model"]]
    ticks = 5
    rng = np.random.default_rng(70)
    dx, dh0, delta, v, w = _disturbed(het.nx, het.ndu, het.ny, B, ticks, 71)
    P = tuple(_scaled(m[0], B, rng) for m in (A, Bm, Bd))           # variations of controller 0's model: no instance's estimator has its plant
    res = het.simulate(x0, u0, ticks, plants=P, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, **refs)
    _assert_steps(res, P, model, L, lambda k: delta, v, w, "bank")
    # each instance's own controller as its plant, each controller's own exogenous input as the true disturbance, no noise
    res = het.simulate(x0, u0, ticks, disturbance_observer=L, xhat0=x0 + dx, **refs)
    assert not np.any(_np(res.dhat[0]))
    _assert_steps(res, (A, Bm, Bd), model, L, lambda k: d0, None, None, "bank own plants")


# ---------------------------------------------------------------------------------------------
# 4. tracking: what the feature is for
# ---------------------------------------------------------------------------------------------
def _tracking_spec(kind):
    """nx = 4, nu = ndu = ny = 2: two stable, minimum-phase channels with a weak random coupling; the disturbance enters at the input
    (Bd = B, Dd = 0) or at the output (Bd = 0, Dd = I)"""
    nx, nu, ndu, ny, ph, ch = 4, 2, 2, 2, 6, 3
    r = np.random.default_rng(7)
    A = np.diag([0.8, 0.7, 0.6, 0.5]) + 0.02 * r.normal(size=(nx, nx))
    Bm = np.array([[1.0, 0.0], [0.5, 0.0], [0.0, 1.0], [0.0, 0.5]]) + 0.05 * r.normal(size=(nx, nu))
    Cm = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]]) + 0.05 * r.normal(size=(ny, nx))
    Bd, Dd = (Bm.copy(), np.zeros((ny, ndu))) if kind == "input" else (np.zeros((nx, ndu)), np.eye(ny))
    return dict(dims=(nx, nu, ndu, ny, ph, ch), A=A, B=Bm, C=Cm, Bd=Bd, Dd=Dd, yref=np.array([0.5, -0.3]))


def _configure_tracking(c, sp):
    """no input weight (no steady-state target is computed: only then is the reference a fixed point), a move weight, bounds far outside"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    assert c.setStateSpaceModel(sp["A"], sp["B"], sp["C"])
    assert c.setDisturbances(sp["Bd"], sp["Dd"])
    assert c.setObjectiveWeights(np.ones(ny), np.zeros(nu), 0.1 * np.ones(nu), (0, ph))
    assert c.setInputBounds(-100 * np.ones(nu), 100 * np.ones(nu), (0, ch))
    assert c.setReferences(sp["yref"], np.zeros(nu), np.zeros(nu), (0, ph))
    return c


@pytest.mark.parametrize("kind", ["input", "output"])
def test_the_outputs_settle_on_their_reference_where_a_state_observer_leaves_an_offset(kind):
    """B = 8 mismatched plants (A + 0.03 N_b, s_b B with s_b in [0.9, 1.1]) under a constant load at the input that nobody measures (it enters as
    the loop's process disturbance w = B_p load), 100 ticks, no noise.  The yardstick is the same loop on the host, its solves the CPU oracle's
    and its tick tests/lmpc_offset_free_ref.py's: r_of its final max |y - yref| with the augmented estimator, r_plain with the state observer.
    The figures are in DESIGN 4.3d."""
    import torch
    from libmpc_amd import LMPC
    from libmpc_amd.utils import disturbance_gains
    from oracle.lmpc_oracle import default_params
    sp = _tracking_spec(kind)
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    B, ticks = 8, 100
    r = np.random.default_rng(11)
    Ap = sp["A"][None] + 0.03 * r.normal(size=(B, nx, nx))
    Bp = sp["B"][None] * r.uniform(0.9, 1.1, size=(B, 1, 1))
    load = np.array([0.3, -0.2]) * r.uniform(0.5, 1.5, size=(B, 1))
    W = np.broadcast_to(ref.mv(Bp, load), (ticks, B, nx)).copy()
    x0, u0 = 0.2 * r.normal(size=(B, nx)), np.zeros((B, nu))
    plants = (Ap, Bp, np.zeros((B, nx, ndu)))
    model = tuple(sp[k] for k in ("A", "B", "Bd", "C", "Dd"))

    c = _configure_tracking(LMPC(*sp["dims"], device=0), sp)
    Qw, Qd, Rv = 0.01 * np.eye(nx), np.eye(ndu), 1e-4 * np.eye(ny)
    L, _, flags = disturbance_gains(*(np.broadcast_to(M, (B,) + M.shape) for M in (sp["A"], sp["Bd"], sp["C"], sp["Dd"])), Qw, Qd, Rv)
    assert not flags.any() and tuple(L.shape) == (B, nx + ndu, ny)
    assert torch.equal(L[0], torch.as_tensor(c.disturbance_gain(Qw, Qd, Rv)).cuda())
    Lp = c.kalman_gain(Qw, Rv)

    f = _configure_tracking(OracleFrontEnd(*sp["dims"]), sp)
    f.o.params = default_params(maximum_iteration=4000)

    def solve(xh, u, dh):
        out = [f.optimize(xh[b], u[b], dMeas=np.tile(dh[b][:, None], (1, ph))) for b in range(B)]
        assert all(o["polished"] for o in out)
        return np.stack([o["cmd"] for o in out])
    yref = sp["yref"]
    r_of = np.abs(ref.host_loop(solve, plants, model, _np(L), x0, u0, ticks, w=W)[4][-1] - yref).max()
    r_plain = np.abs(ref.host_loop(solve, plants, model, Lp, x0, u0, ticks, w=W)[4][-1] - yref).max()

    off = c.simulate(x0, u0, ticks, plants=plants, noise=W, disturbance_observer=L)
    plain = c.simulate(x0, u0, ticks, plants=plants, noise=W, observer=Lp)
    assert int((off.status != 0).sum()) == 0 and int(off.active_count[-1].max()) == 0          # the steady state is interior
    e_of = float((off.y[-1] - torch.as_tensor(yref).cuda()).abs().max())
    e_plain = float((plain.y[-1] - torch.as_tensor(yref).cuda()).abs().max())
    print("%s-disturbance model: final max |y - yref|: host loop %.3e offset-free, %.3e state observer (ratio %.1e); device loop %.3e offset-free, %.3e state observer"
          % (kind, r_of, r_plain, r_plain / r_of, e_of, e_plain))
    assert r_plain / r_of >= 1e6, (r_of, r_plain)
    assert e_of <= 10 * r_of + 1e-9 * np.abs(yref).max(), (e_of, r_of)
    assert e_plain >= r_plain / 2, (e_plain, r_plain)


# ---------------------------------------------------------------------------------------------
# 5. re-run, refills in place, replay past the end, logging off, invalidation
# ---------------------------------------------------------------------------------------------
def test_rerun_refills_replay_past_the_end_logging_off_and_invalidation():
    import ctypes as C
    import torch
    from libmpc_amd import LMPC, MpcxError, _capi
    make, inputs, model = SHAPES["n5"]()
    A, Bm, Bd, Cm, Dd = model
    nx, ndu, ny, B, ticks = 5, 2, 2, 13, 4
    x0, u0, refs = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 72)
    L = _scaled(_host_gain(model), B, np.random.default_rng(73))
    c = make()
    kw = dict(disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w)
    loop = c.make_loop(x0, u0, ticks, **kw, **refs)
    fields = FIELDS + ("dhat",)
    try:
        runs = []
        for _ in range(2):
            res = c.run_loop(loop)
            torch.cuda.synchronize()
            runs.append({k: getattr(res, k).clone() for k in fields})
        for k in fields:
            assert torch.equal(runs[0][k], runs[1][k]), k
        assert int((runs[0]["status"] == 0).sum()) > 0
        _assert_steps(res, (A, Bm, Bd), model, L, lambda k: delta, v, w, "second run")

        # one replay more than `ticks`: the counter stands at `ticks` and nothing is written, the estimates included
        lib = _capi.lib()
        tick = C.c_int(-1)
        _capi.check(lib.mpcx_lmpc_loop_debug_tick(loop.handle, C.byref(tick)))
        assert tick.value == ticks
        for k in fields:
            getattr(loop.result, k).add_(1.0 if getattr(loop.result, k).is_floating_point() else 1)
        torch.cuda.synchronize()
        _capi.check(lib.mpcx_lmpc_loop_debug_replay(loop.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        _capi.check(lib.mpcx_lmpc_loop_debug_tick(loop.handle, C.byref(tick)))
        torch.cuda.synchronize()
        assert tick.value == ticks
        for k in fields:
            assert torch.equal(getattr(loop.result, k), runs[0][k] + 1), k

        # dhat0 refilled in place: the next run starts its estimate there
        assert loop.dhat0 is not None and loop.xhat0 is not None and loop.gains is not None
        new = torch.as_tensor(-dh0).cuda()
        loop.dhat0.copy_(new)
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        assert torch.equal(res.dhat[0], new) and torch.equal(res.xhat[0], runs[0]["xhat"][0]) and not torch.equal(res.dhat[1], runs[0]["dhat"][1])
        _assert_steps(res, (A, Bm, Bd), model, L, lambda k: delta, v, w, "refilled dhat0")
        # the gains refilled: other gains estimate otherwise, within the bounds of their own steps
        L2 = 0.5 * L
        before = res.dhat.clone()
        loop.gains.copy_(LMPC.pack_gains(torch.as_tensor(L2).cuda()))
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        assert not torch.equal(res.dhat, before)
        _assert_steps(res, (A, Bm, Bd), model, L2, lambda k: delta, v, w, "refilled gains")
        kept = {k: getattr(res, k).clone() for k in fields}
    finally:
        c.destroy_loop(loop)

    # the same run without the log of dhat: every other log bit-identical (the descriptor by hand: the front-end always logs)
    real = _capi.lib().mpcx_lmpc_loop_create_offset_free

    class _NoDhatLog:
        def __getattr__(self, name):
            return getattr(_capi.lib(), name)

        @staticmethod
        def mpcx_lmpc_loop_create_offset_free(h, d, od, s, out):
            od._obj.traj_dhat = None
            return real(h, d, od, s, out)
    c._lib = _NoDhatLog()
    try:
        kw2 = dict(kw, disturbance_observer=L2, dhat0=-dh0)
        res = c.simulate(x0, u0, ticks, **kw2, **refs)
    finally:
        c._lib = _capi.lib()
    assert not res.dhat.any()                      # nothing was logged
    for k in FIELDS:
        assert torch.equal(getattr(res, k), kept[k]), k

    # a setter invalidates the loop
    loop = c.make_loop(x0, u0, ticks, **kw, **refs)
    try:
        c.setReferences(np.zeros(ny), np.zeros(c.nu), np.zeros(c.nu), (0, c.ph))
        with pytest.raises(MpcxError) as e:
            c.run_loop(loop)
        assert e.value.code == _capi.E_STATE
    finally:
        c.destroy_loop(loop)
    c.destroy_loop(loop)          # idempotent


# ---------------------------------------------------------------------------------------------
# 6. the gains: the augmented equation against its 60-digit solution, and into the loop as they come
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gain_truths():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offset_free_gain_truth.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["random", "quadrotor"])
def test_disturbance_gains_solve_the_augmented_equation_and_enter_the_loop_unpacked(name):
    """the bound is the Riccati kernel's own (tests/dare_ref.py): |error| <= C n 2^-52 max|truth| for P and for the gain, n = nx + ndu"""
    import torch
    import dare_ref
    from libmpc_amd import LMPC
    from libmpc_amd.utils import disturbance_gains
    t = {k.split(".", 1)[1]: v for k, v in _gain_truths().items() if k.startswith(name + ".")}
    nx, ndu, ny = t["A"].shape[0], t["Bd"].shape[1], t["C"].shape[0]
    B = 3
    L, P, flags = disturbance_gains(*(np.broadcast_to(t[k], (B,) + t[k].shape) for k in ("A", "Bd", "C", "Dd")), t["Qw"], t["Qd"], t["Rv"])
    assert not flags.any() and tuple(L.shape) == (B, nx + ndu, ny) and tuple(P.shape) == (B, nx + ndu, nx + ndu)
    rx, rg = dare_ref.ratios(_np(P), _np(L), np.broadcast_to(t["P"], (B,) + t["P"].shape), np.broadcast_to(t["L"], (B,) + t["L"].shape))
    print("%s: augmented equation, worst error / bound: P %.4f, gain %.4f" % (name, rx / dare_ref.C_BOUND, rg / dare_ref.C_BOUND))
    assert rx <= dare_ref.C_BOUND and rg <= dare_ref.C_BOUND, (name, rx, rg)

    # what came back is a view of gain_batch's layout: packing it copies nothing, and the loop estimates with exactly these numbers
    assert LMPC.pack_gains(L).data_ptr() == L.data_ptr()
    make, inputs, model = SHAPES["n3" if name == "random" else "quadrotor"]()
    assert np.array_equal(model[0], t["A"]) and np.array_equal(model[2], t["Bd"]) and np.array_equal(model[3], t["C"])
    x0, u0, refs = inputs(B)
    ticks = 4
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 74)
    c = make()
    loop = c.make_loop(x0, u0, ticks, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, **refs)
    try:
        assert loop.gains.data_ptr() == L.data_ptr()
        res = c.run_loop(loop)
        torch.cuda.synchronize()
    finally:
        c.destroy_loop(loop)
    _assert_steps(res, model[:3], model, _np(L), lambda k: delta, v, w, "%s device gains" % name)
    one = c.simulate(x0, u0, ticks, disturbance_observer=_np(L[0]), xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, **refs)
    for k in FIELDS + ("dhat",):
        assert torch.equal(getattr(one, k), getattr(res, k)), k
