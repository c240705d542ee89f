"""Steady-state targets on the device: the map kernel (libmpc_amd.utils.target_maps, mpcx_target_map_batch), the product
(utils.steady_state_inputs, mpcx_target_apply_batch) and the offset-free loop with targets (LMPC / LMPCHetero .simulate / make_loop with
target=, mpcx_lmpc_loop_create_offset_free_target): the solve of tick k reads us_k = T [r_k; dhat_k; ubar_k] as its input reference.

Yardsticks: the 60-digit truths of tests/golden/target_truth.npz within the bound of tests/target_ref.py; the offset-free loop of
tests/test_lmpc_offset_free_gpu.py (bit for bit with T = [0 | 0 | I] and ubar as its per-instance uref: the summation-order contract); the
single-step call on the logged estimates and input references (bit for bit); the stand-alone product (bit for bit) and float64 numpy within
(nrhs + 2) 2^-52 sum|t||v|; a host loop of the CPU oracle's solves and the numpy tick of tests/lmpc_offset_free_ref.py for the tracking error.

Shapes (nx, nu, ndu, ny): (1,1,1,1) at B = 1, 64, 65 -- a full tile of 64 instances and one over; (3,2,1,2) at B = 22 -- 21 per wavefront; (2,3,2,2)
at B = 33 -- more rows of us than lanes of an instance, 32 per wavefront and one over; (5,4,2,2) at B = 13 -- 12 per wavefront, 4 idle lanes, two
tiles; the quadrotor with outputs (x, y, z, yaw), Bd = B, Dd = 0 at B = 6 -- 5 per wavefront; (33,3,2,3) with ph = 3, ch = 2 at B = 3 -- one
instance per wavefront; (32,3,2,3) at B = 5 -- two instances fill the 64 lanes exactly, two full tiles and a half; (64,3,2,3) at B = 3 -- every lane a
state row."""
import dataclasses

import numpy as np
import pytest

import lmpc_offset_free_ref as ref
import target_ref as R
from helpers import OracleFrontEnd
from test_lmpc_loop_gpu import EQUAL, _follow, _np
from test_lmpc_loop_fleet_gpu import _bank_case, _scaled
from test_lmpc_offset_free_gpu import SINGLE_STEP_B, _bank_models, _configure_tracking, _disturbed, _host_gain, _random_of, _tracking_spec

pytestmark = pytest.mark.gpu

FIELDS = ("x", "u") + EQUAL + ("xhat", "y", "dhat")


def _quadrotor():
    from libmpc_amd.workloads import quadrotor_batch, quadrotor_target_lmpc, quadrotor_target_model

    def inputs(B):
        x0, u0, yref = quadrotor_batch(B)
        return x0, u0, dict(yref=np.ascontiguousarray(yref[:, [3, 4, 5, 2]]))
    return (lambda device=0: quadrotor_target_lmpc(10, device=device)), inputs, quadrotor_target_model()


SHAPES = {
    "n1": lambda: _random_of(nx=1, nu=1, ndu=1, ny=1),
    "n3": lambda: _random_of(nx=3, nu=2, ndu=1, ny=2),
    "n2_u3": lambda: _random_of(nx=2, nu=3, ndu=2, ny=2),
    "n5": lambda: _random_of(nx=5, nu=4, ndu=2, ny=2),
    "quadrotor": _quadrotor,
    "n33": lambda: _random_of(nx=33, nu=3, ndu=2, ny=3, ph=3, ch=2),
    "n32": lambda: _random_of(nx=32, nu=3, ndu=2, ny=3, ph=3, ch=2),
    "n64": lambda: _random_of(nx=64, nu=3, ndu=2, ny=3, ph=3, ch=2),
}
CASES = [("n1", 1), ("n1", 64), ("n1", 65), ("n3", 22), ("n2_u3", 33), ("n5", 13), ("quadrotor", 6), ("n33", 3), ("n32", 5), ("n64", 3)]
CASE_IDS = ["%s-B%d" % c for c in CASES]


def _dims(model):
    A, Bm, Bd, Cm, _ = model
    return A.shape[0], Bm.shape[1], Bd.shape[1], Cm.shape[0]


def _pass_through(nu, ndu, ny):
    """T = [0 | 0 | I]: us = ubar"""
    return np.concatenate([np.zeros((nu, ny + ndu)), np.eye(nu)], axis=1)


def _own_references(name, model):
    """step 0 of the references the controller of SHAPES[name] was given: the quadrotor's set-point, or the random spec's"""
    from helpers import random_lmpc_spec
    if name == "quadrotor":
        return np.array([0.0, 0.0, 1.0, 0.0]), np.zeros(4)
    nx, nu, ndu, ny = _dims(model)
    sp = random_lmpc_spec(3, nx=nx, nu=nu, ndu=ndu, ny=ny)
    assert np.array_equal(sp["A"], model[0])
    return sp["yref"][:, 0], sp["uref"][:, 0]


def _numpy_map(model):
    Tu, _ = R.numpy_maps(*(M[None] for M in model))
    return Tu[0]


# ---------------------------------------------------------------------------------------------
# 1. the map kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FAMILIES)
def test_maps_against_the_truth(name):
    from libmpc_amd.utils import target_maps
    Tu, Tx, flags = target_maps(*R.model(name), want_x=True)
    assert not flags.any()
    R.check_family(name, _np(Tu), _np(Tx), " (device)")
    only_u, flags = target_maps(*R.model(name))
    assert not flags.any() and np.array_equal(_np(only_u), _np(Tu))


def test_singular_instances_are_flagged_and_leave_their_neighbours_alone():
    """a batch of good instances with, among them, an integrator that the outputs do not see, an input matrix that reaches nothing (dyadic
    entries: the elimination meets an exact zero) and a NaN: flag 1 and NaN throughout for those, the bits of a call of their own for the others.
    The host's rank check is switched off: it would refuse the batch."""
    from libmpc_amd.utils import target_maps
    A, B, Bd, C, Dd = (np.concatenate([np.array(a), np.array(a)], axis=0) for a in R.model("shape_2_1_1_1"))
    bad, good = [1, 3, 4], [0, 2, 5]
    A[1] = [[1.0, 0.0], [0.0, 0.5]]; C[1] = [[0.0, 1.0]]
    A[3] = [[0.5, 0.25], [0.0, 0.5]]; B[3] = 0.0; C[3] = [[1.0, 0.0]]
    A[4, 0, 1] = np.nan
    with pytest.raises(ValueError, match="rank"):
        target_maps(A[:4], B[:4], Bd[:4], C[:4], Dd[:4])
    Tu, Tx, flags = target_maps(A, B, Bd, C, Dd, want_x=True, check_rank=False)
    assert flags.tolist() == [0, 1, 0, 1, 1, 0]
    assert np.isnan(_np(Tu)[bad]).all() and np.isnan(_np(Tx)[bad]).all()
    alone = target_maps(A[good], B[good], Bd[good], C[good], Dd[good], want_x=True)
    assert np.array_equal(_np(Tu)[good], _np(alone[0])) and np.array_equal(_np(Tx)[good], _np(alone[1])) and not alone[2].any()


def test_more_outputs_than_inputs_are_singular():
    """ny > nu: rank [[I - A, -B], [C, 0]] < nx + ny whatever the entries; dyadic entries, so the elimination ends in an exact zero pivot"""
    from libmpc_amd.utils import target_maps
    A = np.array([[[0.5]]]); B = np.array([[[1.0]]]); C = np.array([[[1.0], [2.0]]])
    Tu, Tx, flags = target_maps(A, B, B.copy(), C, np.zeros((1, 2, 1)), want_x=True, check_rank=False)
    assert flags.tolist() == [1] and np.isnan(_np(Tu)).all() and np.isnan(_np(Tx)).all()


def test_the_input_reference_term_is_a_symmetric_projector_and_zero_in_the_square_case():
    """nu = ny: the constraints determine us and Tu = 0 (to the scale of the bound).  nu > ny: Tu projects ubar orthogonally onto the inputs that
    move no output in steady state -- symmetric and idempotent to the scale of the bound -- and rank nu - ny"""
    from libmpc_amd.utils import target_maps
    for name in R.SQUARE + R.WIDE + ["quadrotor", "chain", "limit"]:
        nx, nu, ndu, ny = R.dims(name)
        Tu = _np(target_maps(*R.model(name))[0])[:, :, ny + ndu:]
        tol = R.C_BOUND * (2 * nx + nu + ny) * R.U * R.case(name)["cond"].max()
        if nu == ny:
            assert np.abs(Tu).max() <= tol, name
        else:
            assert np.abs(Tu - np.swapaxes(Tu, 1, 2)).max() <= 4 * tol and np.abs(Tu @ Tu - Tu).max() <= 4 * tol, name
            assert (np.linalg.matrix_rank(Tu, tol=1e-8) == nu - ny).all(), name


# ---------------------------------------------------------------------------------------------
# 2. with T = [0 | 0 | I] the loop is the offset-free loop given ubar as its per-instance uref, bit for bit
# ---------------------------------------------------------------------------------------------
def _assert_equals_the_offset_free_loop(sim, T, ubar, B, ticks, label):
    import torch
    off = sim(uref=ubar)
    tgt = sim(uref=ubar, target=T)
    print("%s: %d of %d solves end with status 0" % (label, int((off.status == 0).sum()), off.status.numel()))
    for f in FIELDS:
        a, b = getattr(tgt, f), getattr(off, f)
        assert torch.equal(a, b), (label, f, int((a != b).sum()))
    assert off.us is None and tuple(tgt.us.shape) == (ticks + 1, B, ubar.shape[1])
    want = torch.as_tensor(ubar).cuda().expand(ticks + 1, B, ubar.shape[1])
    assert torch.equal(tgt.us.view(torch.int64), want.contiguous().view(torch.int64)), label


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_with_a_pass_through_map_the_loop_is_the_offset_free_loop_bit_for_bit(case, warm):
    name, B = case
    make, inputs, model = SHAPES[name]()
    nx, nu, ndu, ny = _dims(model)
    ticks = 5
    x0, u0, refs = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 81)
    rng = np.random.default_rng(82)
    ubar = 0.1 * rng.normal(size=(B, nu))
    c = make()
    L = _host_gain(model)

    def sim(**kw):
        return c.simulate(x0, u0, ticks, warm=warm, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, **kw, **refs)
    T = _pass_through(nu, ndu, ny)
    # one map and one gain; a map and a gain per instance
    _assert_equals_the_offset_free_loop(lambda **kw: sim(disturbance_observer=L, **kw), T, ubar, B, ticks, "%s B=%d one map" % case)
    Lb = _scaled(L, B, rng)
    _assert_equals_the_offset_free_loop(lambda **kw: sim(disturbance_observer=Lb, **kw), np.broadcast_to(T, (B,) + T.shape).copy(), ubar, B, ticks,
                                        "%s B=%d maps" % case)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_a_bank_with_pass_through_maps_is_its_offset_free_loop_bit_for_bit(warm):
    het, _, B, x0, u0, refs = _bank_case("random7_mixed")
    _, gains = _bank_models("random7_mixed")
    ticks = 5
    dx, dh0, delta, v, w = _disturbed(het.nx, het.ndu, het.ny, B, ticks, 83)
    ubar = 0.1 * np.random.default_rng(84).normal(size=(B, het.nu))
    T = _pass_through(het.nu, het.ndu, het.ny)

    def sim(**kw):
        return het.simulate(x0, u0, ticks, warm=warm, disturbance_observer=gains[refs["model"]], xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v,
                            noise=w, **kw, **refs)
    _assert_equals_the_offset_free_loop(sim, np.broadcast_to(T, (B,) + T.shape).copy(), ubar, B, ticks, "bank")
    with pytest.raises(ValueError, match="bank"):
        sim(target=T)


# ---------------------------------------------------------------------------------------------
# 3. every tick against the single-step call, and every us against the stand-alone product and numpy
# ---------------------------------------------------------------------------------------------
def _assert_us(res, T, r_of_tick, ubar_of_tick, label):
    """us[k] = T [r_k; dhat_k; ubar_k] for k = 0 .. ticks: the stand-alone product's bits, and float64 numpy within (nrhs + 2) 2^-52 sum|t||v|"""
    import torch
    from libmpc_amd.utils import steady_state_inputs
    us, dh = _np(res.us), _np(res.dhat)
    B, nu = us.shape[1], us.shape[2]
    Tn = ref.batchwise(_np(T) if hasattr(T, "cpu") else T, B)
    nrhs = Tn.shape[2]
    worst = 0.0
    for k in range(us.shape[0]):
        r = np.ascontiguousarray(np.broadcast_to(r_of_tick(k), (B, nrhs - nu - dh.shape[2])))
        ub = np.ascontiguousarray(np.broadcast_to(ubar_of_tick(k), (B, nu)))
        alone = steady_state_inputs(T, r, res.dhat[k], ub)
        assert torch.equal(res.us[k].view(torch.int64), alone.view(torch.int64)), (label, k)
        vec = np.concatenate([r, dh[k], ub], axis=1)
        err, bound = np.abs(us[k] - ref.mv(Tn, vec)), (nrhs + 2) * ref.EPS * ref.mv(np.abs(Tn), np.abs(vec))
        assert np.isfinite(us[k]).all() and (err <= bound).all(), (label, k, float(err.max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("%s: us against numpy, worst error / bound %.3f" % (label, worst))


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", ["n1", "n3", "n2_u3", "n5", "quadrotor", "n33", "n32", "n64"])
def test_ticks_equal_the_single_step_call_on_the_estimates_and_targets(name, warm):
    import torch
    from libmpc_amd.utils import target_maps
    make, inputs, model = SHAPES[name]()
    nx, nu, ndu, ny = _dims(model)
    B, ticks = SINGLE_STEP_B.get(name, 22), 7
    x0, u0, refs = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 85)
    rng = np.random.default_rng(86)
    yref = refs.get("yref", 0.3 * rng.normal(size=(B, ny)))
    ubar = 0.1 * rng.normal(size=(B, nu))
    L = _host_gain(model)
    c = make()
    T = c.target_map()
    maps, flags = target_maps(*(np.broadcast_to(M, (B,) + M.shape) for M in model))
    assert not flags.any() and np.array_equal(_np(maps[0]), T)
    kw = dict(warm=warm, disturbance_observer=L, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, yref=yref, uref=ubar)
    res = c.simulate(x0, u0, ticks, target=T, **kw)
    assert np.array_equal(_np(res.dhat[0]), dh0) and not torch.equal(res.us[1], res.us[0])
    label = "%s targets %s" % (name, "warm" if warm else "cold")
    _follow(make(), dataclasses.replace(res, x=res.xhat), u0, ticks, label, warm=warm, refs_of_tick=lambda k: dict(dmeas=res.dhat[k], uref=res.us[k]),
            yref=yref)
    _assert_us(res, T, lambda k: yref, lambda k: ubar, label)
    # a map per instance as the map kernel wrote it: not copied on its way into the loop, and the same run
    loop = c.make_loop(x0, u0, ticks, target=maps, **kw)
    try:
        assert loop.maps.data_ptr() == maps.data_ptr()
        per = c.run_loop(loop)
        torch.cuda.synchronize()
        for f in FIELDS + ("us",):
            assert torch.equal(getattr(per, f), getattr(res, f)), (label, f)
    finally:
        c.destroy_loop(loop)


@pytest.mark.parametrize("name", ["n3", "n2_u3", "quadrotor"])
def test_preview_and_shared_references_feed_the_targets_with_step_zero(name):
    """yref and uref as [B, ticks + ph, n] previews: r_k and ubar_k are row k, and the solve still sees the window of yref (uref's window is
    gone: the solve reads us_k).  Then None: the controller's own references, step 0."""
    import torch
    make, inputs, model = SHAPES[name]()
    nx, nu, ndu, ny = _dims(model)
    B, ticks = 13, 5
    x0, u0, _ = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 87)
    c = make()
    rng = np.random.default_rng(88)
    yref = 0.3 * rng.normal(size=(B, ticks + c.ph, ny)); ubar = 0.1 * rng.normal(size=(B, ticks + c.ph, nu))
    if name == "quadrotor":
        yref[:, :, 2] += 1.0
    L, T = _host_gain(model), _numpy_map(model)
    kw = dict(disturbance_observer=L, target=T, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w)
    res = c.simulate(x0, u0, ticks, yref=yref, uref=ubar, preview=True, **kw)
    _assert_us(res, T, lambda k: yref[:, k], lambda k: ubar[:, k], "%s preview" % name)
    _follow(make(), dataclasses.replace(res, x=res.xhat), u0, ticks, "%s preview" % name, warm=True,
            refs_of_tick=lambda k: dict(dmeas=res.dhat[k], uref=res.us[k], yref=np.ascontiguousarray(yref[:, k:k + c.ph])))
    # per step, [B, ph, n]: step 0 at every tick
    res = c.simulate(x0, u0, ticks, yref=yref[:, :c.ph].copy(), uref=ubar[:, :c.ph].copy(), **kw)
    _assert_us(res, T, lambda k: yref[:, 0], lambda k: ubar[:, 0], "%s per step" % name)
    # the controller's own
    res = c.simulate(x0, u0, ticks, **kw)
    own_y, own_u = _own_references(name, model)
    _assert_us(res, T, lambda k: own_y, lambda k: own_u, "%s own references" % name)
    _follow(make(), dataclasses.replace(res, x=res.xhat), u0, ticks, "%s own references" % name, warm=True,
            refs_of_tick=lambda k: dict(dmeas=res.dhat[k], uref=res.us[k]))


def test_ticks_of_a_banks_loop_with_targets():
    """a bank: a map per instance from LMPCHetero.target_maps, each controller's own references as r and ubar"""
    import torch
    from helpers import random_lmpc_spec
    het, _, B, x0, u0, refs = _bank_case("random7_mixed")
    mats, gains = _bank_models("random7_mixed")
    ticks = 6
    dx, dh0, delta, v, w = _disturbed(het.nx, het.ndu, het.ny, B, ticks, 89)
    maps = het.target_maps()
    assert tuple(maps.shape) == (het.count, het.nu, het.ny + het.ndu + het.nu)
    want, _ = R.numpy_maps(*mats)
    assert np.allclose(_np(maps), want, rtol=1e-9, atol=1e-12)
    T = maps[torch.as_tensor(refs["model"]).cuda().long()]
    res = het.simulate(x0, u0, ticks, disturbance_observer=gains[refs["model"]], target=T, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v,
                       noise=w, **refs)
    specs = [random_lmpc_spec(100 + k) for k in range(7)]
    own_y = np.stack([sp["yref"][:, 0] for sp in specs])[refs["model"]]; own_u = np.stack([sp["uref"][:, 0] for sp in specs])[refs["model"]]
    _assert_us(res, T, lambda k: own_y, lambda k: own_u, "bank")
    _follow(het, dataclasses.replace(res, x=res.xhat), u0, ticks, "bank targets", warm=True,
            refs_of_tick=lambda k: dict(dmeas=res.dhat[k], uref=res.us[k]), **refs)


# ---------------------------------------------------------------------------------------------
# 4. tracking: what the feature is for
# ---------------------------------------------------------------------------------------------
def _configure_weighted(c, sp):
    """the tracking set-up of tests/test_lmpc_offset_free_gpu.py with an input weight of 1"""
    _configure_tracking(c, sp)
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    assert c.setObjectiveWeights(np.ones(ny), np.ones(nu), 0.1 * np.ones(nu), (0, ph))
    return c


@pytest.mark.parametrize("kind", ["input", "output"])
def test_the_outputs_settle_on_their_reference_under_an_input_weight(kind):
    """The set-up of the offset-free tracking test -- two disturbance models, B = 8 mismatched plants under a constant load nobody measures, 100
    ticks, no noise -- with UW = 1 in place of 0: the input term now pulls the steady state off the reference unless the input reference is
    the steady-state input.  The yardstick is the loop on the host, its solves the CPU oracle's, its tick tests/lmpc_offset_free_ref.py's and
    its targets from a numpy solve of the KKT system: r_tgt its final max |y - yref| with targets, r_none without.  The figures are in
    DESIGN 4.3e."""
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
    yref = sp["yref"]

    c = _configure_weighted(LMPC(*sp["dims"], device=0), sp)
    Qw, Qd, Rv = 0.01 * np.eye(nx), np.eye(ndu), 1e-4 * np.eye(ny)
    L, _, flags = disturbance_gains(*(np.broadcast_to(M, (B,) + M.shape) for M in (sp["A"], sp["Bd"], sp["C"], sp["Dd"])), Qw, Qd, Rv)
    assert not flags.any()
    T = c.target_map()
    Tn = _numpy_map(model)
    assert np.allclose(T, Tn, rtol=1e-10, atol=1e-13)

    f = _configure_weighted(OracleFrontEnd(*sp["dims"]), sp)
    f.o.params = default_params(maximum_iteration=4000)

    def solver(targets):
        def solve(xh, u, dh):
            us = ref.mv(ref.batchwise(Tn, B), np.concatenate([np.broadcast_to(yref, (B, ny)), dh, np.zeros((B, nu))], axis=1)) if targets else np.zeros((B, nu))
            out = [f.optimize(xh[b], u[b], uRef=np.tile(us[b][:, None], (1, ph)), dMeas=np.tile(dh[b][:, None], (1, ph))) for b in range(B)]
            assert all(o["polished"] for o in out)
            return np.stack([o["cmd"] for o in out])
        return solve
    r_tgt = np.abs(ref.host_loop(solver(True), plants, model, _np(L), x0, u0, ticks, w=W)[4][-1] - yref).max()
    r_none = np.abs(ref.host_loop(solver(False), plants, model, _np(L), x0, u0, ticks, w=W)[4][-1] - yref).max()

    tgt = c.simulate(x0, u0, ticks, plants=plants, noise=W, disturbance_observer=L, target=T)
    none = c.simulate(x0, u0, ticks, plants=plants, noise=W, disturbance_observer=L)
    e_tgt = float((tgt.y[-1] - torch.as_tensor(yref).cuda()).abs().max())
    e_none = float((none.y[-1] - torch.as_tensor(yref).cuda()).abs().max())
    print("%s-disturbance model, UW = 1: final max |y - yref|: host loop %.3e with targets, %.3e without (ratio %.1e); device loop %.3e with targets, %.3e without"
          % (kind, r_tgt, r_none, r_none / r_tgt, e_tgt, e_none))
    assert r_none / r_tgt >= 1e6, (r_tgt, r_none)
    assert e_tgt <= 10 * r_tgt + 1e-9 * np.abs(yref).max(), (e_tgt, r_tgt)
    assert e_none >= r_none / 2, (e_none, r_none)
    assert int((tgt.status != 0).sum()) == 0 and int(tgt.active_count[-1].max()) == 0          # the steady state is interior


# ---------------------------------------------------------------------------------------------
# 5. re-run, the maps refilled in place, replay past the end, logging off, invalidation
# ---------------------------------------------------------------------------------------------
def test_rerun_refill_replay_past_the_end_logging_off_and_invalidation():
    import ctypes as C
    import torch
    from libmpc_amd import LMPC, MpcxError, _capi
    make, inputs, model = SHAPES["n5"]()
    nx, nu, ndu, ny = _dims(model)
    B, ticks = 13, 4
    x0, u0, refs = inputs(B)
    dx, dh0, delta, v, w = _disturbed(nx, ndu, ny, B, ticks, 90)
    rng = np.random.default_rng(91)
    yref, ubar = 0.3 * rng.normal(size=(B, ny)), 0.1 * rng.normal(size=(B, nu))
    L = _host_gain(model)
    T = _scaled(_numpy_map(model), B, rng)
    c = make()
    kw = dict(disturbance_observer=L, target=T, xhat0=x0 + dx, dhat0=dh0, dmeas=delta, meas_noise=v, noise=w, yref=yref, uref=ubar)
    loop = c.make_loop(x0, u0, ticks, **kw)
    fields = FIELDS + ("us",)
    try:
        runs = []
        for _ in range(2):
            res = c.run_loop(loop)
            torch.cuda.synchronize()
            runs.append({k: getattr(res, k).clone() for k in fields})
        for k in fields:
            assert torch.equal(runs[0][k], runs[1][k]), k
        assert int((runs[0]["status"] == 0).sum()) > 0
        _assert_us(res, T, lambda k: yref, lambda k: ubar, "second run")

        # one replay more than `ticks`: the counter stands at `ticks` and nothing is written, the targets included
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

        # the maps refilled in place: the next run computes its targets, the first one included, with them
        assert loop.maps is not None and tuple(loop.maps.shape) == (B, nu * (ny + ndu + nu))
        T2 = 0.5 * T
        loop.maps.copy_(LMPC.pack_gains(torch.as_tensor(T2).cuda()))
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        assert not torch.equal(res.us[0], runs[0]["us"][0])
        _assert_us(res, T2, lambda k: yref, lambda k: ubar, "refilled maps")
        kept = {k: getattr(res, k).clone() for k in fields}
    finally:
        c.destroy_loop(loop)

    # the same run without the log of us: every other log bit-identical (the descriptor by hand: the front-end always logs)
    real = _capi.lib().mpcx_lmpc_loop_create_offset_free_target

    class _NoUsLog:
        def __getattr__(self, name):
            return getattr(_capi.lib(), name)

        @staticmethod
        def mpcx_lmpc_loop_create_offset_free_target(h, d, od, td, s, out):
            td._obj.traj_us = None
            return real(h, d, od, td, s, out)
    c._lib = _NoUsLog()
    try:
        res = c.simulate(x0, u0, ticks, **dict(kw, target=T2))
    finally:
        c._lib = _capi.lib()
    assert not res.us.any()                        # nothing was logged
    for k in FIELDS:
        assert torch.equal(getattr(res, k), kept[k]), k

    # a setter invalidates the loop
    loop = c.make_loop(x0, u0, ticks, **kw)
    try:
        c.setReferences(np.zeros(ny), np.zeros(nu), np.zeros(nu), (0, c.ph))
        with pytest.raises(MpcxError) as e:
            c.run_loop(loop)
        assert e.value.code == _capi.E_STATE
    finally:
        c.destroy_loop(loop)
    c.destroy_loop(loop)          # idempotent
