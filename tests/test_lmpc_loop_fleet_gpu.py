"""Closed loops for fleets: per-instance plants (LMPC.simulate(plants=...)) and loops of a bank (LMPCHetero.simulate / make_loop / run_loop,
mpcx_lmpc_hetero_loop_create).

The yardsticks are those of tests/test_lmpc_loop_gpu.py, whose controllers and helpers are used as they are: every tick against the single-step
call on the loop's logged state and last input, bit for bit; the plant step against float64 numpy within the dot-product bound
(nx + nu + ndu + 2) 2^-52 (|A_b||x| + |B_b||u| + |Bd_b||d| + |w|); tick 0 of a bank against one oracle controller per instance.  The
per-instance advance kernel sums each row in the uniform kernel's order, so on equal plants the two loops agree bit for bit.

Shapes: quadrotor (nx = 12: 5 instances and 4 idle lanes per wavefront, ndu = 4 with Bd = 0), axes_blocked (nx = 4: 16 instances, no idle lane,
ndu = 0), random (nx = 3: 21 instances, 1 idle lane, ndu = 1); B = 1, 22 and 100 are a single partial tile, a tile boundary crossed by one
instance (random) and several tiles with a partial last one."""
import functools

import numpy as np
import pytest

from helpers import OracleFrontEnd, configure_random, random_lmpc_spec
from test_lmpc_loop_gpu import CONTROLLERS, EQUAL, _follow, _np

pytestmark = pytest.mark.gpu

FIELDS = ("x", "u") + EQUAL


def _copies(m, B):
    return np.broadcast_to(m, (B,) + m.shape).copy()


def _scaled(m, B, rng):
    """(1 + 0.05 xi_b) m, one xi per instance"""
    return (1.0 + 0.05 * rng.normal(size=(B, 1, 1))) * m[None]


def _assert_plants(res, A, Bm, Bd, d_of_tick, noise, label, factor=1.0, x_next=None):
    """traj_x[k+1] (or x_next(k)) against float64 numpy A_b x + B_b u + Bd_b d + w with a plant per instance ([B, nx, .] arrays),
    componentwise within `factor` times the dot-product bound"""
    x, u = _np(res.x), _np(res.u)
    nterms = A.shape[2] + Bm.shape[2] + Bd.shape[2]
    for k in range(u.shape[0]):
        d = np.broadcast_to(d_of_tick(k), (x.shape[1], Bd.shape[2]))
        w = noise[k] if noise is not None else np.zeros_like(x[k])
        want = np.einsum("bij,bj->bi", A, x[k]) + np.einsum("bij,bj->bi", Bm, u[k]) + np.einsum("bij,bj->bi", Bd, d) + w
        mag = np.einsum("bij,bj->bi", np.abs(A), np.abs(x[k])) + np.einsum("bij,bj->bi", np.abs(Bm), np.abs(u[k])) + \
            np.einsum("bij,bj->bi", np.abs(Bd), np.abs(d)) + np.abs(w)
        bound = factor * (nterms + 2) * 2.0 ** -52 * mag
        got = x[k + 1] if x_next is None else x_next(k)
        err = np.abs(got - want)
        print("%s tick %d: plant error max %.3e, worst ratio to the bound %.3f" % (label, k, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, k, float(err.max()))


# ---------------------------------------------------------------------------------------------
# banks: name -> (bank, per-controller (A, B, Bd, d0) arrays [K, ...], model index or None, inputs(B) -> x0, u0, references)
# ---------------------------------------------------------------------------------------------
class _ModelRecorder:
    """stands in for a controller given to quadrotor_variant(into=...): keeps the model, accepts every other setter"""
    def setStateSpaceModel(self, A, B, C):
        self.A, self.B = np.array(A, dtype=np.float64), np.array(B, dtype=np.float64)
        return True

    def __getattr__(self, name):
        return lambda *a, **k: True


def _random_inputs(B):
    r = np.random.default_rng(B)
    return r.uniform(-0.5, 0.5, size=(B, 3)), r.uniform(-0.4, 0.4, size=(B, 2)), {}


@functools.lru_cache(maxsize=None)
def _bank(name):
    from libmpc_amd import LMPC, LMPCHetero
    if name.startswith("random"):
        K = 22 if name == "random22" else 7
        specs = [random_lmpc_spec(100 + k) for k in range(K)]
        het = LMPCHetero([configure_random(LMPC(*sp["dims"], device=-1), sp) for sp in specs], device=0)
        mats = tuple(np.stack([sp[n] for sp in specs]) for n in ("A", "B", "Bd")) + (np.stack([sp["dmeas"][:, 0] for sp in specs]),)
        model = {"random22": None, "random7": (7 * np.arange(100)) % 7, "random7_mixed": (3 * np.arange(100)) % 7}[name]
        return het, mats, model, _random_inputs
    from libmpc_amd.workloads import quadrotor_batch, quadrotor_variant
    K, ph = 8, 10
    het = LMPCHetero([quadrotor_variant(k, ph, device=-1) for k in range(K)], device=0)
    recs = [quadrotor_variant(k, ph, into=_ModelRecorder()) for k in range(K)]
    mats = (np.stack([r.A for r in recs]), np.stack([r.B for r in recs]), np.zeros((K, 12, 4)), np.zeros((K, 4)))

    def inputs(B):
        x0, u0, yref = quadrotor_batch(B)
        return x0, u0, dict(yref=yref)
    return het, mats, (7 * np.arange(100)) % K, inputs


BANKS = ["random22", "random7", "random7_mixed", "quadrotor8"]


def _bank_case(name):
    het, mats, model, inputs = _bank(name)
    B = het.count if model is None else len(model)
    idx = np.arange(B) if model is None else model
    x0, u0, refs = inputs(B)
    if model is not None:
        refs = dict(refs, model=model)
    return het, tuple(m[idx] for m in mats), B, x0, u0, refs


# ---------------------------------------------------------------------------------------------
# 1. identical plants: the per-instance kernel against the uniform one, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True], ids=["quiet", "noise"])
@pytest.mark.parametrize("B", [1, 22, 100])
@pytest.mark.parametrize("name", sorted(CONTROLLERS))
def test_identical_plants_equal_the_uniform_loop_bit_for_bit(name, B, noisy):
    import torch
    make, inputs, (A, Bm, Bd, _) = CONTROLLERS[name]()
    ticks = 5
    x0, u0, refs = inputs(B)
    noise = 0.05 * np.random.default_rng(5).normal(size=(ticks, B, A.shape[0])) if noisy else None
    c = make()
    uniform = c.simulate(x0, u0, ticks, noise=noise, **refs)
    # every entry given, or (B = 22) the controller's own completing the triple
    plants = (_copies(A, B), None, None) if B == 22 else (_copies(A, B), _copies(Bm, B), _copies(Bd, B))
    fleet = c.simulate(x0, u0, ticks, noise=noise, plants=plants, **refs)
    for f in FIELDS:
        a, b = getattr(fleet, f), getattr(uniform, f)
        assert torch.equal(a, b), (name, B, f, int((a != b).sum()))
    assert int((uniform.status == 0).sum()) > 0


# ---------------------------------------------------------------------------------------------
# 2. a plant per instance
# ---------------------------------------------------------------------------------------------
def _wide(nx):
    """(nx, 2, 2, 3) with ph = 3, ch = 2: nx = 32, two instances fill the wavefront's 64 lanes exactly; nx = 64, every lane a state row"""
    from libmpc_amd import LMPC
    sp = random_lmpc_spec(3, nx=nx, nu=2, ndu=2, ny=3, ph=3, ch=2)

    def inputs(B):
        r = np.random.default_rng(B)
        return (3.0 / nx) ** 0.5 * r.uniform(-0.5, 0.5, size=(B, nx)), r.uniform(-0.4, 0.4, size=(B, 2)), {}
    return (lambda: configure_random(LMPC(*sp["dims"], device=0), sp)), inputs, (sp["A"], sp["B"], sp["Bd"], sp["dmeas"][:, 0])


# the shapes of the uniform loop's tests at B = 100, and the two at the edge of the lane <-> (instance, row) mapping: two full tiles and a half, three tiles
PLANT_CASES = [(name, 100) for name in sorted(CONTROLLERS)] + [("n32", 5), ("n64", 3)]
PLANT_SHAPES = dict(CONTROLLERS, n32=lambda: _wide(32), n64=lambda: _wide(64))


@pytest.mark.parametrize("name,B", PLANT_CASES, ids=sorted(CONTROLLERS) + ["n32-B5", "n64-B3"])
def test_different_plants_per_instance(name, B):
    import torch
    from libmpc_amd import LMPC
    make, inputs, (A, Bm, Bd, d0) = PLANT_SHAPES[name]()
    ticks = 5
    x0, u0, refs = inputs(B)
    rng = np.random.default_rng(12)
    P1 = tuple(_scaled(m, B, rng) for m in (A, Bm, Bd))
    c = make()
    loop = c.make_loop(x0, u0, ticks, plants=P1, warm=False, **refs)
    try:
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        _assert_plants(res, *P1, lambda k: d0, None, name + " plants")
        _follow(make(), res, u0, ticks, name + " plants", **refs)          # the controller does not notice the plant
        first = res.x.clone()
        # refilled in place: the next run uses the new plants
        P2 = tuple(_scaled(m, B, rng) for m in (A, Bm, Bd))
        loop.plants.copy_(LMPC.pack_plants(*(torch.as_tensor(m).cuda() for m in P2)))
        res = c.run_loop(loop)
        torch.cuda.synchronize()
        _assert_plants(res, *P2, lambda k: d0, None, name + " refilled plants")
        assert not torch.equal(res.x, first)
    finally:
        c.destroy_loop(loop)


# ---------------------------------------------------------------------------------------------
# 3. bank loops against the bank's single-step call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ticks", [1, 7])
@pytest.mark.parametrize("name", BANKS)
def test_cold_bank_ticks_equal_the_single_step_bank_call(name, ticks):
    het, _, B, x0, u0, refs = _bank_case(name)
    res = het.simulate(x0, u0, ticks, warm=False, **refs)
    assert tuple(res.x.shape) == (ticks + 1, B, het.nx) and tuple(res.u.shape) == (ticks, B, het.nu)
    assert np.array_equal(_np(res.x[0]), x0)
    _follow(het, res, u0, ticks, "%s cold ticks=%d" % (name, ticks), **refs)


@pytest.mark.parametrize("ticks", [1, 7])
@pytest.mark.parametrize("name", BANKS)
def test_warm_bank_ticks_equal_the_chained_single_step_bank_calls(name, ticks):
    het, _, B, x0, u0, refs = _bank_case(name)
    res = het.simulate(x0, u0, ticks, warm=True, **refs)
    _follow(het, res, u0, ticks, "%s warm ticks=%d" % (name, ticks), warm=True, **refs)
    if name == "quadrotor8" and ticks > 1:
        cold = het.simulate(x0, u0, ticks, warm=False, **refs)
        warm_rounds = float(res.polish_rounds[1:].double().mean()); cold_rounds = float(cold.polish_rounds[1:].double().mean())
        print("%s: polish rounds per solve over ticks >= 1: warm %.3f, cold %.3f" % (name, warm_rounds, cold_rounds))
        assert warm_rounds < cold_rounds


# ---------------------------------------------------------------------------------------------
# 4. the plants of a bank
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BANKS)
def test_a_bank_without_a_plant_steps_each_instance_with_its_own_controllers_model(name):
    """... and, references being each controller's own, with step 0 of its own exogenous input"""
    import torch
    het, (A, Bm, Bd, d0), B, x0, u0, refs = _bank_case(name)
    ticks = 5
    res = het.simulate(x0, u0, ticks, **refs)
    _assert_plants(res, A, Bm, Bd, lambda k: d0, None, name + " own plants")
    # nominal consistency: the next state is the first predicted one of that tick's single-step call
    seq, u = [], torch.as_tensor(u0).cuda()
    for k in range(ticks):
        r = het.optimizeBatch(res.x[k], u, want_sequence=True, **refs)
        torch.cuda.synchronize()
        assert torch.equal(r.cmd, res.u[k])
        seq.append(_np(r.seq_state)[:, 1, :])
        u = res.u[k]
    _assert_plants(res, A, Bm, Bd, lambda k: d0, None, name + " nominal", factor=2.0, x_next=lambda k: seq[k])


def test_a_bank_with_a_plant_per_instance_and_with_one_plant_for_all():
    het, (A, Bm, Bd, d0), B, x0, u0, refs = _bank_case("random7_mixed")
    ticks = 5
    rng = np.random.default_rng(13)
    noise = 0.02 * rng.normal(size=(ticks, B, het.nx))
    # plants=: every matrix given / the controllers' own B and Bd completing the triple
    P = tuple(_scaled(m[0], B, rng) for m in (A, Bm, Bd))
    res = het.simulate(x0, u0, ticks, plants=P, noise=noise, **refs)
    _assert_plants(res, *P, lambda k: d0, noise, "bank plants=")
    _follow(het, res, u0, ticks, "bank plants=", warm=True, **refs)
    res = het.simulate(x0, u0, ticks, plants=(P[0], None, None), **refs)
    _assert_plants(res, P[0], Bm, Bd, lambda k: d0, None, "bank plants=(A, None, None)")
    # plant=: one plant for all through the uniform kernel (d_k still each controller's own) / a partial one, completed per instance
    one = (1.03 * A[0], 0.97 * Bm[1], 1.1 * Bd[2])
    res = het.simulate(x0, u0, ticks, plant=one, noise=noise, **refs)
    _assert_plants(res, *(_copies(m, B) for m in one), lambda k: d0, noise, "bank plant=")
    _follow(het, res, u0, ticks, "bank plant=", warm=True, **refs)
    res = het.simulate(x0, u0, ticks, plant=(one[0], None), **refs)
    _assert_plants(res, _copies(one[0], B), Bm, Bd, lambda k: d0, None, "bank plant=(A, None)")
    with pytest.raises(ValueError):
        het.simulate(x0, u0, ticks, plant=one, plants=P, **refs)


# ---------------------------------------------------------------------------------------------
# 5. oracle anchor: tick 0 of a bank loop, one oracle controller per instance
# ---------------------------------------------------------------------------------------------
def test_tick_zero_of_a_bank_loop_matches_one_oracle_controller_per_instance():
    """the controllers and inputs of test_lmpc_hetero.py::test_every_instance_its_own_random_controller_matches_the_oracle, and its tolerances"""
    from libmpc_amd import LMPC, LMPCHetero, LParameters
    K = 48
    specs = [random_lmpc_spec(100 + k) for k in range(K)]
    ctrls, oracles = [], []
    for sp in specs:
        c = configure_random(LMPC(*sp["dims"], device=-1), sp)
        c.setOptimizerParameters(LParameters(maximum_iteration=2000))
        ctrls.append(c)
        o = configure_random(OracleFrontEnd(*sp["dims"]), sp)
        o.setOptimizerParameters(maximum_iteration=2000)
        oracles.append(o)
    het = LMPCHetero(ctrls, device=0)
    rng = np.random.default_rng(7)
    nx, nu = specs[0]["dims"][0], specs[0]["dims"][1]
    x0 = rng.uniform(-1, 1, size=(K, nx)); x0[:, 0] *= 0.5
    u0 = rng.uniform(-0.5, 0.5, size=(K, nu))
    res = het.simulate(x0, u0, 1, warm=False)
    cmd, cost, st = _np(res.u[0]), _np(res.cost[0]), _np(res.status[0])
    checked = 0
    for k in range(K):
        ref = oracles[k].optimize(x0[k], u0[k])
        if ref["polished"] != 1:
            continue
        checked += 1
        assert st[k] == 0
        assert np.abs(cmd[k] - ref["cmd"]).max() <= 1e-5 * max(np.abs(ref["cmd"]).max(), 1e-12), (k, cmd[k], ref["cmd"])
        assert abs(cost[k] - ref["cost"]) <= 1e-6 * max(1.0, abs(ref["cost"]))
    assert checked >= K * 3 // 4, checked


# ---------------------------------------------------------------------------------------------
# 6. preview references on a bank
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_preview_windows_on_a_bank_are_the_per_step_references_of_each_tick(warm):
    het, (A, Bm, Bd, _), B, x0, u0, refs = _bank_case("random7_mixed")
    ticks = 5
    r = np.random.default_rng(21)
    yref = r.normal(size=(B, ticks + het.ph, het.ny)); dmeas = 0.2 * r.normal(size=(B, ticks + het.ph, het.ndu))
    res = het.simulate(x0, u0, ticks, yref=yref, dmeas=dmeas, preview=True, warm=warm, **refs)
    _follow(het, res, u0, ticks, "bank preview", warm=warm,
            refs_of_tick=lambda k: dict(yref=np.ascontiguousarray(yref[:, k:k + het.ph]), dmeas=np.ascontiguousarray(dmeas[:, k:k + het.ph])), **refs)
    _assert_plants(res, A, Bm, Bd, lambda k: dmeas[:, k, :], None, "bank preview")
    with pytest.raises(ValueError):
        het.simulate(x0, u0, ticks, yref=yref[:, :-1], preview=True, **refs)


# ---------------------------------------------------------------------------------------------
# 7. re-run and lifetime
# ---------------------------------------------------------------------------------------------
def test_bank_loop_rerun_replay_past_the_end_and_the_bank_afterwards():
    import ctypes as C
    import torch
    from libmpc_amd import _capi
    het, _, B, x0, u0, refs = _bank_case("quadrotor8")
    ticks = 4
    before = het.optimizeBatch(x0, u0, want_active=True, **refs)
    torch.cuda.synchronize()
    names = ("cmd",) + EQUAL + ("active_lower", "active_upper")
    before = {k: getattr(before, k).clone() for k in names}

    loop = het.make_loop(x0, u0, ticks, **refs)
    runs = []
    for _ in range(2):
        res = het.run_loop(loop)
        torch.cuda.synchronize()
        runs.append({k: getattr(res, k).clone() for k in FIELDS})
    for k in FIELDS:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert int((runs[0]["status"] == 0).sum()) > 0

    # one replay more than `ticks`: the counter stands at `ticks` and nothing is written
    lib = _capi.lib()
    tick = C.c_int(-1)
    _capi.check(lib.mpcx_lmpc_loop_debug_tick(loop.handle, C.byref(tick)))
    assert tick.value == ticks
    _capi.check(lib.mpcx_lmpc_loop_debug_replay(loop.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    _capi.check(lib.mpcx_lmpc_loop_debug_tick(loop.handle, C.byref(tick)))
    assert tick.value == ticks
    for k in FIELDS:
        assert torch.equal(getattr(loop.result, k), runs[0][k]), k

    het.destroy_loop(loop)
    het.destroy_loop(loop)          # idempotent

    # a plain solve of the bank after a loop gives what it gave before
    after = het.optimizeBatch(x0, u0, want_active=True, **refs)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(after, k), v), k
