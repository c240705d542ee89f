"""The hand-over from the polish-first solve kernels to the fallback kernel: a device-resident failure queue per handle.  The solve kernels
list the instances they leave open, the fallback kernel serves the list and restores the empty queue; a step that leaves nothing open costs the
fallback one load of the count.  `debug_get("fallback")` = [instances served by the last step that left any (reading clears it), entries the queue
holds, wavefronts of the fallback kernel's grid].

`loaded`: the three-axis controller of test_lmpc_shapes_gpu.py on its own batch (working sets of 0 to ~60 rows: about half the instances leave
the lean kernels); `clean`: the same controller with x0 and u0 scaled down until none does.  Oracle: oracle_batch_parallel_spec, 96 instances."""
import numpy as np
import pytest

from helpers import SHAPES_MAIN, SHAPES_MAXIT
from helpers import assert_matches_oracle, axes_batch, axes_spec, configure_axes, oracle_batch_parallel_spec
from test_lmpc_shapes_gpu import PATHS, _check, _controller, _head, _solve

pytestmark = pytest.mark.gpu

NREF = 96
HANDOVER_PATHS = [p for p in PATHS if p[0] in ("group", "two-kernel", "fused")]
ARRAYS = ("cmd", "cost", "status", "solver_status", "is_feasible", "iterations", "polish_rounds", "active_count", "active_lower", "active_upper")


def _arrays(r):
    return {k: getattr(r, k).cpu().numpy().copy() for k in ARRAYS}


def _assert_same(a, b, label=""):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (label, k, np.nonzero((a[k] != b[k]).reshape(len(a[k]), -1).any(axis=1))[0][:8])


def _fallback(c):
    """(served_last, capacity, W); the read clears served_last"""
    served, cap, w = c.debug_get("fallback")
    return int(served), int(cap), int(w)


@pytest.fixture(scope="module")
def case():
    sp = axes_spec(*SHAPES_MAIN[:2])
    x0, u0, _ = axes_batch(sp, SHAPES_MAIN[2] + 7)           # the batch of test_lmpc_shapes_gpu.py's main case
    ref = oracle_batch_parallel_spec(sp, x0[:NREF], u0[:NREF], maximum_iteration=SHAPES_MAXIT)
    return sp, x0, u0, ref


CLEAN = 0.02      # scale of x0, u0 of the `clean` batch: every optimum well inside the velocity and input boxes


@pytest.mark.parametrize("path", HANDOVER_PATHS, ids=lambda p: p[0])
@pytest.mark.parametrize("B", [1, 16, 17, NREF])
def test_parity_at_the_edges_of_the_hand_over(case, path, B):
    sp, x0, u0, ref = case
    name, generic, fused = path
    c = _controller(sp, generic, fused)
    r = _solve(c, x0[:B], u0[:B])
    ac = _check(r, _head(ref, B), sp, "%s B=%d" % (name, B))
    served, cap, w = _fallback(c)
    print("%s B=%d: served %d, more than 16 rows %d, capacity %d, W %d" % (name, B, served, int((ac > 16).sum()), cap, w))
    assert served >= int((ac > 16).sum())
    assert served <= B
    assert cap >= B


@pytest.mark.parametrize("path", HANDOVER_PATHS, ids=lambda p: p[0])
def test_nothing_leaks_between_steps(case, path):
    sp, x0, u0, ref = case
    name, generic, fused = path
    B = 256
    c = _controller(sp, generic, fused)
    first = _arrays(_solve(c, x0[:B], u0[:B]))
    served1 = _fallback(c)[0]
    assert served1 > 0
    clean = _arrays(_solve(c, CLEAN * x0[:B], CLEAN * u0[:B]))
    assert _fallback(c)[0] == 0
    second = _arrays(_solve(c, x0[:B], u0[:B]))
    assert _fallback(c)[0] == served1
    _assert_same(first, second, "loaded twice")
    fresh = _controller(sp, generic, fused)
    _assert_same(clean, _arrays(_solve(fresh, CLEAN * x0[:B], CLEAN * u0[:B])), "clean against a fresh handle")
    assert _fallback(fresh)[0] == 0


def test_more_failures_than_consumer_wavefronts(case):
    sp, x0, u0, ref = case
    B = 4096
    xb, ub = np.tile(x0[:1024], (4, 1)), np.tile(u0[:1024], (4, 1))      # (instances are independent: the first 96 rows are the oracle's)
    c = _controller(sp)
    whole = _solve(c, xb, ub)
    served, cap, w = _fallback(c)
    print("served %d of %d with %d wavefronts" % (served, B, w))
    assert served > w                                                    # a wavefront served more than one entry of the list
    whole = _arrays(whole)
    parts = [_arrays(_solve(c, xb[i:i + 64], ub[i:i + 64])) for i in range(0, B, 64)]
    sliced = {k: np.concatenate([p[k] for p in parts]) for k in ARRAYS}
    _assert_same(whole, sliced, "one call against slices of 64")
    head = _solve(c, xb[:NREF], ub[:NREF])
    _assert_same({k: v[:NREF] for k, v in whole.items()}, _arrays(head), "first rows")
    _check(head, ref, sp, "first %d rows" % NREF)


def test_a_producer_without_its_consumer_leaves_no_entries_behind(case):
    import ctypes as C
    import torch
    sp, x0, u0, ref = case
    B = 256
    for name, generic, fused in HANDOVER_PATHS:
        c = _controller(sp, generic, fused)
        before = _arrays(_solve(c, x0[:B], u0[:B]))
        served = _fallback(c)[0]
        b, res, keep = c.make_batch(x0[:B], u0[:B], want_active=True)
        s = torch.cuda.current_stream(0)
        assert c.time_launches(b, 3, s) > 0
        ms3 = (C.c_float * 3)()
        assert c._lib.mpcx_lmpc_debug_time_kernels(c._h, C.byref(b), C.c_void_p(s.cuda_stream), 3, ms3) == 0
        torch.cuda.synchronize()
        _fallback(c)
        after = _arrays(_solve(c, x0[:B], u0[:B]))
        _assert_same(before, after, name)
        assert _fallback(c)[0] == served, name


def test_graph_replays_of_a_loaded_step(case):
    import torch
    sp, x0, u0, ref = case
    B = 256
    c = _controller(sp)
    eager = _arrays(_solve(c, x0[:B], u0[:B]))
    assert _fallback(c)[0] > 0
    b, res, keep = c.make_batch(x0[:B], u0[:B], want_active=True)
    side = torch.cuda.Stream(device=0)
    g = c.make_graph(b, side)
    side.synchronize()
    for k in range(3):
        res.cmd.fill_(float("nan")); res.cost.fill_(float("nan")); res.status.fill_(-77); res.active_count.fill_(-77)
        torch.cuda.synchronize()
        c.launch_graph(g, side)
        side.synchronize()
        _assert_same(eager, _arrays(res), "replay %d" % k)
    c.destroy_graph(g)


def test_heterogeneous_bank_has_a_queue_of_its_own():
    import torch
    from libmpc_amd import LMPC
    from libmpc_amd.bank import LMPCHetero
    K, B = 8, 17
    specs = [axes_spec(3, 20, perturb=0.2, seed=1000 + k) for k in range(K)]
    het = LMPCHetero([configure_axes(LMPC(*s["dims"], device=-1), s, SHAPES_MAXIT) for s in specs], device=0)
    x0, u0, _ = axes_batch(specs[0], B, seed=3)
    model = np.arange(B) % K
    r1 = het.optimizeBatch(x0, u0, model=model, want_active=True); torch.cuda.synchronize()
    served1 = int(het.debug_get(0, "fallback")[0])
    a1 = _arrays(r1)
    r2 = het.optimizeBatch(x0, u0, model=model, want_active=True); torch.cuda.synchronize()
    served2 = int(het.debug_get(0, "fallback")[0])
    _assert_same(a1, _arrays(r2), "bank, second solve")
    assert served1 == served2 and served1 >= int((a1["active_count"] > 16).sum()) and served1 <= B
    parts = [(np.nonzero(model == k)[0], None) for k in range(K)]
    parts = [(idx, oracle_batch_parallel_spec(specs[k], x0[idx], u0[idx], maximum_iteration=SHAPES_MAXIT, workers=1)) for k, (idx, _) in enumerate(parts)]
    ref = {"neq": parts[0][1]["neq"], "ncon": parts[0][1]["ncon"]}
    for key, first in parts[0][1].items():
        if isinstance(first, np.ndarray):
            ref[key] = np.zeros((B,) + first.shape[1:], dtype=first.dtype)
            for idx, p in parts:
                ref[key][idx] = p[key]
    assert_matches_oracle(r2, ref, ref["neq"], ref["ncon"])


GROW = (8, 40)      # a handle's scratch sized for 8 instances, then a batch of more than one group workgroup of 16 and no multiple of 16


@pytest.mark.parametrize("path", HANDOVER_PATHS, ids=lambda p: p[0])
def test_scratch_grows_between_two_calls(case, path):
    """workspace, queue and large-working-set slots are allocated anew for the larger batch: same bits as a handle that never had the small ones"""
    sp, x0, u0, ref = case
    name, generic, fused = path
    small, large = GROW
    c = _controller(sp, generic, fused)
    _solve(c, x0[:small], u0[:small])
    assert _fallback(c)[1] == small
    grown = _arrays(_solve(c, x0[:large], u0[:large]))
    assert _fallback(c)[1] == large
    fresh = _controller(sp, generic, fused)
    _assert_same(grown, _arrays(_solve(fresh, x0[:large], u0[:large])), "%s: grown against a fresh handle" % name)
    assert _fallback(fresh)[1] == large


def test_scratch_of_a_bank_grows_between_two_calls():
    import torch
    from libmpc_amd import LMPC
    from libmpc_amd.bank import LMPCHetero
    K = 8
    small, large = GROW
    specs = [axes_spec(3, 20, perturb=0.2, seed=1000 + k) for k in range(K)]
    x0, u0, _ = axes_batch(specs[0], large, seed=3)
    model = np.arange(large) % K

    def bank():
        return LMPCHetero([configure_axes(LMPC(*s["dims"], device=-1), s, SHAPES_MAXIT) for s in specs], device=0)

    def solve(het, n):
        r = het.optimizeBatch(x0[:n], u0[:n], model=model[:n], want_active=True); torch.cuda.synchronize()
        return _arrays(r)

    het = bank()
    solve(het, small)
    assert int(het.debug_get(0, "fallback")[1]) == small
    grown = solve(het, large)
    assert int(het.debug_get(0, "fallback")[1]) == large
    fresh = bank()
    _assert_same(grown, solve(fresh, large), "bank: grown against a fresh handle")
    assert int(fresh.debug_get(0, "fallback")[1]) == large


def test_the_headline_batch_leaves_the_fallback_nothing():
    from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc
    import torch
    c = quadrotor_lmpc(20, device=0)
    x0, u0, yref = quadrotor_batch(256)
    r = c.optimizeBatch(x0, u0, yref=yref); torch.cuda.synchronize()
    assert int((r.status.cpu().numpy() == 0).sum()) > 0
    assert _fallback(c)[0] == 0
