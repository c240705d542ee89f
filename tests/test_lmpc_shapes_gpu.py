"""LMPC parity beyond the quadrotor: controllers whose optimal working sets run past the lean kernels' 16 rows and past the fallback
polish's register (16) and LDS (28) capacities, every template variant of the solve kernels, odd shapes, warm starts and a
heterogeneous bank -- each against the CPU oracle at the tolerances of BASELINE.json (u* 1e-5, cost 1e-7, active sets bit for bit
wherever the oracle polished), with status, solver_status and active_count equal to the oracle's there.  The workloads reaching these
edges is pinned by test_lmpc_shapes.py."""
import numpy as np
import pytest

from helpers import SHAPES_EDGES, SHAPES_MAIN, SHAPES_MAXIT, SHAPES_VARIANTS
from helpers import assert_matches_oracle, axes_batch, axes_spec, configure_axes, oracle_batch_parallel_spec

pytestmark = pytest.mark.gpu

# (name, debug_force_generic, debug_use_fused)
PATHS = [("default", False, None), ("two-kernel", False, 0), ("generic", True, None), ("fused", False, 1), ("group", False, 2)]


def _controller(spec, generic=False, fused=None, warm=False):
    from libmpc_amd import LMPC, LParameters
    c = configure_axes(LMPC(*spec["dims"], device=0), spec, SHAPES_MAXIT)
    if warm:
        c.setOptimizerParameters(LParameters(maximum_iteration=SHAPES_MAXIT, enable_warm_start=1))
    c.debug_force_generic(generic)
    c.debug_use_fused(fused)
    return c


def _solve(c, x0, u0, yref=None, **kw):
    import torch
    r = c.optimizeBatch(x0, u0, yref=yref, want_active=True, **kw)
    torch.cuda.synchronize()
    return r


def _move_blocked_rows(rows, spec, neq):
    """rows compared under move blocking: test_full_feature_controller_parity leaves out the input rows past the control horizon and
    the delta-u rows; here the state and output rows past it go too.  There the input is held, so each state's rows span two
    directions only: three or more of them at their bound are linearly dependent and their multipliers are not unique."""
    nx, nu, ndu, ny, ph, ch = spec["dims"]
    na = nx + nu
    y0 = 2 * neq
    du0 = y0 + (ph + 1) * ny
    return [x for x in rows if not (neq <= x < y0 and (x - neq) // na > ch) and not (y0 <= x < du0 and (x - y0) // ny > ch)
            and not (du0 <= x < du0 + ph * nu)]


def _check(r, ref, spec, label=""):
    """assert_matches_oracle plus status, solver_status and active_count; returns the GPU's active_count"""
    nx, nu, ndu, ny, ph, ch = spec["dims"]
    blocked = ch < ph
    pol = ref["polished"] == 1
    assert pol.mean() >= 0.9, (label, pol.mean())
    assert (ref["polished_raw"] == 1).sum() - pol.sum() <= max(2, len(pol) // 50), label     # oracle points outside the bounds: rare
    # Two kinds of command have no relative error to speak of, and are compared here instead, absolutely: one that is zero up to
    # round-off (closed loop: a velocity held on its bound), and the oracle's ADMM iterate where its polish failed, which is off by ADMM
    # accuracy also where the command is near zero (5e-2, as assert_matches_oracle, but of max(1, |u|)).  assert_matches_oracle checks
    # everything else of those instances.
    cmd = r.cmd.cpu().numpy()
    scale = np.abs(ref["cmd"]).max(axis=1)
    zero = scale < 1e-10
    assert (np.abs(cmd[zero] - ref["cmd"][zero]).max(axis=1, initial=0.0) <= 1e-12).all(), label
    loose = (ref["polished"] != 1) & ~zero
    assert (np.abs(cmd[loose] - ref["cmd"][loose]).max(axis=1, initial=0.0) <= 5e-2 * np.maximum(1.0, scale[loose])).all(), label
    ref = dict(ref, cmd=np.where((zero | loose)[:, None], cmd, ref["cmd"]))
    try:
        assert_matches_oracle(r, ref, ref["neq"], ref["ncon"], check_active=not blocked)
    except AssertionError as e:
        raise AssertionError((label,) + e.args) from e
    st = r.status.cpu().numpy(); sst = r.solver_status.cpu().numpy(); ac = r.active_count.cpu().numpy()
    assert np.array_equal(st, ref["status"]), (label, np.nonzero(st != ref["status"])[0][:8])
    bad = np.nonzero(pol & (sst != ref["solver_status"]))[0]
    assert bad.size == 0, (label, bad[:8], sst[bad[:8]], ref["solver_status"][bad[:8]])
    if blocked:
        from helpers import bits_to_rows
        m, neq = ref["ncon"], ref["neq"]
        lo = bits_to_rows(r.active_lower.cpu().numpy(), m); up = bits_to_rows(r.active_upper.cpu().numpy(), m)
        for b in np.nonzero(pol)[0]:
            rl = np.nonzero(ref["active_lower"][b][neq:])[0] + neq
            ru = np.nonzero(ref["active_upper"][b][neq:])[0] + neq
            assert _move_blocked_rows(lo[b], spec, neq) == _move_blocked_rows(rl, spec, neq), (label, b)
            assert _move_blocked_rows(up[b], spec, neq) == _move_blocked_rows(ru, spec, neq), (label, b)
    else:
        # the working set holds every row with a nonzero multiplier; beyond those it may hold rows at their bound with a zero multiplier
        # (a degenerate optimum -- the zero-weight controller has a few), so the count is exact up to those on all but 1 % of instances
        short = np.nonzero(pol & (ac < ref["n_active"]))[0]
        assert short.size == 0, (label, short[:8], ac[short[:8]], ref["n_active"][short[:8]])
        more = np.nonzero(pol & (ac > ref["n_flagged"]))[0]
        assert more.size <= pol.sum() // 100, (label, more[:8], ac[more[:8]], ref["n_flagged"][more[:8]])
    return ac


def _buckets(ac):
    return int((ac <= 16).sum()), int(((ac > 16) & (ac <= 28)).sum()), int((ac > 28).sum())


# ---------------------------------------------------------------------------------------------
# 1. large working sets on every path
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_case():
    sp = axes_spec(*SHAPES_MAIN[:2])
    x0, u0, _ = axes_batch(sp, SHAPES_MAIN[2] + 7)
    r = np.random.default_rng(77)
    yref = np.zeros((len(x0), sp["dims"][3])); yref[:, 0:2 * sp["nax"]:2] = r.uniform(-0.5, 0.5, size=(len(x0), sp["nax"]))
    ref = oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=SHAPES_MAXIT)
    ref_y = oracle_batch_parallel_spec(sp, x0[:SHAPES_MAIN[2]], u0[:SHAPES_MAIN[2]], yref[:SHAPES_MAIN[2]], maximum_iteration=SHAPES_MAXIT)
    return sp, x0, u0, yref, ref, ref_y


def _head(ref, n):
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


@pytest.mark.parametrize("path", PATHS + [("per-instance-yref", False, None)], ids=lambda p: p[0])
def test_large_working_sets_every_path(main_case, path):
    sp, x0, u0, yref, ref, ref_y = main_case
    name, generic, fused = path
    B = SHAPES_MAIN[2]
    c = _controller(sp, generic, fused)
    if name == "fused":
        assert int(c.debug_get("flags")[2]) == 1           # the fused / persistent form takes this controller
    if name in ("default", "group"):
        assert int(c.debug_get("flags")[1]) == 1           # ... and so does the in-workgroup form
    if name == "per-instance-yref":
        r = _solve(c, x0[:B], u0[:B], yref[:B])
        ac = _check(r, ref_y, sp, name)
    else:
        r = _solve(c, x0[:B], u0[:B])
        ac = _check(r, _head(ref, B), sp, name)
    small, mid, big = _buckets(ac)
    assert mid > 0 and big > 0, (small, mid, big)          # both fallback branches ran: LDS Cholesky (17..28) and beyond
    print("%s: active_count buckets <=16 %d, 17..28 %d, >28 %d; iterations max %d" % (name, small, mid, big, int(r.iterations.max())))


@pytest.mark.parametrize("B", [1, 15, 17, SHAPES_MAIN[2] + 7])
def test_large_working_sets_ragged_batches(main_case, B):
    """partial last workgroups / chunks, with instances of every bucket in them"""
    sp, x0, u0, yref, ref, ref_y = main_case
    for name, generic, fused in PATHS:
        r = _solve(_controller(sp, generic, fused), x0[:B], u0[:B])
        _check(r, _head(ref, B), sp, "%s B=%d" % (name, B))


# ---------------------------------------------------------------------------------------------
# 2. every kernel template variant
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES_VARIANTS))
def test_every_kernel_variant(name):
    kw, variant, cost_direct = SHAPES_VARIANTS[name]
    sp = axes_spec(**kw)
    x0, u0, _ = axes_batch(sp, 512, seed=11)
    ref = oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=SHAPES_MAXIT)
    paths = [("default", False, None), ("two-kernel", False, 0)] + ([("group", False, 2)] if variant == 2 else [])
    for pname, generic, fused in paths:
        c = _controller(sp, generic, fused)
        assert c.info()["kernel_variant"] == variant
        assert int(c.debug_get("flags")[0]) == cost_direct
        if pname == "group":
            assert int(c.debug_get("flags")[1]) == 1
        r = _solve(c, x0, u0)
        ac = _check(r, ref, sp, "%s %s" % (name, pname))
        print("%s %s: buckets %s" % (name, pname, _buckets(ac)))


# ---------------------------------------------------------------------------------------------
# 3. shape edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES_EDGES))
def test_shape_edges_every_path(name):
    sp = axes_spec(**SHAPES_EDGES[name])
    x0, u0, _ = axes_batch(sp, 64, seed=5)
    ref = oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=SHAPES_MAXIT)
    for pname, generic, fused in PATHS:
        r = _solve(_controller(sp, generic, fused), x0, u0)
        _check(r, ref, sp, "%s %s" % (name, pname))


# ---------------------------------------------------------------------------------------------
# 4. warm start with large working sets
# ---------------------------------------------------------------------------------------------
def test_warm_start_closed_loop_with_large_working_sets():
    """30 closed-loop steps of 256 instances, each step seeded with the previous step's active sets (shifted one step): every step
    against a cold oracle solve"""
    sp = axes_spec(*SHAPES_MAIN[:2])
    x, u, _ = axes_batch(sp, 256, seed=99)
    c = _controller(sp, warm=True)
    prev = None
    seen = np.zeros(3, dtype=int)
    for k in range(30):
        ref = oracle_batch_parallel_spec(sp, x, u, maximum_iteration=SHAPES_MAXIT)
        r = _solve(c, x, u, warm=prev, warm_shift=prev is not None)
        ac = _check(r, ref, sp, "step %d" % k)
        seen += np.array(_buckets(ac))
        cmd = r.cmd.cpu().numpy()
        x = x @ sp["A"].T + cmd @ sp["B"].T
        # lastU = the command, kept 0.1 % inside the input box: a lastU exactly on its bound is a step-0 row at its bound, and there
        # the reference's polish fails on almost every instance (the oracle is then only ADMM-accurate, 1e-5 cannot be asked of it)
        u = np.clip(cmd, 0.999 * sp["umin"], 0.999 * sp["umax"])
        prev = r
    assert seen[1] > 0 and seen[2] > 0, seen


# ---------------------------------------------------------------------------------------------
# 5. heterogeneous bank
# ---------------------------------------------------------------------------------------------
def test_heterogeneous_bank_of_perturbed_controllers():
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from libmpc_amd import LMPC
    from libmpc_amd.bank import LMPCHetero
    K, B = 64, 256
    specs = [axes_spec(3, 20, perturb=0.2, seed=1000 + k) for k in range(K)]
    het = LMPCHetero([configure_axes(LMPC(*s["dims"], device=-1), s, SHAPES_MAXIT) for s in specs], device=0)
    x0, u0, yref = axes_batch(specs[0], B, seed=3)
    model = np.arange(B) % K
    r = het.optimizeBatch(x0, u0, model=model, want_active=True); torch.cuda.synchronize()

    def one(k):
        idx = np.nonzero(model == k)[0]
        return idx, oracle_batch_parallel_spec(specs[k], x0[idx], u0[idx], maximum_iteration=SHAPES_MAXIT, workers=1)
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(one, range(K)))
    ref = {"neq": parts[0][1]["neq"], "ncon": parts[0][1]["ncon"]}
    for key, first in parts[0][1].items():
        if isinstance(first, np.ndarray):
            ref[key] = np.zeros((B,) + first.shape[1:], dtype=first.dtype)
            for idx, p in parts:
                ref[key][idx] = p[key]
    ac = _check(r, ref, specs[0], "bank")
    assert _buckets(ac)[1] > 0 and _buckets(ac)[2] > 0


# ---------------------------------------------------------------------------------------------
# 6. refusal
# ---------------------------------------------------------------------------------------------
def test_too_large_a_controller_is_refused_and_the_process_goes_on():
    from libmpc_amd._capi import E_UNSUPPORTED, MpcxError
    big = axes_spec(11, 50)
    x0, u0, _ = axes_batch(big, 4)
    with pytest.raises(MpcxError) as e:
        _solve(_controller(big), x0, u0)
    assert e.value.code == E_UNSUPPORTED
    sp = axes_spec(**SHAPES_EDGES["nu3"])
    x0, u0, _ = axes_batch(sp, 32, seed=8)
    ref = oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=SHAPES_MAXIT)
    _check(_solve(_controller(sp), x0, u0), ref, sp, "after refusal")
