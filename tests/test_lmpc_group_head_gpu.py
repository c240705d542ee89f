"""The head of lmpc_solve_group (csrc/lmpc_fast.hip) -- staging, the two MFMA products, the cost constants and flags, the deal of the
instances over the wavefronts -- and the finish behind the rounds: the group form against the two-kernel form bit for bit on every result
array (they run the same rounds from the same record; which wavefront solves which instance changes nothing of an instance's arithmetic),
and against the CPU oracle at the suite's tolerances.  Shapes: full and ragged last workgroups (the deal is skipped there), both assemble
variants, the two-chunk kernel of eight wavefronts, and instances that start outside their state bounds (the fixed-row flags)."""
import numpy as np
import pytest

from helpers import assert_matches_oracle, quadrotor_oracle

pytestmark = pytest.mark.gpu

GROUP, TWO_KERNEL = 2, 0          # debug_use_fused
ARRAYS = ("cmd", "cost", "status", "solver_status", "is_feasible", "iterations", "polish_rounds", "active_count", "active_lower", "active_upper")


def _bitwise(a, b, label, arrays=ARRAYS):
    for k in arrays:
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        same = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert same, (label, k, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:8])


def _both_forms(ph, x0, u0, yref, strict=False):
    import torch
    from libmpc_amd.workloads import quadrotor_lmpc
    out = []
    for fused in (GROUP, TWO_KERNEL):
        c = quadrotor_lmpc(ph, device=0)
        c.debug_use_fused(fused)
        if strict:
            c.setStrictInfeasibility(True)
        if fused == GROUP:
            assert int(c.debug_get("flags")[1]) == 1           # the in-workgroup form takes this controller
        r = c.optimizeBatch(x0, u0, yref=yref, want_active=True)
        torch.cuda.synchronize()
        out.append(r)
    return out


def _head(ref, n):
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


def _case(ph, B):
    """inputs and the oracle's answers for both assemble variants: a reference per instance, and the controller's own for all"""
    from libmpc_amd.workloads import quadrotor_batch
    x0, u0, yref = quadrotor_batch(B)
    o = quadrotor_oracle(ph)
    shared = np.zeros((B, 12)); shared[:, 2] = 1.0              # what quadrotor_lmpc sets with setReferences
    refs = {"per-instance": o.solve_batch_constref(x0, u0, yref, want_active=True),
            "shared": o.solve_batch_constref(x0, u0, shared, want_active=True)}
    return x0, u0, yref, refs, o.neq, o.ncon


@pytest.fixture(scope="module")
def case20():
    return _case(20, 33)


@pytest.fixture(scope="module")
def case50():
    return _case(50, 17)


def _compare(ph, case, B, variant, arrays=ARRAYS):
    x0, u0, yref, refs, neq, ncon = case
    g, t = _both_forms(ph, x0[:B], u0[:B], yref[:B] if variant == "per-instance" else None)
    label = "N=%d B=%d %s" % (ph, B, variant)
    if "cost" in arrays:
        cg, ct = g.cost.cpu().numpy(), t.cost.cpu().numpy()
        print("%s: cost, group against two-kernel: %d of %d differ, largest |difference| / max(1, |cost|) %.3g"
              % (label, int((cg != ct).sum()), B, float((np.abs(cg - ct) / np.maximum(1.0, np.abs(ct))).max())))
    _bitwise(g, t, label, arrays)
    if arrays == ("cost",):
        return
    ref = _head(refs[variant], B)
    if (ref["polished"] == 1).any():
        for r in (g, t):
            assert_matches_oracle(r, ref, neq, ncon)


@pytest.mark.parametrize("variant", ["per-instance", "shared"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_one_chunk_group_of_sixteen(case20, B, variant):
    _compare(20, case20, B, variant)


@pytest.mark.parametrize("variant", ["per-instance", "shared"])
@pytest.mark.parametrize("B", [7, 8, 9, 17])
def test_two_chunk_group_of_eight(case50, B, variant):
    _compare(50, case50, B, variant, tuple(k for k in ARRAYS if k != "cost"))


@pytest.mark.parametrize("variant", ["per-instance", "shared"])
@pytest.mark.parametrize("B", [7, 8, 9, 17])
def test_two_chunk_group_of_eight_cost(case50, B, variant):
    """The cost of the two-chunk controller, bit for bit between the forms, as the other arrays above.  Such a controller's cost comes from its
    definition; the group form takes it by the two-kernel form's arithmetic (lmpc_cost_mfma's, step for step).  Before round 11 it took one product
    with H per instance inside the solve, and 6 of 7, 7 of 8, 8 of 9 and 16 of 17 of these costs differed from the other form's, by up to 5.6e-12 of
    max(1, |cost|)."""
    _compare(50, case50, B, variant, ("cost",))


@pytest.mark.parametrize("strict", [False, True], ids=["reference-mode", "strict"])
@pytest.mark.parametrize("B", [16, 23])
def test_half_the_instances_outside_their_state_bounds(case20, B, strict):
    """the recipe of test_infeasible_instances_both_modes: every odd instance starts with its roll outside +-pi/6, a fixed row of the QP --
    the first product's flags, gathered over the workgroup, reach the solve of the right instance, in a full workgroup (dealt) and a
    ragged one (not dealt)"""
    import torch
    x0, u0, yref, refs, neq, ncon = case20
    x0 = x0[:B].copy(); u0 = u0[:B]; yref = yref[:B]
    odd = np.arange(B) % 2 == 1
    x0[odd, 0] = 1.0
    g, t = _both_forms(20, x0, u0, yref, strict=strict)
    label = "B=%d strict=%d" % (B, strict)
    _bitwise(g, t, label)
    st = g.status.cpu().numpy(); cmd = g.cmd.cpu().numpy(); feas = g.is_feasible.cpu().numpy(); cost = g.cost.cpu().numpy()
    assert (st[~odd] == 0).all() and (feas[~odd] == 1).all(), label
    if strict:
        assert (st[odd] == 2).all() and np.isnan(cmd[odd]).all() and (feas[odd] == 0).all() and (cost[odd] == 1e30).all(), label
    else:
        ref_bad = quadrotor_oracle(20).solve_batch_constref(x0[odd], u0[odd], yref[odd])
        assert (ref_bad["status"] == 1).all()                   # the reference: MAX_ITER_REACHED, an unconverged iterate
        assert (st[odd] == 1).all() and np.isfinite(cmd).all() and (feas == 1).all(), label
    # the instances inside their bounds are the untouched batch's, to the oracle's tolerances
    ref = _head(refs["per-instance"], B)
    keep = {k: (v[~odd] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}

    class _Sub:
        pass
    sub = _Sub()
    for k in ("cmd", "cost", "status", "active_lower", "active_upper"):
        setattr(sub, k, getattr(g, k).cpu()[torch.from_numpy(~odd)])
    assert_matches_oracle(sub, keep, neq, ncon)
