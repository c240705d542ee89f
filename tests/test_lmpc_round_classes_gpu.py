"""The lean polish round, class by class: a workload whose working sets fall in every size class of ws_solve_reg (pinned by
test_lmpc_round_classes.py), solved by lmpc_solve_group and by the two-kernel form -- each against the CPU oracle at the suite's
tolerances (u* 1e-5, cost 1e-7, active sets bit for bit where the oracle polished), and the two forms against each other bit for bit:
they run the same rounds from the same record.  Linearly dependent working rows (move blocking) take the failed-pivot path and its
retry; ragged batches leave wavefronts of the last workgroup without an instance."""
import numpy as np
import pytest

from helpers import SHAPES_EDGES, SHAPES_MAXIT, axes_batch, axes_spec, oracle_batch_parallel_spec
from test_lmpc_round_classes import round_case
from helpers import assert_matches_oracle, bits_to_rows
from test_lmpc_shapes_gpu import _check, _controller, _head, _move_blocked_rows, _solve

pytestmark = pytest.mark.gpu

GROUP, TWO_KERNEL = 2, 0          # debug_use_fused


@pytest.fixture(scope="module")
def case():
    return round_case()


def _bitwise(a, b, label):
    for k in ("cmd", "cost", "polish_rounds", "active_count"):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        same = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert same, (label, k, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:8])


def test_size_classes_both_forms(case):
    sp, x0, u0, ref = case
    out = {}
    for name, fused in (("group", GROUP), ("two-kernel", TWO_KERNEL)):
        c = _controller(sp, fused=fused)
        if fused == GROUP:
            assert int(c.debug_get("flags")[1]) == 1           # the in-workgroup form takes this controller
        out[name] = _solve(c, x0, u0)
        ac = _check(out[name], ref, sp, name)
        # the lean kernels closed instances in every class themselves (an instance the fallback closed reports iterations or more than 16 rows)
        rounds = out[name].polish_rounds.cpu().numpy()
        lean = (ac <= 16) & (rounds > 0)
        print("%s: lean solves per active_count %s" % (name, np.bincount(ac[lean], minlength=17).tolist()))
    _bitwise(out["group"], out["two-kernel"], "group vs two-kernel")


def _check_blocked(r, ref, spec, label):
    """_check of test_lmpc_shapes_gpu.py for a move-blocked controller, without its demand that the oracle polished nine instances in ten
    (at this batch it polishes three in four; the others are compared at the looser bound of assert_matches_oracle)"""
    pol = ref["polished"] == 1
    assert pol.mean() >= 0.5, (label, pol.mean())
    cmd = r.cmd.cpu().numpy()
    scale = np.abs(ref["cmd"]).max(axis=1)
    # a command that is zero up to round-off, and the oracle's ADMM iterate where its polish failed, have no relative error to speak of
    zero = scale < 1e-10
    assert (np.abs(cmd[zero] - ref["cmd"][zero]).max(axis=1, initial=0.0) <= 1e-12).all(), label
    loose = ~pol & ~zero
    assert (np.abs(cmd[loose] - ref["cmd"][loose]).max(axis=1, initial=0.0) <= 5e-2 * np.maximum(1.0, scale[loose])).all(), label
    assert_matches_oracle(r, dict(ref, cmd=np.where((zero | loose)[:, None], cmd, ref["cmd"])), ref["neq"], ref["ncon"], check_active=False)
    assert np.array_equal(r.status.cpu().numpy(), ref["status"]), label
    assert np.array_equal(r.solver_status.cpu().numpy()[pol], ref["solver_status"][pol]), label
    m, neq = ref["ncon"], ref["neq"]
    lo = bits_to_rows(r.active_lower.cpu().numpy(), m); up = bits_to_rows(r.active_upper.cpu().numpy(), m)
    for b in np.nonzero(pol)[0]:
        rl = np.nonzero(ref["active_lower"][b][neq:])[0] + neq
        ru = np.nonzero(ref["active_upper"][b][neq:])[0] + neq
        assert _move_blocked_rows(lo[b], spec, neq) == _move_blocked_rows(rl, spec, neq), (label, b)
        assert _move_blocked_rows(up[b], spec, neq) == _move_blocked_rows(ru, spec, neq), (label, b)


def test_linearly_dependent_rows_both_forms():
    sp = axes_spec(**SHAPES_EDGES["ch_lt_ph"])
    x0, u0, _ = axes_batch(sp, 128, seed=5)
    ref = oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=SHAPES_MAXIT)
    out = {}
    for name, fused in (("group", GROUP), ("two-kernel", TWO_KERNEL)):
        out[name] = _solve(_controller(sp, fused=fused), x0, u0)
        _check_blocked(out[name], ref, sp, "ch_lt_ph " + name)
    _bitwise(out["group"], out["two-kernel"], "ch_lt_ph group vs two-kernel")


@pytest.mark.parametrize("B", [17, 1])
def test_ragged_batches_group_form(case, B):
    sp, x0, u0, ref = case
    r = _solve(_controller(sp, fused=GROUP), x0[:B], u0[:B])
    _check(r, _head(ref, B), sp, "group B=%d" % B)
