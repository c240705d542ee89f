"""Round 9 of the lean polish round (pipelined rows of Y, branch-free verify phase): every size class of ws_solve_reg at both working-set
sizes of its class, on each launch path, against the CPU oracle.

Workload: axes_spec(3, 20) (nz = 60, one chunk; bounded state rows, so box rows and general rows are both exercised), the 256 instances of
axes_batch(spec, 256, seed=2024).  On the CPU oracle 90 of the 256 optima hold at most 16 active rows (2 of them none), every size from 1 to 16 occurs
at least twice and 98.8 % are polished; the other 166 instances go to the fallback kernel.  Tolerances are those of assert_matches_oracle (u* 1e-5, cost 1e-7,
active sets bit for bit where the oracle polished).  The coverage of the sizes 1..16 is a condition of the test, not an observation.

(tests/test_lmpc_round_classes_gpu.py is round 8's test of the same kernels on another draw and is left as it is.)"""
import numpy as np
import pytest

from helpers import assert_matches_oracle, axes_batch, axes_spec, configure_axes, oracle_batch_parallel_spec

pytestmark = pytest.mark.gpu

B = 256
PATHS = [("default", None), ("group", 2), ("two-kernel", 0)]          # debug_use_fused


@pytest.fixture(scope="module")
def case():
    sp = axes_spec(3, 20)
    x0, u0, _ = axes_batch(sp, B, seed=2024)
    ref = oracle_batch_parallel_spec(sp, x0, u0)
    pol = (ref["polished"] == 1).mean()
    assert pol >= 0.9, pol
    return sp, x0, u0, ref


def _controller(sp, fused):
    from libmpc_amd import LMPC
    c = configure_axes(LMPC(*sp["dims"], device=0), sp)
    if fused is not None:
        c.debug_use_fused(fused)
    return c


def _solve(c, x0, u0):
    import torch
    r = c.optimizeBatch(x0, u0, want_active=True)
    torch.cuda.synchronize()
    return r


def _head(ref, n):
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


def _check(r, ref, label):
    """the oracle's tolerances and its status; returns the active_count of the instances the lean kernels closed themselves (an instance
    the fallback closed reports ADMM iterations or more than 16 rows)"""
    try:
        assert_matches_oracle(r, ref, ref["neq"], ref["ncon"])
    except AssertionError as e:
        raise AssertionError((label,) + e.args) from e
    st = r.status.cpu().numpy()
    assert np.array_equal(st, ref["status"]), (label, np.nonzero(st != ref["status"])[0][:8])
    ac = r.active_count.cpu().numpy().astype(np.int64)
    lean = (ac <= 16) & (r.polish_rounds.cpu().numpy() > 0) & (r.iterations.cpu().numpy() == 0)
    return ac[lean]


@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0])
def test_every_size_class_at_both_sizes(case, path):
    sp, x0, u0, ref = case
    name, fused = path
    c = _controller(sp, fused)
    if name in ("default", "group"):
        assert int(c.debug_get("flags")[1]) == 1           # the in-workgroup form takes this controller
    ac = _check(_solve(c, x0, u0), ref, name)
    counts = np.bincount(ac, minlength=17)
    print("%s: lean solves per active_count %s" % (name, counts.tolist()))
    assert (counts[1:17] > 0).all(), (name, counts.tolist())


def test_ragged_tail_group_form(case):
    """one full workgroup and one instance: the pipelined loads run next to idle wavefronts"""
    sp, x0, u0, ref = case
    _check(_solve(_controller(sp, 2), x0[:17], u0[:17]), _head(ref, 17), "group B=17")


def test_two_launches_repeat_bit_for_bit(case):
    """a load issued early into a register that is still read would show as a difference between two launches (the timing differs)"""
    sp, x0, u0, ref = case
    c = _controller(sp, 2)
    keys = ("cmd", "cost", "polish_rounds", "active_count")
    r = _solve(c, x0, u0)
    first = {k: getattr(r, k).cpu().numpy().copy() for k in keys}          # (on the host before the second launch: it may write the same buffers)
    r = _solve(c, x0, u0)
    for k in keys:
        x, y = first[k], getattr(r, k).cpu().numpy()
        same = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert same, (k, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:8])
