"""Round 10 of the lean polish round: the elimination's pivot row and right-hand side broadcast through the LDS crossbar (ds_swizzle), the update's
multipliers read back from LDS, per size class of ws_solve_reg (MPCX_FAST_XBAR_CLASSES).  No floating-point operation changed, so whatever form a class
is built with, every path gives the oracle's results and the paths agree with each other bit for bit.

Workload: that of test_lmpc_round9_classes_gpu.py -- axes_spec(3, 20) (nz = 60, one chunk), the 256 instances of axes_batch(spec, 256, seed=2024).  On
the CPU oracle every working-set size from 1 to 16 occurs at least twice and 98.8 % are polished; instances with more than 16 active rows go to the
fallback kernel.  Tolerances are those of assert_matches_oracle (u* 1e-5, cost 1e-7, active sets bit for bit where the oracle polished).  The coverage
of the sizes 1..16 by solves the lean kernels closed themselves is a condition of the test, not an observation."""
import numpy as np
import pytest

from helpers import assert_matches_oracle, axes_batch, axes_spec, configure_axes, oracle_batch_parallel_spec

pytestmark = pytest.mark.gpu

B = 256
PATHS = [("default", None), ("group", 2), ("two-kernel", 0)]          # debug_use_fused
KEYS = ("cmd", "cost", "status", "polish_rounds", "iterations", "active_count", "active_lower", "active_upper")


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
    """one launch; the results on the host (copied before a later launch may write the same buffers)"""
    import torch
    r = c.optimizeBatch(x0, u0, want_active=True)
    torch.cuda.synchronize()
    return r, {k: getattr(r, k).cpu().numpy().copy() for k in KEYS}


def _check(r, ref, label):
    try:
        assert_matches_oracle(r, ref, ref["neq"], ref["ncon"])
    except AssertionError as e:
        raise AssertionError((label,) + e.args) from e
    st = r.status.cpu().numpy()
    assert np.array_equal(st, ref["status"]), (label, np.nonzero(st != ref["status"])[0][:8])


def _assert_same(a, b, label, rows=None):
    for k in KEYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        same = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert same, (label, k, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:8])


@pytest.fixture(scope="module")
def solved(case):
    """the batch once on each path"""
    sp, x0, u0, ref = case
    out = {}
    for name, fused in PATHS:
        c = _controller(sp, fused)
        if name in ("default", "group"):
            assert int(c.debug_get("flags")[1]) == 1           # the in-workgroup form takes this controller
        out[name] = _solve(c, x0, u0)
    return out


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_every_size_class_against_the_oracle(case, solved, path):
    ref = case[3]
    r, h = solved[path]
    _check(r, ref, path)
    ac = h["active_count"].astype(np.int64)
    lean = (ac <= 16) & (h["polish_rounds"] > 0) & (h["iterations"] == 0)       # closed by the lean kernels, not by the fallback
    counts = np.bincount(ac[lean], minlength=17)
    print("%s: lean solves per active_count %s" % (path, counts.tolist()))
    assert (counts[1:17] > 0).all(), (path, counts.tolist())


def test_group_and_two_kernel_paths_bit_for_bit(solved):
    _assert_same(solved["group"][1], solved["two-kernel"][1], "group vs two-kernel")
    _assert_same(solved["default"][1], solved["group"][1], "default vs group")


def _rows(ref, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


@pytest.mark.parametrize("n", [1, 17])
def test_partly_filled_workgroups(case, solved, n):
    """wavefronts without an instance beside the broadcasts: one instance alone (the first one the oracle polished with a working set the lean kernels
    take), and one full workgroup plus one instance"""
    sp, x0, u0, ref = case
    first = int(np.nonzero((ref["polished"] == 1) & (ref["n_active"] >= 1) & (ref["n_active"] <= 16))[0][0])
    rows = np.arange(first, first + 1) if n == 1 else np.arange(n)
    r, h = _solve(_controller(sp, 2), x0[rows], u0[rows])
    _check(r, _rows(ref, rows), "group B=%d" % n)
    _assert_same(h, {k: v[rows] for k, v in solved["group"][1].items()}, "group B=%d vs B=%d" % (n, B))


def test_two_launches_repeat_bit_for_bit(case, solved):
    """a crossbar result or an LDS read consumed ahead of its wait would show as a difference between two launches (the timing differs)"""
    sp, x0, u0, _ = case
    c = _controller(sp, 2)
    _, first = _solve(c, x0, u0)
    _, second = _solve(c, x0, u0)
    _assert_same(first, second, "first vs second launch")
    _assert_same(first, solved["group"][1], "another controller")


def test_bad_neighbour_in_the_workgroup(case, solved):
    """one instance of a workgroup of sixteen starts from a NaN: every value of its wavefront is NaN, crossbar traffic and LDS slice included.  It ends as
    the kernels before this round end it (measured on them, this test run against the parent's library): the lean kernel's NaN screen leaves it to the
    fallback, whose ADMM loop runs to the iteration limit on NaNs -- iterations 4000 (configure_axes' maximum_iteration), polish_rounds 400, status 0,
    no active row, cost and command NaN -- and its fifteen neighbours are bit for bit what they are without it."""
    sp, x0, u0, _ = case
    bad = 21                                                    # workgroup 1 = instances 16..31
    xb = x0[:48].copy(); xb[bad, 0] = np.nan
    r, h = _solve(_controller(sp, 2), xb, u0[:48])
    good = np.delete(np.arange(48), bad)
    _assert_same(h, {k: v[:48] for k, v in solved["group"][1].items()}, "neighbours of a NaN instance", rows=good)
    print("NaN instance: status %d iterations %d polish_rounds %d active_count %d cost %r cmd %r" %
          (h["status"][bad], h["iterations"][bad], h["polish_rounds"][bad], h["active_count"][bad], h["cost"][bad], h["cmd"][bad]))
    assert h["status"][bad] == 0 and h["iterations"][bad] == 4000 and h["polish_rounds"][bad] == 400 and h["active_count"][bad] == 0
    assert np.isnan(h["cost"][bad]) and np.isnan(h["cmd"][bad]).all()
