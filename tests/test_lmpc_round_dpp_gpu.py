"""Round 12 of the lean polish round, end to end: the elimination of ws_solve_reg (csrc/lmpc_fast.hip) takes its pivot row and right-hand side by DPP row
broadcast inside the FMA, per size class (MPCX_FAST_DPP_CLASSES).  No floating-point operation changed, so whatever form a class is built with, every
path gives the oracle's results.  test_lmpc_round_bcast_gpu.py runs the one-chunk kernels of a single controller; this file adds the kernels it does not
run -- lmpc_solve_hetero through a bank, the two-chunk lmpc_solve<2, 2> and lmpc_solve_group<2, 2> -- and a non-finite instance in a workgroup.

One chunk: the fixture of test_lmpc_round_bcast_gpu.py, axes_spec(3, 20) and the 256 instances of axes_batch(spec, 256, seed=2024); on the CPU oracle every
working-set size from 1 to 16 occurs at least twice and 98.8 % are polished.  Two chunks: the quadrotor controller at N = 50 of
test_lmpc_group_head_gpu.py on the 64 instances quadrotor_batch(64, first=3584), chosen on the CPU oracle: all 64 polished, none with more than 16 active
rows, active rows per instance 0: 1, 1: 1, 2: 2, 3: 10, 4: 7, 5: 11, 6: 9, 7: 5, 8: 5, 9: 4, 10: 2, 11: 4, 12: 1, 14: 1, 15: 1 -- per size class (1-4, 5-6, 7-8,
9-10, 11-12, 13-14, 15-16 rows) 20, 20, 10, 6, 5, 1, 1.  Tolerances are those of assert_matches_oracle (u* 1e-5, cost 1e-7, active sets bit for bit where the
oracle polished).  The coverage conditions are conditions of the tests, not observations."""
import numpy as np
import pytest

from helpers import assert_matches_oracle, axes_batch, axes_spec, configure_axes, oracle_batch_parallel_spec, quadrotor_oracle

pytestmark = pytest.mark.gpu

B = 256
NBANK = 16
KEYS = ("cmd", "cost", "status", "polish_rounds", "iterations", "active_count", "active_lower", "active_upper")
CLASSES = [(1, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
B50, FIRST50 = 64, 3584


def _host(r):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy().copy() for k in KEYS}


def _assert_same(a, b, label, rows=None):
    for k in KEYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        same = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert same, (label, k, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:8])


def _lean_counts(h):
    ac = h["active_count"].astype(np.int64)
    lean = (ac <= 16) & (h["polish_rounds"] > 0) & (h["iterations"] == 0)       # closed by the lean kernels, not by the fallback
    return np.bincount(ac[lean], minlength=17)


@pytest.fixture(scope="module")
def case():
    sp = axes_spec(3, 20)
    x0, u0, _ = axes_batch(sp, B, seed=2024)
    ref = oracle_batch_parallel_spec(sp, x0, u0)
    assert (ref["polished"] == 1).mean() >= 0.9
    return sp, x0, u0, ref


def _single(sp, fused):
    from libmpc_amd import LMPC
    c = configure_axes(LMPC(*sp["dims"], device=0), sp)
    c.debug_use_fused(fused)
    return c


@pytest.fixture(scope="module")
def two_kernel(case):
    sp, x0, u0, _ = case
    r = _single(sp, 0).optimizeBatch(x0, u0, want_active=True)
    return _host(r)


@pytest.fixture(scope="module")
def bank(case):
    """sixteen copies of the controller as a bank; instance b on controller b mod 16"""
    from libmpc_amd import LMPC, LMPCHetero
    sp, x0, u0, _ = case
    het = LMPCHetero([configure_axes(LMPC(*sp["dims"], device=-1), sp) for _ in range(NBANK)], device=0)
    r = het.optimizeBatch(x0, u0, model=np.arange(B) % NBANK, want_active=True)
    return r, _host(r)


def test_bank_every_size_class_against_the_oracle(case, bank):
    ref = case[3]
    r, h = bank
    assert_matches_oracle(r, ref, ref["neq"], ref["ncon"])
    assert np.array_equal(h["status"], ref["status"]), np.nonzero(h["status"] != ref["status"])[0][:8]
    counts = _lean_counts(h)
    print("bank: lean solves per active_count %s" % counts.tolist())
    assert (counts[1:17] > 0).all(), counts.tolist()


def test_bank_and_two_kernel_paths_agree(bank, two_kernel):
    """the bank path against the two-kernel path of the single controller.  Measured on the library before this round (this recipe against the parent's
    library, the bank condensed on the device and on the host alike): the two paths are NOT bit-equal in the command and the cost -- 255 of the 256 commands
    differ by up to 5.2e-14, 248 to 250 of the costs by up to 4.6e-12: a bank instance's record comes from its own controller's matrices through the bank's
    assemble, not from the single controller's -- while status, polish_rounds, iterations, active_count and both active bitmaps are equal bit for bit.  So
    the bitwise comparison holds what was equal before, and the command and the cost are held to rounding-level bounds: two evaluation orders of the same
    sums of at most nz = 60 terms per entry, chained through the record, the solve and the unpack -- a few thousand roundings of eps = 1.1e-16 on values of
    order 1, i.e. 1e-12 absolute on the commands (|u| <= 1); the cost is a quadratic form of 60 x 60 terms that cancel to it, 1e-10 of max(1, |cost|)."""
    h = bank[1]
    for k in ("status", "polish_rounds", "iterations", "active_count", "active_lower", "active_upper"):
        assert np.array_equal(h[k], two_kernel[k]), (k, np.nonzero((h[k] != two_kernel[k]).reshape(B, -1).any(axis=1))[0][:8])
    dc = np.abs(h["cmd"] - two_kernel["cmd"]).max()
    dj = (np.abs(h["cost"] - two_kernel["cost"]) / np.maximum(1.0, np.abs(two_kernel["cost"]))).max()
    print("bank vs two-kernel: largest |cmd difference| %.3g, largest relative cost difference %.3g" % (dc, dj))
    assert dc <= 1e-12 and dj <= 1e-10, (dc, dj)


@pytest.fixture(scope="module")
def case50():
    from libmpc_amd.workloads import quadrotor_batch
    x0, u0, yref = quadrotor_batch(B50, first=FIRST50)
    o = quadrotor_oracle(50)
    ref = o.solve_batch_constref(x0, u0, yref, want_active=True)
    # the choice of the batch, held here: the oracle alone meets the coverage condition
    n = ((ref["active_lower"][:, o.neq:] != 0) | (ref["active_upper"][:, o.neq:] != 0)).sum(axis=1)
    pol = ref["polished"] == 1
    assert pol.all() and (n <= 16).all()
    assert [int(((n >= lo) & (n <= hi)).sum()) for lo, hi in CLASSES] == [20, 20, 10, 6, 5, 1, 1]
    return x0, u0, yref, ref, o.neq, o.ncon


@pytest.mark.parametrize("path,fused", [("two-kernel", 0), ("group", 2)])
def test_two_chunks_every_size_class_against_the_oracle(case50, path, fused):
    from libmpc_amd.workloads import quadrotor_lmpc
    x0, u0, yref, ref, neq, ncon = case50
    c = quadrotor_lmpc(50, device=0)
    c.debug_use_fused(fused)
    if fused == 2:
        assert int(c.debug_get("flags")[1]) == 1               # the in-workgroup form takes this controller
    r = c.optimizeBatch(x0, u0, yref=yref, want_active=True)
    h = _host(r)
    assert_matches_oracle(r, ref, neq, ncon)
    counts = _lean_counts(h)
    per_class = [int(counts[lo:hi + 1].sum()) for lo, hi in CLASSES]
    print("N=50 %s: lean solves per active_count %s, per class %s" % (path, counts.tolist(), per_class))
    assert min(per_class) > 0, (path, per_class)


def test_infinite_neighbour_in_the_workgroup(case):
    """one instance of a workgroup of sixteen starts from x0[0] = inf, in the manner of test_bad_neighbour_in_the_workgroup: a non-finite entry in a pivot
    row is where the DPP form differs from the scalar reads (lane K's row turns NaN where it stayed inf), and the NaN screen takes such an instance in both.
    It ends as the library before this round ends it (measured on it, this test's recipe run against the parent's library): left to the fallback, whose
    ADMM loop runs to the iteration limit -- iterations 4000 (configure_axes' maximum_iteration), polish_rounds 400, status 0, no active row, cost and
    command NaN -- and its fifteen neighbours are bit for bit what they are without it."""
    sp, x0, u0, _ = case
    clean = _host(_single(sp, 2).optimizeBatch(x0[:48], u0[:48], want_active=True))
    bad = 21                                                    # workgroup 1 = instances 16..31
    xb = x0[:48].copy(); xb[bad, 0] = np.inf
    h = _host(_single(sp, 2).optimizeBatch(xb, u0[:48], want_active=True))
    good = np.delete(np.arange(48), bad)
    _assert_same(h, clean, "neighbours of an inf instance", rows=good)
    print("inf instance: status %d iterations %d polish_rounds %d active_count %d cost %r cmd %r" %
          (h["status"][bad], h["iterations"][bad], h["polish_rounds"][bad], h["active_count"][bad], h["cost"][bad], h["cmd"][bad]))
    assert h["status"][bad] == 0 and h["iterations"][bad] == 4000 and h["polish_rounds"][bad] == 400 and h["active_count"][bad] == 0
    assert np.isnan(h["cost"][bad]) and np.isnan(h["cmd"][bad]).all()
