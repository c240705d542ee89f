"""The workload of test_lmpc_round_classes_gpu.py reaches every size class of the lean polish round (ws_solve_reg<CAP>, CAP = 4, 6, ..., 16)
and the hand-over to the fallback kernel.  Oracle only (no GPU), so that the GPU test cannot silently stop reaching a class."""
import numpy as np

from helpers import SHAPES_MAXIT, axes_batch, axes_spec, oracle_batch_parallel_spec

# the workload both files use: variant 1 (nz = 60), one fixed draw of 256 instances
ROUND_SPEC = dict(nax=3, ph=20)
ROUND_BATCH = 256
ROUND_SEED = 31
# working-set sizes per size class of the round: none, then the classes of ws_solve_reg, then more than the lean kernels hold
ROUND_CLASSES = [(0, 0), (1, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]


def round_case():
    sp = axes_spec(**ROUND_SPEC)
    x0, u0, _ = axes_batch(sp, ROUND_BATCH, seed=ROUND_SEED)
    return sp, x0, u0, oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=SHAPES_MAXIT)


def test_oracle_active_sets_fall_in_every_size_class():
    """The oracle's n_active over the 256 instances, per class 0 | 1-4 | 5-6 | 7-8 | 9-10 | 11-12 | 13-14 | 15-16 | more than 16:
    7 | 14 | 10 | 7 | 8 | 8 | 7 | 6 | 189 (252 of the 256 polished).  At least three in each."""
    sp, x0, u0, ref = round_case()
    na = ref["n_active"]
    assert len(na) == ROUND_BATCH
    counts = [int(((na >= lo) & (na <= hi)).sum()) for lo, hi in ROUND_CLASSES]
    over = int((na > 16).sum())
    print("n_active per class %s, past 16: %d, polished %d" % (counts, over, int((ref["polished"] == 1).sum())))
    assert min(counts) >= 3, counts
    assert over >= 3, over
    assert (ref["status"] == 0).all()
    assert np.isfinite(ref["cmd"]).all()
