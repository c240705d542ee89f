"""TEST INFRASTRUCTURE -- what tests/test_c2d_gpu.py and tests/test_emu_c2d.py share: the 60-digit truths of tests/golden/c2d_truth.npz
(tests/golden/make_c2d_golden.py) and the bound the discretisation kernel (libmpc_amd/csrc/c2d_kernels.hip) is held to.

The bound, element-wise on [Ad Bd] against the truth E, n = nx + nu, u = 2^-52, s the kernel's documented number of squarings
(the 1-norm of [[A B]; [0 0]] Ts, s = ceil(log2(norm / 0.5)) above 0.5, else 0):

    |out - E| <= 3 n u 2^s max(1, max|E|)

First order: a dot product of length n contributes n u; the Taylor phase (norm <= 1/2, terms falling factorially) less than 2 n u; each squaring
doubles the relative error and adds n u; under 3 n u 2^s in total.  A float64 numpy restatement of the algorithm stays below 0.18 of
n u 2^s max(1, max|E|), sixteen times inside."""
import os

import numpy as np

U = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2d_truth.npz")
TINY = ["tiny_%d_%d" % s for s in ((1, 0), (1, 1), (2, 1), (5, 2), (6, 2), (7, 2))]
LIMIT = ["limit_%d_%d" % s for s in ((40, 5), (45, 1), (40, 8), (47, 1))]
FAMILIES = ["random_g1", "random_g30"] + TINY + ["nu0"] + LIMIT + ["chain", "zero", "cs_edge", "skew", "stiff", "be"]
EXACT = ("chain", "zero")           # families whose results must equal the truth bit for bit

_cache = {}


def case(name):
    """A [m, nx, nx], B [m, nx, nu], Ts [m], Ad, Bd of a family, read-only ("be": B and Bd with Be's three columns appended; "Be" beside them)"""
    if not _cache:
        with np.load(GOLDEN) as z:
            for k in z.files:
                fam, key = k.rsplit(".", 1)
                _cache.setdefault(fam, {})[key] = z[k]
        for c in _cache.values():
            if "Be" in c:
                c["B2"] = c["B"]
                c["B"] = np.concatenate([c["B"], c["Be"]], axis=2)
            for a in c.values():
                a.setflags(write=False)
    return _cache[name]


def squarings(A, B, Ts):
    """the documented rule, per instance"""
    A, B, Ts = np.asarray(A, float), np.asarray(B, float), np.broadcast_to(np.asarray(Ts, float).reshape(-1), (np.shape(A)[0],))
    top = np.concatenate([A, B], axis=2) * Ts[:, None, None]
    norm = np.abs(top).sum(axis=1).max(axis=1)
    s = np.zeros(norm.shape, int)
    big = norm > 0.5
    s[big] = np.ceil(np.log2(norm[big] / 0.5)).astype(int)
    return s


def bound(A, B, Ts, Ad, Bd):
    """[m]: 3 n u 2^s max(1, max|E|) of every instance, E = [Ad Bd] the truth"""
    n = A.shape[1] + B.shape[2]
    E = np.concatenate([Ad, Bd], axis=2).reshape(A.shape[0], -1)
    return 3.0 * n * U * 2.0 ** squarings(A, B, Ts) * np.maximum(1.0, np.abs(E).max(axis=1))


def worst_ratio(A, B, Ts, Ad_true, Bd_true, Ad, Bd):
    """max over the instances and entries of |out - E| / bound (NaN-safe: a non-finite entry gives inf)"""
    m = A.shape[0]
    err = np.abs(np.concatenate([Ad - Ad_true, Bd - Bd_true], axis=2).reshape(m, -1))
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err.max(axis=1) / bound(A, B, Ts, Ad_true, Bd_true)).max())


def check_family(name, Ad, Bd, where=""):
    """the accuracy check of one family; prints and returns the worst error / bound"""
    c = case(name)
    assert Ad.shape == c["Ad"].shape and Bd.shape == c["Bd"].shape, (name, Ad.shape, Bd.shape)
    r = worst_ratio(c["A"], c["B"], c["Ts"], c["Ad"], c["Bd"], Ad, Bd)
    s = squarings(c["A"], c["B"], c["Ts"])
    print("c2d %s%s: squarings %d..%d, worst error / bound %.4f" % (name, where, s.min(), s.max(), r))
    assert r <= 1.0, (name, r)
    if name in EXACT:
        assert np.array_equal(Ad, c["Ad"]) and np.array_equal(Bd, c["Bd"]), name
    return r


def grid_stride_inputs(rng, m, tail):
    """(nx, nu) = (2, 1): m - tail stiff and stable instances (A = Q diag(-l1, -l2) Q^T, l2 in [1000, 3000], Ts = 0.1: a norm above 64), then
    `tail` instances of norm at most 0.5"""
    th = rng.uniform(0.0, 2.0 * np.pi, size=m)
    Q = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    lam = np.stack([rng.uniform(0.1, 1.0, size=m), rng.uniform(1000.0, 3000.0, size=m)], -1)
    A = -np.einsum("bij,bj,bkj->bik", Q, lam, Q)
    B = rng.normal(size=(m, 2, 1))
    Ts = np.full(m, 0.1)
    A[m - tail:] = rng.uniform(-1.0, 1.0, size=(tail, 2, 2)); B[m - tail:] = rng.uniform(-1.0, 1.0, size=(tail, 2, 1)); Ts[m - tail:] = 0.2
    return A, B, Ts
