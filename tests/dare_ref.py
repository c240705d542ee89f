"""TEST INFRASTRUCTURE -- what tests/test_dare_gpu.py and tests/test_emu_dare.py share: the 60-digit truths of tests/golden/dare_truth.npz
(tests/golden/make_dare_golden.py), the families, and the bound the Riccati kernel (libmpc_amd/csrc/dare_kernels.hip) is held to.

The bound, element-wise against the truth X* (and K* for the gain, with its own magnitude), u = 2^-52:

    |X - X*| <= C n u max|X*|,      |K - K*| <= C n u max|K*|

C is not taken from the kernel: `restate` below is a float64 numpy restatement of the kernel's algorithm (Cholesky of R, g_0 = Y'Y, the
doubling step with [W | a | g] eliminated by partial pivoting with reciprocal pivots, symmetrised increments, the stopping rule, the gain
through the Cholesky factor of R + B'XB), and C is 8 times the worst ratio error / (n u max|truth|) that the restatement reaches over the
families (c2d's bound sits 16 times above its restatement; a doubling iteration has fewer error-doubling steps).  The restatement's ratios,
max(X, gain) per family (python tests/dare_ref.py prints them):

    shape_1_1      X   1.64   gain   1.99   doublings  8
    shape_2_1      X   1.67   gain   2.51   doublings  9
    shape_3_2      X   0.38   gain   1.67   doublings  7
    shape_5_2      X   0.18   gain   0.44   doublings  8
    shape_2_3      X   0.33   gain   2.08   doublings  6
    shape_4_4      X   0.22   gain   0.54   doublings  6
    shape_15_3     X   0.11   gain   0.21   doublings  7
    shape_16_4     X   0.24   gain   0.23   doublings  7
    shape_17_3     X   0.15   gain   0.20   doublings  8
    rho_050        X   0.08   gain   0.20   doublings  6
    rho_098        X   0.22   gain   0.66   doublings  7
    rho_130        X   0.21   gain   0.35   doublings  7
    chain          X   0.54   gain   0.22   doublings 10
    chain_rank1q   X  12.86   gain   4.33   doublings 11
    chain_r1e-8    X   0.65   gain   0.39   doublings 10
    chain_r1e6     X   6.78   gain   3.48   doublings 13
    limit_n        X   0.17   gain   0.17   doublings  8
    limit_m        X   0.13   gain   1.21   doublings  5
    limit_nm       X   0.05   gain   0.38   doublings  5

The worst is the integrator chain with a rank-one Q, as with every method tried on it (an ill-conditioned equation: the closed loop has
its poles close to the unit circle); C = 8 x 12.86 = 102.88."""
import os

import numpy as np

U = 2.0 ** -52
C_BOUND = 8 * 12.86
MAX_DOUBLINGS = 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dare_truth.npz")
SHAPES = ["shape_%d_%d" % s for s in ((1, 1), (2, 1), (3, 2), (5, 2), (2, 3), (4, 4), (15, 3), (16, 4), (17, 3))]
LIMIT = ["limit_n", "limit_m", "limit_nm"]                          # (32, 3), (5, 32), (32, 32)
CONDITIONING = ["rho_050", "rho_098", "rho_130", "chain", "chain_rank1q", "chain_r1e-8", "chain_r1e6"]
FAMILIES = SHAPES + CONDITIONING + LIMIT
FORMS = ("control", "estimator")

_cache = {}


def case(name):
    """A [k, n, n], B [k, n, m], Q [k, n, n], R [k, m, m], X [k, n, n], K [k, m, n] of a family in the control form, read-only; "shared": Q and R
    are the same for every instance"""
    if not _cache:
        with np.load(GOLDEN) as z:
            for k in z.files:
                fam, key = k.rsplit(".", 1)
                _cache.setdefault(fam, {})[key] = z[k]
        for c in _cache.values():
            for a in c.values():
                a.setflags(write=False)
            c["shared"] = bool((c["Q"] == c["Q"][0]).all() and (c["R"] == c["R"][0]).all())
    return _cache[name]


def inputs(name, form):
    """(A, BorC, Q, R) of a family as the front-end takes them in that form, row-major: the estimator form of an instance is (A', C = B')"""
    c = case(name)
    if form == "control":
        return c["A"], c["B"], c["Q"], c["R"]
    return np.swapaxes(c["A"], 1, 2), np.swapaxes(c["B"], 1, 2), c["Q"], c["R"]


def truth(name, form):
    """(X, gain): K [k, m, n] in the control form, L = K' [k, n, m] in the estimator form"""
    c = case(name)
    return c["X"], (c["K"] if form == "control" else np.swapaxes(c["K"], 1, 2))


def ratios(X, G, Xt, Gt):
    """worst |error| / (n u max|truth|) over the instances, of X and of the gain (a non-finite entry gives inf)"""
    n = Xt.shape[1]

    def one(a, t):
        k = t.shape[0]
        err = np.abs(a - t).reshape(k, -1)
        err = np.where(np.isfinite(err), err, np.inf)
        return float((err.max(axis=1) / (n * U * np.abs(t).reshape(k, -1).max(axis=1))).max())
    return one(X, Xt), one(G, Gt)


def check_family(name, form, X, G, where=""):
    """the accuracy check of one family in one form; prints and returns the worst error / bound"""
    Xt, Gt = truth(name, form)
    assert X.shape == Xt.shape and G.shape == Gt.shape, (name, form, X.shape, G.shape)
    rx, rg = ratios(X, G, Xt, Gt)
    print("dare %s %s%s: worst error / bound: X %.4f, gain %.4f" % (name, form, where, rx / C_BOUND, rg / C_BOUND))
    assert rx <= C_BOUND and rg <= C_BOUND, (name, form, rx, rg, C_BOUND)
    return max(rx, rg) / C_BOUND


def _chol(S):
    """the kernel's right-looking Cholesky; None where a pivot is not positive and finite"""
    S = S.copy()
    m = S.shape[0]
    for k in range(m):
        d = S[k, k]
        if not (d > 0.0 and np.isfinite(d)):
            return None
        S[k:, k] = np.concatenate([[np.sqrt(d)], S[k + 1:, k] / np.sqrt(d)])
        S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k], S[k + 1:, k])
    return np.tril(S)


def _tri_solve(L, Y, both):
    Y = Y.copy()
    m = L.shape[0]
    for i in range(m):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    if both:
        for i in range(m - 1, -1, -1):
            Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def _lu_solve(W, T):
    """W^-1 T as the kernel forms it: [W | T] eliminated with partial pivoting and reciprocal pivots, then back-substituted"""
    n = W.shape[0]
    M = np.concatenate([W, T], axis=1)
    for k in range(n):
        col = np.abs(M[k:, k])
        if not np.isfinite(col).all() or not col.max() > 0.0:
            return None
        p = k + int(np.argmax(col))
        if p != k:
            M[[k, p]] = M[[p, k]]
        lfac = M[k + 1:, k] * (1.0 / M[k, k])
        M[k + 1:, k + 1:] -= np.outer(lfac, M[k, k + 1:])
    Xs = M[:, n:]
    for i in range(n - 1, -1, -1):
        Xs[i] = (Xs[i] - M[i, i + 1:n] @ Xs[i + 1:]) / M[i, i]
    return Xs


def restate(A, B, Q, R):
    """one instance in the control form, float64: (X, K, flag, doublings) by the kernel's algorithm"""
    n, m = B.shape
    nanX, nanK = np.full((n, n), np.nan), np.full((m, n), np.nan)
    L = _chol(0.5 * (R + R.T))
    if L is None:
        return nanX, nanK, 1, 0
    Y = _tri_solve(L, B.T, False)
    a, g, h = A.copy(), Y.T @ Y, 0.5 * (Q + Q.T)
    flag, it = 2, 0
    with np.errstate(all="ignore"):
        while it < MAX_DOUBLINGS:
            it += 1
            T = _lu_solve(np.eye(n) + g @ h, np.concatenate([a, g], axis=1))
            if T is None:
                flag = 3
                break
            T1, T2 = T[:, :n], T[:, n:]
            P = (a @ T2) @ a.T
            g = g + 0.5 * (P + P.T)
            P = (a.T @ h) @ T1
            d = 0.5 * (P + P.T)
            h = h + d
            a = a @ T1
            if not (np.isfinite(a).all() and np.isfinite(g).all() and np.isfinite(h).all()):
                flag = 3
                break
            if np.abs(d).max() <= U * np.abs(h).max():
                flag = 0
                break
    if flag:
        return nanX, nanK, flag, it
    Yx = B.T @ h
    S = Yx @ B
    Ls = _chol(0.5 * (S + S.T) + 0.5 * (R + R.T))
    if Ls is None:
        return nanX, nanK, 3, it
    return h, _tri_solve(Ls, Yx @ A, True), 0, it


def restatement_ratios():
    """{family: (ratio of X, ratio of the gain, doublings)} of the restatement against the truths"""
    out = {}
    for name in FAMILIES:
        c = case(name)
        sols = [restate(c["A"][i], c["B"][i], c["Q"][i], c["R"][i]) for i in range(c["A"].shape[0])]
        assert all(s[2] == 0 for s in sols), name
        rx, rg = ratios(np.stack([s[0] for s in sols]), np.stack([s[1] for s in sols]), c["X"], c["K"])
        out[name] = (rx, rg, max(s[3] for s in sols))
    return out


if __name__ == "__main__":
    r = restatement_ratios()
    for name, (rx, rg, it) in r.items():
        print("    %-14s X %6.2f   gain %6.2f   doublings %2d" % (name, rx, rg, it))
    worst = max(max(v[:2]) for v in r.values())
    print("worst %.3f -> C = %.1f" % (worst, 8 * worst))
