"""Writes tests/golden/dare_truth.npz: the 60-digit truths that the Riccati kernel (libmpc_amd/csrc/dare_kernels.hip, mpcx_dare_batch) is held to,
read by tests/dare_ref.py for tests/test_dare_gpu.py and tests/test_emu_dare.py.  Needs mpmath; run from the repository root:

    python tests/golden/make_dare_golden.py

Every instance is stored in the control form: A [n, n], B [n, m], Q, R -> X with X = A'XA - A'XB (R + B'XB)^-1 B'XA + Q and the gain
K = (R + B'XB)^-1 B'XA [m, n].  The estimator form of the same instance is (A', C = B') with P = X and L = K' (tests/dare_ref.py).
The truth is the doubling iteration in 60-digit arithmetic, run until the relative change of X is below 1e-45; the relative residual of the
equation is then checked to be below 1e-50."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dare_truth.npz")


def truth(A, B, Q, R):
    A_, B_, Q_, R_ = (mp.matrix(M.tolist()) for M in (A, B, Q, R))
    n = A.shape[0]
    a, g, h = A_, B_ * mp.inverse(R_) * B_.T, Q_
    for _ in range(200):
        Wi = mp.inverse(mp.eye(n) + g * h)
        hn = h + a.T * h * Wi * a
        g = g + a * Wi * g * a.T
        a = a * Wi * a
        d = mp.norm(hn - h, mp.inf)
        h = (hn + hn.T) / 2
        g = (g + g.T) / 2
        if d < mp.mpf(10) ** -45 * mp.norm(h, mp.inf):
            break
    else:
        raise RuntimeError("no convergence")
    X = h
    Si = mp.inverse(R_ + B_.T * X * B_)
    K = Si * B_.T * X * A_
    res = A_.T * X * A_ - A_.T * X * B_ * K + Q_ - X
    rel = mp.norm(res, mp.inf) / mp.norm(X, mp.inf)
    assert rel < mp.mpf(10) ** -50, rel
    f = lambda M: np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])
    return f(X), f(K)


def spd(rng, k, scale):
    M = rng.normal(size=(k, k))
    return scale * (M @ M.T / k + 0.5 * np.eye(k))


def random_instance(rng, n, m, rho, per):
    A = rng.normal(size=(n, n))
    A *= rho / max(abs(np.linalg.eigvals(A)))
    B = rng.normal(size=(n, m))
    Q, R = (spd(rng, n, 0.01), spd(rng, m, 0.04)) if per else (0.01 * np.eye(n), 0.04 * np.eye(m))
    return A, B, Q, R


def chain(q_rank1=False, r=0.04):
    """the integrator chain observed at its head (estimator form: A = I + 0.1 N, C = e1'), stored as its control-form dual"""
    n = 6
    A = np.eye(n) + 0.1 * np.diag(np.ones(n - 1), 1)
    C = np.zeros((1, n)); C[0, 0] = 1.0
    Q = 0.01 * np.eye(n)
    if q_rank1:
        Q = np.zeros((n, n)); Q[-1, -1] = 0.01
    return A.T.copy(), C.T.copy(), Q, r * np.eye(1)


def main():
    rng = np.random.default_rng(20240611)
    fams = {}
    # (n, m), instances, Q and R per instance?
    shapes = [((1, 1), 3, False), ((2, 1), 3, False), ((3, 2), 3, True), ((5, 2), 3, True), ((2, 3), 3, True), ((4, 4), 3, True),
              ((15, 3), 2, False), ((16, 4), 2, True), ((17, 3), 2, False)]
    for (n, m), count, per in shapes:
        fams["shape_%d_%d" % (n, m)] = [random_instance(rng, n, m, 0.9, per) for _ in range(count)]
    fams["limit_n"] = [random_instance(rng, 32, 3, 0.9, False)]
    fams["limit_m"] = [random_instance(rng, 5, 32, 0.9, False)]
    fams["limit_nm"] = [random_instance(rng, 32, 32, 0.9, False)]
    for rho, tag in ((0.5, "050"), (0.98, "098"), (1.3, "130")):
        fams["rho_" + tag] = [random_instance(rng, 8, 3, rho, False) for _ in range(3)]
    fams["chain"] = [chain()]
    fams["chain_rank1q"] = [chain(q_rank1=True)]
    fams["chain_r1e-8"] = [chain(r=1e-8)]
    fams["chain_r1e6"] = [chain(r=1e6)]
    out = {}
    for name, insts in fams.items():
        sols = [truth(*i) for i in insts]
        for key, vals in zip(("A", "B", "Q", "R"), zip(*insts)):
            out[name + "." + key] = np.stack(vals)
        out[name + ".X"] = np.stack([s[0] for s in sols])
        out[name + ".K"] = np.stack([s[1] for s in sols])
        print(name, out[name + ".A"].shape, out[name + ".B"].shape, "max|X| %.3e" % np.abs(out[name + ".X"]).max())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
