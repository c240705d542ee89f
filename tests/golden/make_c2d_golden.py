"""Writes tests/golden/c2d_truth.npz: inputs and 60-digit truths for the discretisation kernel (libmpc_amd/csrc/c2d_kernels.hip,
mpcx_discretize_batch), read by tests/test_c2d_gpu.py and tests/test_emu_c2d.py.

The truth of every instance is [Ad Bd] = the first nx rows of exp([[A B]; [0 0]] Ts), computed by mpmath at mp.dps = 60
(mpmath.expm, method="taylor") from the float64 inputs taken exactly (the product with Ts is formed in mpmath, not in double) and
rounded once to float64.  The tests need only the .npz: mpmath is a requirement of this script alone.

Keys: "<family>.A" [m, nx, nx], ".B" [m, nx, nu], ".Ts" [m], ".Ad" [m, nx, nx], ".Bd" [m, nx, nu]; row-major matrices, as
libmpc_amd.utils.discretization takes them.  The family "be" also has ".Be" [m, nx, 3]; its ".Bd" is [m, nx, 2 + 3], the truth
of B with Be appended to its columns (reference include/mpc/Utils.hpp:63-89).

Families (seeds: default_rng(4100 + position in FAMILIES)):
  random_g1, random_g30   nx 9, nu 4: normal A times 1 and times 30, normal B, Ts in [0.005, 0.3] with both ends present -- the
                          regime of tests/test_utils.py, 0 to 8 squarings, unsymmetric
  tiny_<nx>_<nu>          (1,0) (1,1) (2,1) (5,2) (6,2) (7,2): (nx+nu)^2 = 1, 4, 9, 49, 64, 81 around one pass of the kernel's
                          loops of stride 64
  nu0                     nx 5, nu 0
  limit_<nx>_<nu>         (40,5) (45,1) (40,8) (47,1): n = 45 (the last under 64 KiB of LDS), 46, 48, 48; one instance each, the
                          inputs multiples of 2^-6 so that they compress (the truths cannot)
  chain                   nx 6, nu 6: three double integrators' worth of positions over velocities over inputs (nilpotent:
                          Ad = [I Ts I; 0 I], Bd = [Ts^2/2 I; Ts I]); Ts 0.02, 0.3 and 0.5 need no squaring, 0.75 and 3 are short
                          dyadic numbers whose squares are exact -- so every operation of the kernel is exact but the one rounding
                          of Ts^2, which the truth has too
  zero                    nx 3, nu 2: A = B = 0 at Ts = 0.1; random A, B at Ts = 0; both: Ad = I, Bd = 0
  cs_edge                 nx 4, nu 2: entries multiples of 2^-10 (of 2^-9 at Ts = 0.5) with the largest absolute column sum of
                          [[A B]; [0 0]] Ts exactly 0.5 (instances 0-2: in a column of A, of B, of A at Ts = 0.5) and exactly 1.0
                          (3-5 likewise): the edges of the squaring rule, the sums exact in any order
  skew                    nx 10, nu 3: A = 20 (R - R^T), Ts = 0.2: a large norm, exp(A Ts) orthogonal, about 7 squarings
  stiff                   nx 8, nu 2: A = Q diag(-10^[-1 .. 3.5]) Q^T, Ts = 0.1: about 11 squarings
  be                      nx 6, nu 2 + 3

Run from the repository root (about a minute, nearly all of it the four limit instances):  python tests/golden/make_c2d_golden.py"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = [(1, 0), (1, 1), (2, 1), (5, 2), (6, 2), (7, 2)]
LIMIT = [(40, 5), (45, 1), (40, 8), (47, 1)]
FAMILIES = (["random_g1", "random_g30"] + ["tiny_%d_%d" % s for s in TINY] + ["nu0"] + ["limit_%d_%d" % s for s in LIMIT] +
            ["chain", "zero", "cs_edge", "skew", "stiff", "be"])


def truth(A, B, Ts):
    """the first nx rows of exp([[A B]; [0 0]] Ts) at 60 digits, rounded to float64"""
    import mpmath as mp
    mp.mp.dps = 60
    nx, nu = B.shape
    n = nx + nu
    M = mp.zeros(n, n)
    t = mp.mpf(float(Ts))
    for i in range(nx):
        for j in range(n):
            M[i, j] = mp.mpf(float(A[i, j] if j < nx else B[i, j - nx])) * t
    E = mp.expm(M, method="taylor")
    out = np.array([[float(E[i, j]) for j in range(n)] for i in range(nx)]).reshape(nx, n)
    return out[:, :nx], out[:, nx:]


def _ts(rng, m):
    ts = rng.uniform(0.005, 0.3, size=m)
    ts[0], ts[-1] = 0.005, 0.3
    return ts


def _cs_edge(rng):
    """integers over 1024 with one column's absolute sum exactly `target`, every other column's below 0.25"""
    nx, nu = 4, 2
    As, Bs, Ts = [], [], []
    for target in (512, 1024):
        for col, ts in ((1, 1.0), (nx + 1, 1.0), (2, 0.5)):
            top = rng.integers(-60, 61, size=(nx, nx + nu))
            c = rng.integers(50, 151, size=nx) * rng.choice([-1, 1], size=nx)
            c[nx - 1] = -(target - np.abs(c[:nx - 1]).sum())
            top[:, col] = c
            assert np.abs(top).sum(axis=0).max() == target == np.abs(top[:, col]).sum()
            top = top / 1024.0 / ts
            As.append(top[:, :nx]); Bs.append(top[:, nx:]); Ts.append(ts)
    return np.array(As), np.array(Bs), np.array(Ts)


def inputs(name, rng):
    """A [m, nx, nx], B [m, nx, nu], Ts [m] of a family (for "be": B has the 2 + 3 columns)"""
    if name.startswith("random_g"):
        m, nx, nu = 4, 9, 4
        return rng.normal(size=(m, nx, nx)) * float(name[8:]), rng.normal(size=(m, nx, nu)), _ts(rng, m)
    if name.startswith("tiny_"):
        nx, nu = map(int, name.split("_")[1:])
        m = 3
        return rng.normal(size=(m, nx, nx)) * np.array([0.3, 3.0, 20.0])[:, None, None], rng.normal(size=(m, nx, nu)), _ts(rng, m)
    if name == "nu0":
        m = 4
        return rng.normal(size=(m, 5, 5)) * np.array([0.5, 2.0, 8.0, 30.0])[:, None, None], np.zeros((m, 5, 0)), _ts(rng, m)
    if name.startswith("limit_"):
        nx, nu = map(int, name.split("_")[1:])
        q = lambda a: np.round(a * 64.0) / 64.0
        return q(rng.normal(size=(1, nx, nx))), q(rng.normal(size=(1, nx, nu))), np.array([0.125])
    if name == "chain":
        ts = np.array([0.02, 0.3, 0.5, 0.75, 3.0])
        A = np.zeros((6, 6)); A[:3, 3:] = np.eye(3)          # positions over velocities ...
        B = np.zeros((6, 6)); B[3:, :3] = np.eye(3)          # ... over three forces; three inputs that act on nothing
        return np.repeat(A[None], ts.size, 0), np.repeat(B[None], ts.size, 0), ts
    if name == "zero":
        A = np.zeros((3, 3, 3)); B = np.zeros((3, 3, 2))
        A[1:] = rng.normal(size=(2, 3, 3)) * 5.0; B[1:] = rng.normal(size=(2, 3, 2))
        A[2] = -np.abs(A[2])                                  # (every product with Ts = 0 a negative zero)
        return A, B, np.array([0.1, 0.0, 0.0])
    if name == "cs_edge":
        return _cs_edge(rng)
    if name == "skew":
        R = rng.normal(size=(3, 10, 10))
        return 20.0 * (R - np.swapaxes(R, 1, 2)), rng.normal(size=(3, 10, 3)), np.full(3, 0.2)
    if name == "stiff":
        A = []
        for _ in range(3):
            Q, _r = np.linalg.qr(rng.normal(size=(8, 8)))
            A.append(Q @ np.diag(-10.0 ** np.linspace(-1.0, 3.5, 8)) @ Q.T)
        return np.array(A), rng.normal(size=(3, 8, 2)), np.full(3, 0.1)
    if name == "be":
        return rng.normal(size=(3, 6, 6)) * 3.0, rng.normal(size=(3, 6, 5)), _ts(rng, 3)
    raise KeyError(name)


def main():
    out = {}
    for pos, name in enumerate(FAMILIES):
        A, B, Ts = inputs(name, np.random.default_rng(4100 + pos))
        T = [truth(a, b, t) for a, b, t in zip(A, B, Ts)]
        out[name + ".A"] = A; out[name + ".Ts"] = Ts
        out[name + ".Ad"] = np.array([t[0] for t in T]); out[name + ".Bd"] = np.array([t[1] for t in T]).reshape(B.shape)
        if name == "be":
            out[name + ".B"], out[name + ".Be"] = B[:, :, :2].copy(), B[:, :, 2:].copy()
        else:
            out[name + ".B"] = B
        print(name, A.shape, B.shape, flush=True)
    path = os.path.join(HERE, "c2d_truth.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
