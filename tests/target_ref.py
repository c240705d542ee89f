"""TEST INFRASTRUCTURE -- what tests/test_lmpc_target_gpu.py and tests/test_emu_target.py share: the 60-digit truths of
tests/golden/target_truth.npz (tests/golden/make_target_golden.py), the families, and the bound the target-map kernel
(libmpc_amd/csrc/target_kernels.hip) is held to.

The bound, element-wise against the truth T* (map_u and map_x, each with its own magnitude), u = 2^-52, nk = 2 nx + nu + ny the order of the
KKT matrix K and cond = |K|_inf |K^-1|_inf from the 60-digit inverse:

    |T - T*| <= C nk u cond max|T*|

C is not taken from the kernel: `restate` below is a float64 numpy restatement of the kernel's elimination ([K | rhs] with partial pivoting --
the largest magnitude, the lowest row among equals --, rows swapped across the augmented matrix, reciprocal pivots, back-substitution), and C is
8 times the worst ratio error / (nk u cond max|truth|) that the restatement reaches over the families (the rule of tests/dare_ref.py).  The
restatement's ratios, max(map_u, map_x) per family (python tests/target_ref.py prints them):

    shape_1_1_1_1      map_u  0.05935   map_x  0.00431   cond 4.638e+01
    shape_2_1_1_1      map_u  0.15435   map_x  0.09144   cond 3.071e+00
    shape_3_2_1_2      map_u  0.01364   map_x  0.00759   cond 1.711e+02
    shape_4_2_2_2      map_u  0.01676   map_x  0.02712   cond 1.537e+02
    shape_12_4_4_4     map_u  0.02381   map_x  0.02419   cond 4.026e+01
    shape_2_3_2_2      map_u  0.03171   map_x  0.07402   cond 1.792e+02
    shape_5_4_2_2      map_u  0.04530   map_x  0.10829   cond 4.322e+00
    shape_16_8_3_5     map_u  0.00219   map_x  0.00251   cond 8.035e+01
    shape_24_6_3_5     map_u  0.00666   map_x  0.00574   cond 1.416e+01
    shape_30_4_2_3     map_u  0.00325   map_x  0.00325   cond 3.151e+01
    chain              map_u  0.00042   map_x  0.00000   cond 1.000e+02
    rho_0999           map_u  0.01181   map_x  0.02041   cond 3.254e+02
    quadrotor          map_u  0.00027   map_x  0.00020   cond 1.524e+01
    limit              map_u  0.00577   map_x  0.00576   cond 1.361e+01

The worst is a 2-state instance with cond = 3: the bound's cond factor is nearly 1 there, and elimination loses its usual digit or so.
C = 8 x 0.15435 = 1.2348.
"""
import os

import numpy as np

U = 2.0 ** -52
C_BOUND = 8 * 0.15435
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_truth.npz")
SQUARE = ["shape_%d_%d_%d_%d" % s for s in ((1, 1, 1, 1), (2, 1, 1, 1), (3, 2, 1, 2), (4, 2, 2, 2), (12, 4, 4, 4))]
WIDE = ["shape_%d_%d_%d_%d" % s for s in ((2, 3, 2, 2), (5, 4, 2, 2), (16, 8, 3, 5))]
LARGE = ["shape_24_6_3_5", "shape_30_4_2_3"]             # more than 64 augmented columns; more than 64 rows
SPECIAL = ["chain", "rho_0999", "quadrotor"]
LIMIT = ["limit"]                                         # (58, 8, 4, 8): 160 512 bytes of LDS
FAMILIES = SQUARE + WIDE + LARGE + SPECIAL + LIMIT

_cache = {}


def case(name):
    """A [k, nx, nx], B [k, nx, nu], Bd [k, nx, ndu], C [k, ny, nx], Dd [k, ny, ndu], map_u [k, nu, nrhs], map_x [k, nx, nrhs], cond [k] of a
    family, row-major, read-only"""
    if not _cache:
        with np.load(GOLDEN) as z:
            for k in z.files:
                fam, key = k.rsplit(".", 1)
                _cache.setdefault(fam, {})[key] = z[k]
        for c in _cache.values():
            for a in c.values():
                a.setflags(write=False)
    return _cache[name]


def model(name):
    c = case(name)
    return c["A"], c["B"], c["Bd"], c["C"], c["Dd"]


def dims(name):
    c = case(name)
    return c["A"].shape[1], c["B"].shape[2], c["Bd"].shape[2], c["C"].shape[1]


def ratios(Tu, Tx, name):
    """worst |error| / (nk u cond max|truth|) over the instances, of map_u and of map_x (a non-finite entry gives inf)"""
    c = case(name)
    nx, nu, ndu, ny = dims(name)
    nk = 2 * nx + nu + ny

    def one(a, t):
        k = t.shape[0]
        err = np.abs(a - t).reshape(k, -1)
        err = np.where(np.isfinite(err), err, np.inf)
        return float((err.max(axis=1) / (nk * U * c["cond"] * np.abs(t).reshape(k, -1).max(axis=1))).max())
    return one(Tu, c["map_u"]), one(Tx, c["map_x"])


def check_family(name, Tu, Tx, where=""):
    """the accuracy check of one family; prints and returns the worst error / bound"""
    c = case(name)
    assert Tu.shape == c["map_u"].shape and Tx.shape == c["map_x"].shape, (name, Tu.shape, Tx.shape)
    ru, rx = ratios(Tu, Tx, name)
    print("target %s%s: worst error / bound: map_u %.4f, map_x %.4f" % (name, where, ru / C_BOUND, rx / C_BOUND))
    assert ru <= C_BOUND and rx <= C_BOUND, (name, ru, rx, C_BOUND)
    return max(ru, rx) / C_BOUND


def kkt(A, B, Bd, C, Dd):
    """(K, rhs) of one instance in float64 as the kernel lays them out: unknowns [xs; us; lambda], columns [r | dhat | ubar]"""
    nx, nu = B.shape
    ndu, ny = Bd.shape[1], C.shape[0]
    nz, nk, nrhs = nx + nu, 2 * nx + nu + ny, ny + ndu + nu
    S = np.zeros((nx + ny, nz))
    S[:nx, :nx] = np.eye(nx) - A; S[:nx, nx:] = -B; S[nx:, :nx] = C
    K = np.zeros((nk, nk))
    K[nx:nz, nx:nz] = np.eye(nu); K[:nz, nz:] = S.T; K[nz:, :nz] = S
    R = np.zeros((nk, nrhs))
    R[nz + nx:, :ny] = np.eye(ny)
    R[nz:nz + nx, ny:ny + ndu] = Bd; R[nz + nx:, ny:ny + ndu] = -Dd
    R[nx:nz, ny + ndu:] = np.eye(nu)
    return K, R


def restate(A, B, Bd, C, Dd):
    """one instance, float64: (map_u [nu, nrhs], map_x [nx, nrhs], flag) by the kernel's elimination"""
    nx, nu = B.shape
    K, R = kkt(A, B, Bd, C, Dd)
    nk, nrhs = R.shape
    nan = (np.full((nu, nrhs), np.nan), np.full((nx, nrhs), np.nan), 1)
    M = np.concatenate([K, R], axis=1)
    with np.errstate(all="ignore"):
        for k in range(nk):
            col = np.abs(M[k:, k])
            if not np.isfinite(col).all() or not col.max() > 0.0:
                return nan
            p = k + int(np.argmax(col))              # the first of the largest: the lowest row among equals
            if p != k:
                M[[k, p]] = M[[p, k]]
            lfac = M[k + 1:, k] * (1.0 / M[k, k])
            M[k + 1:, k + 1:] -= np.outer(lfac, M[k, k + 1:])
        X = M[:, nk:]
        for i in range(nk - 1, -1, -1):
            v = X[i].copy()
            for j in range(i + 1, nk):               # the kernel's order: one subtraction per column, ascending
                v -= M[i, j] * X[j]
            X[i] = v / M[i, i]
    if not np.isfinite(X[:nx + nu]).all():
        return nan
    return X[nx:nx + nu].copy(), X[:nx].copy(), 0


def numpy_maps(A, B, Bd, C, Dd):
    """(map_u, map_x) of a batch by numpy.linalg.solve per instance: the host's way, for yardsticks and timings"""
    Tu, Tx = [], []
    for i in range(A.shape[0]):
        K, R = kkt(A[i], B[i], Bd[i], C[i], Dd[i])
        Z = np.linalg.solve(K, R)
        nx, nu = B[i].shape
        Tu.append(Z[nx:nx + nu]); Tx.append(Z[:nx])
    return np.stack(Tu), np.stack(Tx)


def restatement_ratios():
    """{family: (ratio of map_u, ratio of map_x)} of the restatement against the truths"""
    out = {}
    for name in FAMILIES:
        A, B, Bd, C, Dd = model(name)
        sols = [restate(A[i], B[i], Bd[i], C[i], Dd[i]) for i in range(A.shape[0])]
        assert all(s[2] == 0 for s in sols), name
        out[name] = ratios(np.stack([s[0] for s in sols]), np.stack([s[1] for s in sols]), name)
    return out


if __name__ == "__main__":
    r = restatement_ratios()
    for name, (ru, rx) in r.items():
        print("    %-18s map_u %8.5f   map_x %8.5f   cond %9.3e" % (name, ru, rx, case(name)["cond"].max()))
    worst = max(max(v) for v in r.values())
    print("worst %.5f -> C = %.4f" % (worst, 8 * worst))
