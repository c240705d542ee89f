"""Writes tests/golden/target_truth.npz: the 60-digit truths that the target-map kernel (libmpc_amd/csrc/target_kernels.hip,
mpcx_target_map_batch) is held to, read by tests/target_ref.py for tests/test_lmpc_target_gpu.py and tests/test_emu_target.py.  Needs mpmath;
run from the repository root:

    python tests/golden/make_target_golden.py

An instance is a model A [nx, nx], B [nx, nu], Bd [nx, ndu], C [ny, nx], Dd [ny, ndu] (row-major here).  Its target for (r, dhat, ubar) is
    minimise 1/2 |us - ubar|^2   subject to   (I - A) xs - B us = Bd dhat,   C xs = r - Dd dhat
and the truth is the solution of the KKT system K [xs; us; lambda] = rhs in 60-digit arithmetic (LU with partial pivoting), K = [[W, S'], [S, 0]],
S = [[I - A, -B], [C, 0]], W = blkdiag(0, I_nu), for the nrhs = ny + ndu + nu columns of [r | dhat | ubar]; the relative residual of the system is
checked to be below 1e-50.  Stored per family: the model, map_u [k, nu, nrhs], map_x [k, nx, nrhs] and cond [k] = |K|_inf |K^-1|_inf."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "target_truth.npz")


def kkt(A, B, Bd, C, Dd):
    """(K, rhs) in float64, exactly as the entries are defined (I - A is rounded once, as the kernel rounds it)"""
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


def truth(A, B, Bd, C, Dd):
    nx, nu = B.shape
    # I - A in exact arithmetic: the truth belongs to the model, not to the kernel's rounding of 1 - a_ii
    K, R = kkt(A, B, Bd, C, Dd)
    K_ = mp.matrix(K.tolist())
    IA = mp.eye(nx) - mp.matrix(A.tolist())
    nz = nx + nu
    for i in range(nx):
        for j in range(nx):
            K_[nz + i, j] = IA[i, j]
            K_[j, nz + i] = IA[i, j]
    R_ = mp.matrix(R.tolist())
    Ki = mp.inverse(K_)                              # (LU with partial pivoting; lu_solve takes one right-hand side at a time)
    Z = Ki * R_
    res = mp.norm(K_ * Z - R_, mp.inf) / (mp.norm(K_, mp.inf) * mp.norm(Z, mp.inf))
    assert res < mp.mpf(10) ** -50, res
    cond = mp.norm(K_, mp.inf) * mp.norm(Ki, mp.inf)
    f = lambda M, r0, r1: np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(r0, r1)])
    return f(Z, nx, nz), f(Z, 0, nx), float(cond)


def random_instance(rng, nx, nu, ndu, ny, rho=0.9):
    A = rng.normal(size=(nx, nx))
    A *= rho / max(abs(np.linalg.eigvals(A)))
    return A, rng.normal(size=(nx, nu)), rng.normal(size=(nx, ndu)), rng.normal(size=(ny, nx)), rng.normal(size=(ny, ndu))


def chain():
    """an integrator chain observed through C: A = I + 0.1 N, the input at its tail, the output its head.  I - A = -0.1 N has a zero diagonal and
    rank nx - 1; the row of C makes [I - A; C] full rank"""
    n = 5
    A = np.eye(n) + 0.1 * np.diag(np.ones(n - 1), 1)
    B = np.zeros((n, 1)); B[-1, 0] = 0.1
    C = np.zeros((1, n)); C[0, 0] = 1.0
    return A, B, B.copy(), C, np.zeros((1, 1))


def quadrotor(k):
    """the quadrotor of the reference's example (numeric data, libmpc_amd/workloads.py) with outputs (x, y, z, yaw) = rows [3, 4, 5, 2] of the
    state, an input disturbance Bd = B and Dd = 0; variant k scales the dynamics as workloads.quadrotor_variant does"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from libmpc_amd.workloads import quadrotor_target_model
    Ad, Bd, _, C, Dd = quadrotor_target_model()
    Bv = Bd * (1.0 + 0.05 * k)
    return Ad, Bv, Bv.copy(), C, Dd


def main():
    rng = np.random.default_rng(20240917)
    fams = {}
    shapes = [((1, 1, 1, 1), 3), ((2, 1, 1, 1), 3), ((3, 2, 1, 2), 3), ((4, 2, 2, 2), 3),          # small and square
              ((2, 3, 2, 2), 3), ((5, 4, 2, 2), 3), ((16, 8, 3, 5), 2),                           # wide
              ((12, 4, 4, 4), 2),
              ((24, 6, 3, 5), 1),                                                                 # more than 64 augmented columns
              ((30, 4, 2, 3), 1)]                                                                 # nk > 64
    for s, count in shapes:
        fams["shape_%d_%d_%d_%d" % s] = [random_instance(rng, *s) for _ in range(count)]
    fams["limit"] = [random_instance(rng, 58, 8, 4, 8)]       # nk = 132, 132 x 152 doubles = 160 512 bytes of the 163 840 a workgroup may request
    fams["chain"] = [chain()]
    fams["rho_0999"] = [random_instance(rng, 6, 2, 2, 2, rho=0.999) for _ in range(3)]
    fams["quadrotor"] = [quadrotor(k) for k in range(2)]
    out = {}
    for name, insts in fams.items():
        sols = [truth(*i) for i in insts]
        for key, vals in zip(("A", "B", "Bd", "C", "Dd"), zip(*insts)):
            out[name + "." + key] = np.stack(vals)
        out[name + ".map_u"] = np.stack([s[0] for s in sols])
        out[name + ".map_x"] = np.stack([s[1] for s in sols])
        out[name + ".cond"] = np.array([s[2] for s in sols])
        print(name, out[name + ".A"].shape, "cond %.3e" % out[name + ".cond"].max(), "max|map_u| %.3e" % np.abs(out[name + ".map_u"]).max())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
