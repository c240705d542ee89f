"""The extended Kalman filter of the observed NLMPC loop (include/mpcx/nlmpc_ekf.hpp) restated in numpy, with the tolerances the
kernel is held to.  Shared by test_emu_nlmpc_ekf.py, test_nlmpc_ekf.py and test_nlmpc_ekf_gpu.py.

Contract (Phi: the plant step of nlmpc_plant_ref.py without noise -- its state functions are imported, not restated):
    x_{k+1}  = Phi(x_k, cmd_k, p_plant) + w_k          y_{k+1} = Cm x_{k+1} + v_k
    xhat-    = Phi(xhat_k, cmd_k, p_ctrl)
    F[:, j]  = (Phi(xhat_k + h_j e_j) - Phi(xhat_k - h_j e_j)) / (x+_j - x-_j),   h_j = 2^-17 max(1, |xhat_k,j|)   (the divisor: the perturbed values as stored)
    P-       = F P_k F' + Q;   S = Cm P- Cm' + R;   K = P- Cm' S^-1 (Cholesky of S, written out below so that it also runs in np.longdouble)
    xhat_{k+1} = xhat- + K (y_{k+1} - Cm xhat-);   P_{k+1} = sym((I - K Cm) P- (I - K Cm)' + K R K')
    a pivot of S not > 0 or not finite: xhat_{k+1} = xhat-, P_{k+1} = sym(P-), flag 1

Tolerances.  The kernel and this module are two float64 roundings of one exact computation: they differ in the order of the sums and in which
multiply-add pairs are fused, so each sits about as far from the exact value as this module's float64 run sits from its own np.longdouble run,
and their distance from each other is a small multiple of that.  TOL[model] = (xhat, P) is 8 x the largest ONE-STEP difference between the two
runs over the tests' own inputs -- `cases()` below: every tick of every variant, each step taken from the float64 run's xhat_k, P_k -- xhat
relative to max(1, |xhat|) per component, P relative to max |P| of the instance.  The dominant term is the finite difference's amplification
2^-52 / 2^-17 = 2^-35 = 3e-11 of the round-off of Phi.  `python tests/nlmpc_ekf_ref.py` prints the measurement; on x86-64 (80-bit long double):

    model      xhat        P
    vanderpol  2.32e-12    4.16e-11
    ugv        1.11e-12    7.51e-12
    osc6       1.96e-12    1.92e-11
    osc8       1.88e-12    2.08e-11

(MEASURED holds these with the last digit rounded up; TOL is 8 x MEASURED.)"""
import numpy as np

import nlmpc_plant_ref as P_

MODELS = dict(P_.MODELS)
MODELS["osc8"] = (P_._osc(8), True)
DEFAULT_PARAMS = dict(P_.DEFAULT_PARAMS)
DEFAULT_PARAMS["osc8"] = [1.0, 0.1]
DIMS = {"vanderpol": (2, 1), "ugv": (4, 2), "osc6": (12, 6), "osc8": (16, 8)}
MEASURED = {"vanderpol": (2.33e-12, 4.17e-11), "ugv": (1.12e-12, 7.52e-12), "osc6": (1.97e-12, 1.93e-11), "osc8": (1.89e-12, 2.09e-11)}
TOL = {k: (8 * a, 8 * b) for k, (a, b) in MEASURED.items()}
REL = 2.0 ** -17


def meas_matrix(model):
    """the tests' measurement matrices: Van der Pol [0 1]; the UGV's two positions; the oscillators' q_i = x[2 i]"""
    nx = DIMS[model][0]
    if model == "vanderpol":
        return np.array([[0.0, 1.0]])
    if model == "ugv":
        return np.eye(4)[:2]
    C = np.zeros((nx // 2, nx))
    C[np.arange(nx // 2), 2 * np.arange(nx // 2)] = 1.0
    return C


def phi(model, x, u, p, Ts, substeps=1, dtype=np.float64):
    """the noise-free step, [B, nx], in `dtype`"""
    f, continuous = MODELS[model]
    x = np.array(x, dtype=dtype); u = np.asarray(u, dtype=dtype)
    p = np.atleast_2d(np.asarray(p, dtype=dtype))
    p = np.broadcast_to(p, (x.shape[0], p.shape[1]))
    if not continuous:
        return f(x, u, p)[0]
    h = dtype(Ts) / dtype(substeps)
    for _ in range(substeps):
        x = x + h * f(x, u, p)[0]
    return x


def cholesky(S):
    """(L, ok): lower factor of one matrix, right-looking, the pivot tested before the square root and before any division"""
    n = S.shape[0]
    L = np.array(S)
    for k in range(n):
        piv = L[k, k]
        if not (piv > 0 and np.isfinite(piv)):
            return L, False
        d = np.sqrt(piv)
        L[k, k] = d
        L[k + 1:, k] = L[k + 1:, k] / d
        for r in range(k + 1, n):
            L[r, k + 1:r + 1] = L[r, k + 1:r + 1] - L[r, k] * L[k + 1:r + 1, k]
    return np.tril(L), True


def chol_solve(L, Bm):
    """X with L L' X = Bm, by substitution"""
    n = L.shape[0]
    X = np.array(Bm)
    for i in range(n):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def jacobian(model, xhat, u, p, Ts, substeps, dtype=np.float64):
    xhat = np.asarray(xhat, dtype=dtype)
    B, nx = xhat.shape
    F = np.empty((B, nx, nx), dtype=dtype)
    for j in range(nx):
        h = dtype(REL) * np.maximum(dtype(1), np.abs(xhat[:, j]))
        xp = xhat.copy(); xm = xhat.copy()
        xp[:, j] = xhat[:, j] + h; xm[:, j] = xhat[:, j] - h
        F[:, :, j] = (phi(model, xp, u, p, Ts, substeps, dtype) - phi(model, xm, u, p, Ts, substeps, dtype)) / (xp[:, j] - xm[:, j])[:, None]
    return F


def ekf_step(model, xhat, P, u, y, p, Ts, substeps, Cm, Q, R, dtype=np.float64):
    """(xhat_next [B, nx], P_next [B, nx, nx], flags [B]); P is a stack of symmetric matrices, Cm None = the identity"""
    xhat = np.asarray(xhat, dtype=dtype); P = np.asarray(P, dtype=dtype); y = np.asarray(y, dtype=dtype)
    B, nx = xhat.shape
    Cm = np.eye(nx, dtype=dtype) if Cm is None else np.asarray(Cm, dtype=dtype)
    Q = np.asarray(Q, dtype=dtype); R = np.asarray(R, dtype=dtype)
    xm = phi(model, xhat, u, p, Ts, substeps, dtype)
    F = jacobian(model, xhat, u, p, Ts, substeps, dtype)
    xn = np.empty_like(xm); Pn = np.empty_like(P); flags = np.zeros(B, dtype=np.int32)
    I = np.eye(nx, dtype=dtype)
    for b in range(B):
        Pm = F[b] @ P[b] @ F[b].T + Q
        S = Cm @ Pm @ Cm.T + R
        L, ok = cholesky(S)
        if not ok:
            xn[b] = xm[b]; Pn[b] = (Pm + Pm.T) / 2; flags[b] = 1
            continue
        K = chol_solve(L, Cm @ Pm).T
        xn[b] = xm[b] + K @ (y[b] - Cm @ xm[b])
        A = I - K @ Cm
        Pj = A @ Pm @ A.T + K @ R @ K.T
        Pn[b] = (Pj + Pj.T) / 2
    return xn, Pn, flags


def advance(model, x, xhat, P, cmd, p_plant, p_ctrl, Ts, substeps, Cm, Q, R, w=None, v=None, dtype=np.float64):
    """one tick of the observed loop's advance step: (x_next, y, xhat_next, P_next, flags)"""
    xn = phi(model, x, cmd, p_plant, Ts, substeps, dtype)
    if w is not None:
        xn = xn + np.asarray(w, dtype=dtype)
    C = np.eye(xn.shape[1], dtype=dtype) if Cm is None else np.asarray(Cm, dtype=dtype)
    y = xn @ C.T
    if v is not None:
        y = y + np.asarray(v, dtype=dtype)
    xh, Pn, fl = ekf_step(model, xhat, P, cmd, y, p_ctrl, Ts, substeps, Cm, Q, R, dtype)
    return xn, y, xh, Pn, fl


def rel_x(a, b):
    """largest difference of two estimates relative to max(1, |xhat|)"""
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def rel_P(a, b):
    """largest difference of two covariance stacks relative to max |P| of each instance"""
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    B = b.shape[0]
    scale = np.abs(b).reshape(B, -1).max(axis=1)
    return float((np.abs(a - b).reshape(B, -1).max(axis=1) / np.maximum(scale, np.finfo(np.float64).tiny)).max())


# ---- the tests' own inputs --------------------------------------------------------------------------------------------------------------
BATCH = {"vanderpol": 23, "ugv": 13, "osc6": 5, "osc8": 3}
TICKS = 3
Q_DIAG, R_DIAG, P0_DIAG = 1e-4, 1e-2, 1e-2
VARIANTS = ("", "noise", "plant", "noise+plant", "noise+full")


def cases():
    """(model, substeps, variant) of every case the tolerances are measured on and the CPU and GPU tests run"""
    out = []
    for model in ("vanderpol", "ugv", "osc6", "osc8"):
        for substeps in ((1, 4) if model == "vanderpol" else (1,)):
            for variant in VARIANTS:
                out.append((model, substeps, variant))
    return out


def inputs(model, variant, seed=41):
    """seeded inputs of a case: states and commands in the range the controllers work in; `noise`: process and measurement noise and an
    estimate that starts off the truth; `plant`: per-instance controller parameters and other ones for the plant; `full`: Cm = None, every state
    is measured (ny = nx)"""
    nx, nu = DIMS[model]
    B = BATCH[model]
    Cm = None if "full" in variant else meas_matrix(model)
    ny = nx if Cm is None else Cm.shape[0]
    rng = np.random.default_rng(seed)
    d = dict(x0=rng.uniform(-1.0, 1.0, size=(B, nx)), u0=rng.uniform(-0.5, 0.5, size=(B, nu)), cmd=rng.uniform(-0.5, 0.5, size=(TICKS, B, nu)),
             cost=rng.uniform(0.0, 10.0, size=(TICKS, B)), ints=rng.integers(-5, 200, size=(TICKS, 4, B)), ctrl=np.array(DEFAULT_PARAMS[model]),
             Cm=Cm, Q=Q_DIAG * np.eye(nx), R=R_DIAG * np.eye(ny), P0=P0_DIAG * np.eye(nx), noise=None, meas_noise=None, xhat0=None, params=None, plant=None)
    # full matrices, not multiples of the identity: a transposed or mis-strided read of any of them shows
    for key, n in (("Q", nx), ("R", ny), ("P0", nx)):
        G = rng.uniform(-1.0, 1.0, size=(n, n))
        d[key] = d[key] + 0.1 * d[key][0, 0] * (G @ G.T) / n
    if "noise" in variant:
        d["noise"] = rng.normal(scale=1e-2, size=(TICKS, B, nx))
        d["meas_noise"] = rng.normal(scale=1e-1, size=(TICKS, B, ny))
        d["xhat0"] = d["x0"] + rng.normal(scale=1e-1, size=(B, nx))
    if "plant" in variant:
        base = np.tile(d["ctrl"], (B, 1))
        d["params"] = base * (1.0 + rng.uniform(-0.1, 0.1, size=base.shape))
        d["plant"] = base * (1.0 + rng.uniform(-0.1, 0.1, size=base.shape))
        if model == "ugv":
            d["plant"][:, 8] = rng.choice([0.05, 0.1, 0.2], size=B)
    return d


def run(model, substeps, d, Ts=0.1, dtype=np.float64):
    """the reference's own trajectory of a case: lists over ticks of (x, xhat, P) with TICKS + 1 entries, y and flags with TICKS"""
    pc = d["ctrl"] if d["params"] is None else d["params"]
    pp = d["plant"] if d["plant"] is not None else pc
    x = [np.asarray(d["x0"], dtype=dtype)]
    xh = [np.asarray(d["x0"] if d["xhat0"] is None else d["xhat0"], dtype=dtype)]
    B = x[0].shape[0]
    Pk = [np.tile(np.asarray(d["P0"], dtype=dtype), (B, 1, 1))]
    ys, fl = [], []
    for k in range(d["cmd"].shape[0]):
        xn, y, xhn, Pn, f = advance(model, x[k], xh[k], Pk[k], d["cmd"][k], pp, pc, Ts, substeps, d["Cm"], d["Q"], d["R"],
                                    None if d["noise"] is None else d["noise"][k], None if d["meas_noise"] is None else d["meas_noise"][k], dtype)
        x.append(xn); xh.append(xhn); Pk.append(Pn); ys.append(y); fl.append(f)
    return x, xh, Pk, ys, fl


def measure():
    """per model: the largest one-step difference (xhat, P) between the float64 and the long-double run over cases()"""
    worst = {}
    for model, substeps, variant in cases():
        d = inputs(model, variant)
        pc = d["ctrl"] if d["params"] is None else d["params"]
        _, xh, Pk, ys, _ = run(model, substeps, d)
        ex, eP = worst.get(model, (0.0, 0.0))
        for k in range(TICKS):
            a = ekf_step(model, xh[k], Pk[k], d["cmd"][k], ys[k], pc, 0.1, substeps, d["Cm"], d["Q"], d["R"])
            b = ekf_step(model, xh[k], Pk[k], d["cmd"][k], ys[k], pc, 0.1, substeps, d["Cm"], d["Q"], d["R"], dtype=np.longdouble)
            ex = max(ex, rel_x(a[0], b[0])); eP = max(eP, rel_P(a[1], b[1]))
        worst[model] = (ex, eP)
    return worst


if __name__ == "__main__":
    for model, (ex, eP) in measure().items():
        print("%-10s xhat %.3e  P %.3e   MEASURED %.2e %.2e   TOL %.2e %.2e" % ((model, ex, eP) + MEASURED[model] + TOL[model]))
