"""Reference for the model sensitivities of a solved batch, numpy only: gradients of a loss on cmd / the input sequence with
respect to every entry of A, B, C, Bd and Dd.

Truth.gradients is the truth.  On the oracle's active set, with K = [[P, A_W'], [A_W, 0]] over the equality rows and the active rows, it solves
K [z; y] = [-q; b_W] and K [v; nu] = [p; 0], p being the cotangent on z.  For a model entry theta the builders of sens_ref.builder are rebuilt at
theta + 1 and theta - 1; with dP, dq, dA, db half the differences of the QP's data (an infinite bound does not move, a bound counts on its
active side) the gradient is g = -v' (dP z + dq + dA_W' y) - nu' (dA_W z - db_W).  The data is at most quadratic in one entry of the model, so
the unit central difference is exact (third_difference checks it).  It knows nothing of the condensed problem.

condensed_gradients restates the kernel's formulas in float64 numpy on the arrays of mpcx_lmpc_debug_get of a host-only handle, the host-built
Xq among them, and on the optimum's own sequences.

RESTATEMENT_WORST is the worst |restatement - truth| / max(1, max|truth|) over the families of tests/test_lmpc_model_sens.py (measured there, on
the CPU); the kernel is held to KERNEL_TOL = max(8 x that, 1e-12) everywhere -- a figure of the restatement against the truth, not of the kernel
(the convention of sens_ref.py)."""
import copy
import functools

import numpy as np

import param_sens_ref as P
import rate_ref as RR
import sens_ref as S

RESTATEMENT_WORST = 1.2e-10            # soft family (measured 1.18e-10); the others are at 9e-13 and below
KERNEL_TOL = max(8.0 * RESTATEMENT_WORST, 1e-12)
SKIP_CAP = S.SKIP_CAP

MODEL = ("A", "B", "C", "Bd", "Dd")
G_STATE, G_OUTPUT, G_SCALAR, G_RATE, G_LINEAR = range(5)


# ---------------------------------------------------------------------------------------------
# families: those of sens_ref, "refs" of param_sens_ref, three at the row-tile edge of the product Xq q (nx ph = 15, 16, 17), one whose state is
# longer than half a wavefront, one with two exogenous inputs that differ from step to step
# ---------------------------------------------------------------------------------------------
EDGE = {"xrows15": (3, 2, 2, 5, 31), "xrows16": (4, 2, 2, 4, 34), "xrows17": (17, 2, 2, 1, 33)}      # nx, nu, ny, ph, seed
FAMILIES = S.FAMILIES + ("refs",) + tuple(EDGE) + ("nx33", "ndu2")


def family(name):
    if name in EDGE:
        nx, nu, ny, ph, seed = EDGE[name]
        sp = RR.rate_spec(90 + nx, nx, nu, 0, ny, ph, ph, rate=0.3, box=0.6)
        return S._batch(sp, 16, seed, 1.0, 0.5)
    if name == "nx33":
        sp = RR.rate_spec(133, 33, 1, 0, 1, 2, 2, rate=0.3, box=0.6)
        return S._batch(sp, 16, 34, 1.0, 0.5)
    if name == "ndu2":
        sp = RR.rate_spec(142, 3, 2, 2, 2, 6, 6, rate=0.3, box=0.6, output=True)
        return S._batch(sp, 20, 39, 1.0, 0.5)
    return P.family(name)


def entries(sp):
    """(matrix name, row, column) of every model entry the spec has"""
    return [(m, j, i) for m in MODEL if m in sp for j in range(sp[m].shape[0]) for i in range(sp[m].shape[1])]


def _moved(sp, m, j, i, h):
    s2 = copy.deepcopy(sp)
    s2[m][j, i] += h
    return s2


def _refs(sp, yref):
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    yR = np.tile(np.asarray(yref, float)[:, None], (1, ph)) if np.ndim(yref) == 1 else np.asarray(yref, float)
    return yR, sp.get("dmeas", np.zeros((ndu, ph)))


def _working(pb, active_lower, active_upper):
    d = pb.d
    lo = np.asarray(active_lower).astype(bool); up = np.asarray(active_upper).astype(bool)
    act = lo | up
    act[:d.neq] = False
    W = np.concatenate([np.arange(d.neq), np.nonzero(act)[0]])
    return W, lo, up


def _bW(d, W, lo, up, l0, u0b):
    bW = np.where(lo[W] & ~up[W], l0[W], u0b[W])
    bW[:d.neq] = l0[:d.neq]
    return bW


class Truth:
    """the builders of a family with every model entry plus and minus one, built once"""

    def __init__(self, sp):
        self.sp, self.pb = sp, S.builder(sp)
        self.var = {}
        for (m, j, i) in entries(sp):
            sp_p, sp_m = _moved(sp, m, j, i, 1.0), _moved(sp, m, j, i, -1.0)
            pb_p, pb_m = S.builder(sp_p), S.builder(sp_m)
            self.var[m, j, i] = (sp_p, pb_p, sp_m, pb_m, 0.5 * (pb_p.P - pb_m.P), 0.5 * (np.asarray(pb_p.A) - np.asarray(pb_m.A)))

    def gradients(self, x0, u0, yref, active_lower, active_upper, seed_cmd=None, seed_input=None):
        """dict(A, B, C (, Bd, Dd), residual, full_rank, z)"""
        sp, pb = self.sp, self.pb
        nx, nu, ndu, ny, ph, ch = sp["dims"]
        d = pb.d
        yR, dM = _refs(sp, yref)
        x0 = np.asarray(x0, float); u0 = np.asarray(u0, float)
        q0, l0, u0b = S._qlu(pb, sp, x0, u0, yR, dM)
        W, lo, up = _working(pb, active_lower, active_upper)
        bW = _bW(d, W, lo, up, l0, u0b)
        n = pb.P.shape[0]
        AW = np.asarray(pb.A)[W]
        K = np.block([[pb.P, AW.T], [AW, np.zeros((len(W), len(W)))]])
        p = P.scatter_seed(d, nx, nu, ph, seed_cmd, seed_input, n)
        rhs = np.stack([np.concatenate([-q0, bW]), np.concatenate([p, np.zeros(len(W))])], axis=1)
        sol = np.linalg.lstsq(K, rhs, rcond=None)[0]
        residual = float(np.abs(K @ sol - rhs).max())
        full_rank = np.linalg.matrix_rank(np.vstack([pb.P, AW])) == n
        z, y, v, nu_ = sol[:n, 0], sol[n:, 0], sol[:n, 1], sol[n:, 1]
        out = {m: np.zeros(sp[m].shape) for m in MODEL if m in sp}
        for (m, j, i), (sp_p, pb_p, sp_m, pb_m, dP, dA) in self.var.items():
            qp, lp, up_ = S._qlu(pb_p, sp_p, x0, u0, yR, dM)
            qm, lm, um_ = S._qlu(pb_m, sp_m, x0, u0, yR, dM)
            dq = 0.5 * (qp - qm)
            dl, du = 0.5 * S._diff(lp, lm), 0.5 * S._diff(up_, um_)
            db = np.where(lo[W] & ~up[W], dl[W], du[W])
            db[:d.neq] = dl[:d.neq]
            dAW = dA[W]
            out[m][j, i] = -v @ (dP @ z + dq + dAW.T @ y) - nu_ @ (dAW @ z - db)
        out.update(residual=residual, full_rank=bool(full_rank), z=z)
        return out


def third_difference(sp, m, j, i, x0, u0, yref):
    """the largest third difference of the QP's data (P, q, the constraint matrix, the finite bounds) at unit steps of one model entry, relative to
    the data's size: zero up to rounding where the data is at most quadratic in the entry"""
    yR, dM = _refs(sp, yref)
    data = []
    for k in (-1.0, 0.0, 1.0, 2.0):
        s2 = _moved(sp, m, j, i, k)
        pb = S.builder(s2)
        q, l, u = S._qlu(pb, s2, np.asarray(x0, float), np.asarray(u0, float), yR, dM)
        fin = lambda b: np.where(np.isfinite(b), b, 0.0)
        data.append(np.concatenate([np.asarray(pb.P).ravel(), q, np.asarray(pb.A).ravel(), fin(l), fin(u)]))
    t = data[3] - 3.0 * data[2] + 3.0 * data[1] - data[0]
    return float(np.abs(t).max() / max(1.0, max(np.abs(x).max() for x in data)))


def perturbed_input(sp, x0, u0, yref, active_lower, active_upper, m, j, i, h):
    """the input sequence [(ph + 1) x nu] of the KKT solution on the same active set with model entry (m, j, i) moved by h"""
    s2 = _moved(sp, m, j, i, h)
    pb = S.builder(s2)
    nx, nu, ndu, ny, ph, ch = s2["dims"]
    d = pb.d
    yR, dM = _refs(s2, yref)
    q0, l0, u0b = S._qlu(pb, s2, np.asarray(x0, float), np.asarray(u0, float), yR, dM)
    W, lo, up = _working(pb, active_lower, active_upper)
    bW = _bW(d, W, lo, up, l0, u0b)
    AW = np.asarray(pb.A)[W]
    K = np.block([[pb.P, AW.T], [AW, np.zeros((len(W), len(W)))]])
    z = np.linalg.lstsq(K, np.concatenate([-q0, bW]), rcond=None)[0][:pb.P.shape[0]]
    return np.stack([z[min(k + 1, ph) * d.na + nx:(min(k + 1, ph) + 1) * d.na] for k in range(ph + 1)])


# ---------------------------------------------------------------------------------------------
# the kernel's formulas on the product's own arrays
# ---------------------------------------------------------------------------------------------
def arrays(c):
    """what condensed_gradients and the emulator runner read of a controller (a host-only handle serves)"""
    a = S.arrays(c)
    nx, nu, ny, ph, ldg = a["nx"], a["nu"], a["ny"], a["ph"], a["ldg"]
    ndu = a["ndu"] = c.ndu
    rows16 = (nx * ph + 15) // 16 * 16
    a["Xq"] = c.debug_get("Xq").reshape(a["nz"], rows16).T[:nx * ph]                  # column-major [rows16 x nz]
    a["m_rows"] = c.info()["m_ref"]
    model = c.debug_get("model")                                                      # A | B | C | Bd | Dd, column-major
    o = 0
    for n, r, k in (("A", nx, nx), ("B", nx, nu), ("C", ny, nx), ("Bd", nx, ndu), ("Dd", ny, ndu)):
        a[n] = model[o:o + r * k].reshape(k, r).T.copy()
        o += r * k
    a["Wy"] = c.debug_get("wOutput").reshape(ph + 1, ny).T                            # internal columns: stage i
    a["Wu"] = c.debug_get("wU").reshape(ph + 1, nu).T
    a["Wdu"] = c.debug_get("wDeltaU").reshape(ph, nu).T
    sc = c.debug_get("scalar")                                                        # sX | row c: Fx(c, :), Fu(c, :)
    a["sX"] = sc[:nx]
    a["sU"] = c.debug_get("sU")
    nc = a["nc"] = (len(sc) - nx) // (nx + nu)
    F = sc[nx:].reshape(nc, nx + nu)
    a["Fx"], a["Fu"] = F[:, :nx], F[:, nx:]
    for n in ("g_kind", "g_step", "g_comp"):
        a[n] = c.debug_get(n).astype(int)
    a["g_soft"], a["lg0"], a["ug0"] = c.debug_get("g_soft"), c.debug_get("lg0"), c.debug_get("ug0")
    t = c.debug_get("terminal")
    a["terminal"] = None
    if len(t):
        a["terminal"] = (t[:nx * nx].reshape(nx, nx).T, t[nx * nx:nx * nx + nx], t[nx * nx + nx:].reshape(ny + ndu, nx).T)
    return a


def xq_numpy(sp, blk):
    """d (states of the steps 1 .. ph) / d w, [nx ph x nz], by rolling the model out"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    nz = (max(blk[1:]) + 1) * nu
    out = np.zeros((nx * ph, nz))
    for q in range(nz):
        w = np.zeros(nz); w[q] = 1.0
        x = np.zeros(nx)
        for i in range(1, ph + 1):
            x = sp["A"] @ x + sp["B"] @ w[blk[i] * nu:(blk[i] + 1) * nu]
            out[(i - 1) * nx:i * nx, q] = x
    return out


def rollout(sp, x0, inp, dmeas=None):
    """seq_state [(ph + 1) x nx] and seq_output [(ph + 1) x ny] of the input sequence `inp` [(ph + 1) x nu] as the solve writes them"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    dM = sp.get("dmeas", np.zeros((ndu, ph))) if dmeas is None else dmeas
    Bd = sp.get("Bd", np.zeros((nx, ndu))); Dd = sp.get("Dd", np.zeros((ny, ndu)))
    x = np.asarray(x0, float)
    X = np.zeros((ph + 1, nx)); Yo = np.zeros((ph + 1, ny))
    for i in range(ph + 1):
        X[i] = x
        Yo[i] = sp["C"] @ x + Dd @ dM[:, max(i - 1, 0)]
        if i < ph:
            x = sp["A"] @ x + sp["B"] @ inp[i] + Bd @ dM[:, i]
    return X, Yo


def condensed_gradients(a, active_lower, active_upper, u0, seq_state, seq_output, seq_input, yref, uref, duref, dmeas, seed_cmd=None, seed_input=None):
    """dict(A, B, C, Bd, Dd, n, dependent); yref [ny x ph], uref, duref [nu x ph], dmeas [ndu x ph] are the references of the instance,
    column = step"""
    nz, ldz, nx, nu, ny, ndu, ph, blk = a["nz"], a["ldz"], a["nx"], a["nu"], a["ny"], a["ndu"], a["ph"], a["blk"]
    Am, Bm, Cm = a["A"], a["B"], a["C"]
    lo = np.zeros(a["m_rows"], bool); up = np.zeros(a["m_rows"], bool)
    lo[:len(active_lower)] = np.asarray(active_lower).astype(bool)[:a["m_rows"]]; up[:len(active_upper)] = np.asarray(active_upper).astype(bool)[:a["m_rows"]]
    A = S.working_set(a, lo | up)
    p = np.zeros(nz)
    si = np.zeros((ph + 1, nu)) if seed_input is None else np.array(seed_input, float)
    if seed_cmd is not None:
        si[0] += seed_cmd
    for i in range(ph + 1):
        b = blk[min(i + 1, ph)]
        p[b * nu:(b + 1) * nu] += si[i]
    Y = a["Y"]
    q = Y[:nz, :nz] @ p
    out = dict(n=len(A), dependent=False)
    shapes = dict(A=(nx, nx), B=(nx, nu), C=(ny, nx), Bd=(nx, ndu), Dd=(ny, ndu))
    # the optimum's trajectory: v_0 = lastU, v_i = row i - 1 of the sequence
    X, Yo = np.asarray(seq_state, float), np.asarray(seq_output, float)
    v = np.vstack([np.asarray(u0, float)] + [seq_input[i - 1] for i in range(1, ph + 1)])
    # the cost's own stage gradients and its condensed gradient at the optimum, one backward pass
    e = np.zeros((ph + 1, ny))
    for i in range(1, ph + 1):
        e[i] = a["Wy"][:, i] * (Yo[i] - yref[:, i - 1])
    eT = np.zeros(nx)
    Pm = None
    if a["terminal"] is not None:
        Pm, xT0, Tx = a["terminal"]
        xT = xT0 + Tx[:, :ny] @ yref[:, ph - 1] + (Tx[:, ny:] @ dmeas[:, ph - 1] if ndu else 0.0)
        eT = Pm @ (X[ph] - xT)
    r = np.stack([a["Wdu"][:, i] * (v[i + 1] - v[i] - duref[:, max(i - 1, 0)]) for i in range(ph)])
    grad = np.zeros(nz)
    c = np.zeros(nx)
    for i in range(ph, 0, -1):
        c = Cm.T @ e[i] + Am.T @ c + (eT if i == ph else 0.0)
        gv = Bm.T @ c + a["Wu"][:, i] * (v[i] - uref[:, i - 1]) + r[i - 1] - (r[i] if i < ph else 0.0)
        grad[blk[i] * nu:(blk[i] + 1) * nu] += gv
    mu = np.zeros(0); lam = np.zeros(0)
    if len(A):
        Sm = Y[np.ix_(A, A)]
        try:
            L = np.linalg.cholesky(Sm)
            out["dependent"] = bool((np.diag(L) ** 2 <= 1e-11 * np.diag(Sm)).any())
        except np.linalg.LinAlgError:
            out["dependent"] = True
        if not out["dependent"]:
            mu = np.linalg.solve(Sm, Y[A][:, :nz] @ p)
            q = q - Y[:nz][:, A] @ mu
            # the optimum's multipliers: stationarity on the hard rows, a soft row's own relation (its 1 / weight is on S's diagonal)
            rhs = -(Y[A][:, :nz] @ grad)
            for k, eidx in enumerate(A):
                if eidx >= ldz and a["g_soft"][eidx - ldz] > 0.0:
                    rr = eidx - ldz
                    rhs[k] += row_value(a, rr, X, Yo, v) - (a["ug0"][rr] if up[a["g_refrow"][rr]] else a["lg0"][rr])
            lam = np.linalg.solve(Sm, rhs)
    if out["dependent"]:
        for m, shp in shapes.items():
            out[m] = np.full(shp, np.nan)
        return out
    dX = np.vstack([np.zeros(nx), (a["Xq"] @ q).reshape(ph, nx)])
    dv = np.vstack([np.zeros(nu)] + [q[blk[i] * nu:(blk[i] + 1) * nu] for i in range(1, ph + 1)])
    # stage gradients with the rows' multipliers, the optimum's (lam) and the adjoint system's (mu), and the two costates
    o = e.copy()
    do = np.stack([a["Wy"][:, i] * (Cm @ dX[i]) if i else np.zeros(ny) for i in range(ph + 1)])
    gx = np.zeros((ph + 1, nx)); dgx = np.zeros((ph + 1, nx))
    for k, eidx in enumerate(A):
        if eidx < ldz:
            continue
        rr = eidx - ldz
        kind, st, cp = a["g_kind"][rr], a["g_step"][rr], a["g_comp"][rr]
        if st < 1:
            continue
        if kind == G_OUTPUT:
            o[st, cp] += lam[k]; do[st, cp] += mu[k]
        elif kind == G_STATE:
            gx[st, cp] += lam[k]; dgx[st, cp] += mu[k]
        elif kind == G_SCALAR:
            gx[st] += lam[k] * a["sX"]; dgx[st] += mu[k] * a["sX"]
        elif kind == G_LINEAR:
            gx[st] += lam[k] * a["Fx"][cp]; dgx[st] += mu[k] * a["Fx"][cp]
    pi = np.zeros((ph + 2, nx)); eta = np.zeros((ph + 2, nx))
    for i in range(ph, 0, -1):
        pi[i] = Cm.T @ o[i] + gx[i] + Am.T @ pi[i + 1] + (eT if i == ph else 0.0)
        eta[i] = Cm.T @ do[i] + dgx[i] + Am.T @ eta[i + 1] + (Pm @ dX[ph] if (i == ph and Pm is not None) else 0.0)
    out["A"] = -sum(np.outer(pi[i], dX[i - 1]) + np.outer(eta[i], X[i - 1]) for i in range(1, ph + 1))
    out["B"] = -sum(np.outer(pi[i], dv[i]) + np.outer(eta[i], v[i]) for i in range(1, ph + 1))
    out["C"] = -sum(np.outer(o[i], dX[i]) + np.outer(do[i], X[i]) for i in range(1, ph + 1))
    out["Bd"] = -sum(np.outer(eta[i], dmeas[:, i - 1]) for i in range(1, ph + 1)) if ndu else np.zeros((nx, 0))
    out["Dd"] = -sum(np.outer(do[i], dmeas[:, i - 1]) for i in range(1, ph + 1)) if ndu else np.zeros((ny, 0))
    out["lam"], out["mu"] = lam, mu
    return out


def row_value(a, rr, X, Yo, v):
    """the value of general row rr at the optimum, from its sequences"""
    kind, st, cp = a["g_kind"][rr], a["g_step"][rr], a["g_comp"][rr]
    if kind == G_STATE:
        return X[st, cp]
    if kind == G_OUTPUT:
        return Yo[st, cp]
    if kind == G_SCALAR:
        return a["sX"] @ X[st] + a["sU"] @ v[st]
    if kind == G_LINEAR:
        return a["Fx"][cp] @ X[st] + a["Fu"][cp] @ v[st]
    return v[st, cp] - v[st - 1, cp]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's solve of a family and the truth for one random seed pair per usable instance: dict(sp, x0, u0, yref, res, truth [B] (None:
    unusable), seed_cmd, seed_input, tr)"""
    if name in P.FAMILIES:                       # the same controller and batch: the oracle's solve is shared with tests/param_sens_ref.py
        Rp = P.reference(name)
        sp, x0, u0, yref, res = (Rp[k] for k in ("sp", "x0", "u0", "yref", "res"))
    else:
        sp, x0, u0, yref = family(name)
        res = S.solve_batch(sp, x0, u0, yref)
    tr = Truth(sp)
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    rg = np.random.default_rng(19)
    B = len(x0)
    sc, sq = rg.normal(size=(B, nu)), rg.normal(size=(B, ph + 1, nu))
    truth = []
    for b in range(B):
        t = tr.gradients(x0[b], u0[b], yref[b], res["active_lower"][b], res["active_upper"][b], sc[b], sq[b]) if S.usable(res, b) else None
        truth.append(t if t is not None and S.good(t) else None)
    return dict(sp=sp, x0=x0, u0=u0, yref=yref, res=res, truth=truth, seed_cmd=sc, seed_input=sq, tr=tr)


def compare(t, g):
    """worst |g - truth| / max(1, max|truth|) over the matrices the truth has"""
    names = [m for m in MODEL if m in t]
    scale = max(1.0, max(np.abs(t[m]).max(initial=0.0) for m in names))
    return max(np.abs(np.asarray(g[m]) - t[m]).max(initial=0.0) for m in names) / scale
