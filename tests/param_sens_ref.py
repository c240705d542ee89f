"""Reference for the parameter sensitivities of a solved batch, numpy only: gradients of a loss on cmd / the input sequence
with respect to OWeight, UWeight, DeltaUWeight and to every bound of the QP.

Truth.gradients is the truth.  On the oracle's active set, with K = [[P, A_W'], [A_W, 0]] over the equality rows and the active rows, it solves
K [z; y] = [-q; b_W] and K [v; nu] = [p; 0], p being the cotangent on z.  A weight entry theta gives g = -v' ((P(theta + 1) - P(theta)) z +
(q(theta + 1) - q(theta))) with the builders of sens_ref.builder rebuilt for that entry plus one -- P and q are linear in the weights, so the
unit difference is exact -- and a bound gives nu_r on its active side (the upper one where both bits are set, as sens_ref.kkt_jacobian
chooses).  It knows nothing of the condensed problem.

condensed_gradients restates the kernel's formulas in float64 numpy on the arrays of mpcx_lmpc_debug_get of a host-only handle, the host-built
Cq among them, and on the optimum's own sequences.

RESTATEMENT_WORST is the worst |restatement - truth| / max(1, max|truth|) over the families of tests/test_lmpc_param_sens.py (measured there, on
the CPU); the kernel is held to KERNEL_TOL = max(8 x that, 1e-12) everywhere -- a figure of the restatement against the truth, not of the kernel
(the convention of sens_ref.py)."""
import copy
import functools

import numpy as np

import rate_ref as RR
import sens_ref as S

RESTATEMENT_WORST = 1.6e-11            # soft family (measured 1.59e-11); the others are at 5e-13 and below
KERNEL_TOL = max(8.0 * RESTATEMENT_WORST, 1e-12)
SKIP_CAP = S.SKIP_CAP

WEIGHTS = ("OW", "UW", "DUW")


# ---------------------------------------------------------------------------------------------
# families: those of sens_ref, three at the row-tile edge of the product Cq q (ny ph = 15, 16, 17), one with per-step input references
# ---------------------------------------------------------------------------------------------
EDGE = {"rows15": (3, 2, 3, 5, 21), "rows16": (3, 2, 4, 4, 22), "rows17": (4, 2, 17, 1, 23)}      # nx, nu, ny, ph, seed
FAMILIES = S.FAMILIES + tuple(EDGE) + ("refs",)


def family(name):
    if name == "refs":                           # input and rate references that differ from step to step: the stage map of the two input terms
        sp = RR.rate_spec(81, 3, 2, 0, 2, 6, 6, rate=0.3, box=0.6)
        r = np.random.default_rng(82)
        sp["uref"] = 0.2 * r.normal(size=(2, 6)); sp["duref"] = 0.05 * r.normal(size=(2, 6))
        return S._batch(sp, 16, 24, 1.0, 0.5)
    if name in EDGE:
        nx, nu, ny, ph, seed = EDGE[name]
        sp = RR.rate_spec(70 + ny, nx, nu, 0, ny, ph, ph, rate=0.3, box=0.6)
        return S._batch(sp, 16, seed, 1.0, 0.5)
    return S.family(name)


def scatter_seed(d, nx, nu, ph, seed_cmd=None, seed_input=None, n=None):
    """the cotangent on z: row i of the sequence is the x_u block of xi_{min(i + 1, ph)}, cmd is row 0"""
    p = np.zeros(n)
    si = np.zeros((ph + 1, nu)) if seed_input is None else np.array(seed_input, float)
    if seed_cmd is not None:
        si[0] += seed_cmd
    for i in range(ph + 1):
        k = min(i + 1, ph)
        p[k * d.na + nx:(k + 1) * d.na] += si[i]
    return p


class Truth:
    """the builders of a family with every weight entry plus one, built once"""

    def __init__(self, sp):
        self.sp, self.pb = sp, S.builder(sp)
        self.var = {}
        for w in WEIGHTS:
            for j in range(sp[w].shape[0]):
                for i in range(sp[w].shape[1]):
                    s2 = copy.deepcopy(sp)
                    s2[w][j, i] += 1.0
                    pb2 = S.builder(s2)
                    self.var[w, j, i] = (s2, pb2, pb2.P - self.pb.P)

    def gradients(self, x0, u0, yref, active_lower, active_upper, seed_cmd=None, seed_input=None):
        """dict(OW [ny x ph], UW, DUW [nu x ph], lower, upper [ncon], residual, full_rank)"""
        sp, pb = self.sp, self.pb
        nx, nu, ndu, ny, ph, ch = sp["dims"]
        d = pb.d
        yR = np.tile(np.asarray(yref, float)[:, None], (1, ph)) if np.ndim(yref) == 1 else np.asarray(yref, float)
        dM = sp.get("dmeas", np.zeros((ndu, ph)))
        x0 = np.asarray(x0, float); u0 = np.asarray(u0, float)
        q0, l0, u0b = S._qlu(pb, sp, x0, u0, yR, dM)
        lo = np.asarray(active_lower).astype(bool); up = np.asarray(active_upper).astype(bool)
        act = lo | up
        act[:d.neq] = False
        W = np.concatenate([np.arange(d.neq), np.nonzero(act)[0]])
        bW = np.where(lo[W] & ~up[W], l0[W], u0b[W])
        bW[:d.neq] = l0[:d.neq]
        n = pb.P.shape[0]
        AW = pb.A[W]
        K = np.block([[pb.P, AW.T], [AW, np.zeros((len(W), len(W)))]])
        p = scatter_seed(d, nx, nu, ph, seed_cmd, seed_input, n)
        rhs = np.stack([np.concatenate([-q0, bW]), np.concatenate([p, np.zeros(len(W))])], axis=1)
        sol = np.linalg.lstsq(K, rhs, rcond=None)[0]
        residual = float(np.abs(K @ sol - rhs).max())
        full_rank = np.linalg.matrix_rank(np.vstack([pb.P, AW])) == n
        z, v, nu_ = sol[:n, 0], sol[:n, 1], sol[n:, 1]
        out = {w: np.zeros(sp[w].shape) for w in WEIGHTS}
        for (w, j, i), (s2, pb2, dP) in self.var.items():
            dq = S._qlu(pb2, s2, x0, u0, yR, dM)[0] - q0
            out[w][j, i] = -v @ (dP @ z + dq)
        gl = np.zeros(len(l0)); gu = np.zeros(len(l0))
        for k, r in enumerate(W[d.neq:]):
            if up[r]:
                gu[r] = nu_[d.neq + k]
            else:
                gl[r] = nu_[d.neq + k]
        out.update(lower=gl, upper=gu, residual=residual, full_rank=bool(full_rank), z=z)
        return out


def perturbed_input(tr, x0, u0, yref, active_lower, active_upper, w, j, i, h):
    """the input sequence [(ph + 1) x nu] of the KKT solution on the same active set with weight entry (w, j, i) moved by h"""
    sp = copy.deepcopy(tr.sp)
    sp[w][j, i] += h
    pb = S.builder(sp)
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = pb.d
    yR = np.tile(np.asarray(yref, float)[:, None], (1, ph)) if np.ndim(yref) == 1 else np.asarray(yref, float)
    dM = sp.get("dmeas", np.zeros((ndu, ph)))
    q0, l0, u0b = S._qlu(pb, sp, np.asarray(x0, float), np.asarray(u0, float), yR, dM)
    lo = np.asarray(active_lower).astype(bool); up = np.asarray(active_upper).astype(bool)
    act = lo | up
    act[:d.neq] = False
    W = np.concatenate([np.arange(d.neq), np.nonzero(act)[0]])
    bW = np.where(lo[W] & ~up[W], l0[W], u0b[W])
    bW[:d.neq] = l0[:d.neq]
    AW = pb.A[W]
    K = np.block([[pb.P, AW.T], [AW, np.zeros((len(W), len(W)))]])
    z = np.linalg.lstsq(K, np.concatenate([-q0, bW]), rcond=None)[0][:pb.P.shape[0]]
    return np.stack([z[min(k + 1, ph) * d.na + nx:(min(k + 1, ph) + 1) * d.na] for k in range(ph + 1)])


# ---------------------------------------------------------------------------------------------
# the kernel's formulas on the product's own arrays
# ---------------------------------------------------------------------------------------------
def arrays(c):
    a = S.arrays(c)
    rows16 = (a["ny"] * a["ph"] + 15) // 16 * 16
    a["Cq"] = c.debug_get("Cq").reshape(a["nz"], rows16).T[:a["ny"] * a["ph"]]        # column-major [rows16 x nz]
    a["m_rows"] = c.info()["m_ref"]
    return a


def cq_numpy(sp, blk):
    """d (outputs of the steps 1 .. ph) / d w, [ny ph x nz], by rolling the model out"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    nz = (max(blk[1:]) + 1) * nu
    out = np.zeros((ny * ph, nz))
    for q in range(nz):
        w = np.zeros(nz); w[q] = 1.0
        x = np.zeros(nx)
        for i in range(1, ph + 1):
            x = sp["A"] @ x + sp["B"] @ w[blk[i] * nu:(blk[i] + 1) * nu]
            out[(i - 1) * ny:i * ny, q] = sp["C"] @ x
    return out


def rollout(sp, x0, inp, dmeas=None):
    """seq_output [(ph + 1) x ny] of the input sequence `inp` [(ph + 1) x nu] as the solve writes it (row i = v_{min(i + 1, ph)})"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    dM = sp.get("dmeas", np.zeros((ndu, ph))) if dmeas is None else dmeas
    Bd = sp.get("Bd", np.zeros((nx, ndu))); Dd = sp.get("Dd", np.zeros((ny, ndu)))
    x = np.asarray(x0, float)
    out = np.zeros((ph + 1, ny))
    for i in range(ph + 1):
        out[i] = sp["C"] @ x + Dd @ dM[:, max(i - 1, 0)]
        if i < ph:
            x = sp["A"] @ x + sp["B"] @ inp[i] + Bd @ dM[:, i]
    return out


def condensed_gradients(a, active_lower, active_upper, u0, seq_output, seq_input, yref, uref, duref, seed_cmd=None, seed_input=None):
    """dict(OW, UW, DUW, lower, upper [m_rows], n, dependent); yref [ny x ph] etc. are the references of the instance, column = step"""
    nz, ldz, nu, ny, ph, blk = a["nz"], a["ldz"], a["nu"], a["ny"], a["ph"], a["blk"]
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
    mu = np.zeros(0)
    dependent = False
    if len(A):
        Sm = Y[np.ix_(A, A)]
        try:
            L = np.linalg.cholesky(Sm)
            dependent = bool((np.diag(L) ** 2 <= 1e-11 * np.diag(Sm)).any())
        except np.linalg.LinAlgError:
            dependent = True
        if not dependent:
            mu = np.linalg.solve(Sm, Y[A][:, :nz] @ p)
            q = q - Y[:nz][:, A] @ mu
    out = dict(n=len(A), dependent=dependent)
    gl = np.zeros(a["m_rows"]); gu = np.zeros(a["m_rows"])
    if dependent:
        for w, r in zip(WEIGHTS, (ny, nu, nu)):
            out[w] = np.full((r, ph), np.nan)
        out.update(lower=gl + np.nan, upper=gu + np.nan)
        return out
    for k, e in enumerate(A):
        if e < nz:
            rows = [r for r in a["boxrow_ref"][a["boxrow_ptr"][e]:a["boxrow_ptr"][e + 1]] if lo[r] or up[r]]
            r = min(rows)
        else:
            r = a["g_refrow"][e - ldz]
        (gu if up[r] else gl)[r] = mu[k]
    dy = (a["Cq"] @ q).reshape(ph, ny)                                   # row i - 1: step i
    dv = np.vstack([np.zeros(nu)] + [q[blk[i] * nu:(blk[i] + 1) * nu] for i in range(1, ph + 1)])       # row i: v_i, v_0 = lastU is data
    v = np.vstack([np.asarray(u0, float)] + [seq_input[i - 1] for i in range(1, ph + 1)])
    out["OW"] = np.stack([-dy[i] * (seq_output[i + 1] - yref[:, i]) for i in range(ph)], axis=1)
    out["UW"] = np.stack([-dv[i + 1] * (v[i + 1] - uref[:, i]) for i in range(ph)], axis=1)
    out["DUW"] = np.stack([-(dv[i + 1] - dv[i]) * (v[i + 1] - v[i] - duref[:, max(i - 1, 0)]) for i in range(ph)], axis=1)
    out.update(lower=gl, upper=gu)
    return out


def box_sums(a, g):
    """[m_rows] -> the same with the entries of the reference rows of one condensed variable replaced by their sum on the lowest-numbered row
    (move blocking: the truth spreads a multiplier over the parallel rows, the product files it under one)"""
    g = np.array(g, float)
    for e in range(a["nz"]):
        rows = a["boxrow_ref"][a["boxrow_ptr"][e]:a["boxrow_ptr"][e + 1]]
        rows = rows[rows < len(g)]
        if len(rows) > 1:
            s = g[rows].sum()
            g[rows] = 0.0
            g[rows.min()] = s
    return g


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's solve of a family and the truth for one random seed pair per usable instance: dict(sp, x0, u0, yref, res, truth [B] (None:
    unusable), seed_cmd, seed_input, tr)"""
    sp, x0, u0, yref = family(name)
    res = S.solve_batch(sp, x0, u0, yref)
    tr = Truth(sp)
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    rg = np.random.default_rng(17)
    B = len(x0)
    sc, sq = rg.normal(size=(B, nu)), rg.normal(size=(B, ph + 1, nu))
    truth = []
    for b in range(B):
        t = tr.gradients(x0[b], u0[b], yref[b], res["active_lower"][b], res["active_upper"][b], sc[b], sq[b]) if S.usable(res, b) else None
        truth.append(t if t is not None and S.good(t) else None)
    return dict(sp=sp, x0=x0, u0=u0, yref=yref, res=res, truth=truth, seed_cmd=sc, seed_input=sq, tr=tr)


def known_rows(a, n):
    """the rows of the reference QP that bound something in the condensed problem: the box rows of its variables and its general rows"""
    m = np.zeros(n, bool)
    for r in list(a["boxrow_ref"][:a["boxrow_ptr"][a["nz"]]]) + list(a["g_refrow"][:a["mg"]]):
        if 0 <= r < n:
            m[r] = True
    return m


def compare(a, t, g, blocked=False):
    """worst |g - truth| / max(1, max|truth|) over the five outputs.  lower / upper: over the rows the condensed problem has a bound for
    (known_rows); the product's entries of every other row must be zero.  Those others are the step-0 rows and, under move blocking, the rows
    that fix the moves past the control horizon at zero -- equalities of the reference QP written as rows with equal bounds, which the
    condensing has eliminated: their multipliers in the truth are no gradient this interface offers."""
    scale = max(1.0, max(np.abs(t[k]).max(initial=0.0) for k in WEIGHTS + ("lower", "upper")))
    worst = max(np.abs(np.asarray(g[k]) - t[k]).max(initial=0.0) for k in WEIGHTS)
    for k in ("lower", "upper"):
        n = min(len(t[k]), len(g[k]))
        known = known_rows(a, n)
        tk, gk = (box_sums(a, t[k][:n]), box_sums(a, np.asarray(g[k])[:n])) if blocked else (t[k][:n], np.asarray(g[k])[:n])
        worst = max(worst, np.abs(gk - tk)[known].max(initial=0.0))
        assert not np.abs(np.asarray(g[k])[:n][~known]).any() and not np.abs(np.asarray(g[k])[n:]).any()
    return worst / scale
