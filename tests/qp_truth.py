"""A certified truth for the LMPC solve kernels: the optimum of the reference's sparse QP itself, numpy + mpmath, no GPU, no product code.

    minimise  0.5 z'Pz + q'z   subject to   l <= Az <= u        (P, A, q, l, u of sens_ref.builder(sp): the reference's variables xi_i, delta_i,
                                                                 slack columns of soft rows; nothing of the condensed problem)

certified_optimum finds a working set with a float64 dual active-set iteration and then *certifies* it: the KKT system on the working
set is solved in float64 and refined with residuals evaluated in mpmath at 60 digits until the residual is below 1e-25 of the right-hand
side's scale; then, still in mpmath, every row is checked to lie inside its bounds and every active inequality row to carry a multiplier of
the right sign.  P is positive definite on the null space of the equality rows in every workload here, so a point that passes is the one
optimum of the QP -- a property of the QP, not of any solver.  The float64 work (an LU of the equality-constrained KKT matrix, shared by all
instances of a controller, and the Schur complement of the candidate rows on it) only proposes; nothing it computes is trusted.  P and A are
sparse: a residual costs as many mpmath operations as they have non-zeros, also at nz = 300 where a 60-digit LU would take hours.

restate_condensed is the kernels' formula (t0, S = Y[A, A], lambda, w; the cost from the multiplier identity or from its
definition as the controller's cost_direct flag says) in float64 numpy on the truth's working set and the arrays of mpcx_lmpc_debug_get of a
host-only handle.  Its only use is to derive the bound: RESTATEMENT_WORST[family] is its worst error against the truth (cmd and the three
sequences relative to max(1, max|.|) per instance, cost relative to max(1, |cost|)), measured on the CPU by tests/test_qp_truth.py, and the
kernels are held to KERNEL_TOL[family] = max(8 x that, 1e-12) -- the convention of sens_ref.RESTATEMENT_WORST and of the condensing
kernel's tests.  No bound is taken from a GPU run.

Degenerate instances.  Where margin < 1e-7 (a multiplier or a slack that small, each relative to its scale) or the working rows are linearly
dependent, the optimal working set or its multipliers are not unique: such an instance is left out of the active-bit and active_count
equalities -- never of cmd, cost or the sequences --, at most SKIP_CAP of a family, decided from the truth alone.  With move blocking the
bits are compared on rate_ref.compared_rows only and degeneracy is judged on those rows ('degenerate'); active_count counts every row, so it
is compared where no row at all is degenerate ('degenerate_all').

The workloads (families()) and their fixtures (tests/golden/qp_truth_*.npz, written by tests/golden/make_qp_golden.py) are defined here.
helpers.SHAPES_VARIANTS' v1_zero_weight is left out: its set-up regularises a singular Hessian, so the kernels solve another QP than the
reference's there."""
import functools
import os

import numpy as np

DPS = 60                    # mpmath digits
RES_TOL = 1e-25             # KKT residual / scale of the right-hand side after refinement
CHECK_TOL = 1e-18           # mpmath checks of bounds and signs: the refined point carries cond x RES_TOL of error (cond up to 3e5 here)
MARGIN_MIN = 1e-7
SKIP_CAP = 0.10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# worst error of restate_condensed against the truth per family, measured by tests/test_qp_truth.py on the CPU (the figure beside each is the
# measurement; the test asserts measured <= recorded <= 2 x measured)
RESTATEMENT_WORST = {
    "classes": 1.4e-13,     # measured 1.01e-13 (sequences 1.01e-13, cost 8.21e-14)
    "large": 1.3e-13,       # measured 9.07e-14 (sequences 9.07e-14, cost 1.55e-14)
    "v2": 5.2e-11,          # measured 3.68e-11 (sequences 3.37e-12, cost 3.68e-11)
    "v4": 4.4e-11,          # measured 3.17e-11 (sequences 2.14e-12, cost 3.17e-11)
    "ldg": 1.8e-11,         # measured 1.32e-11 (sequences 1.01e-12, cost 1.32e-11)
    "ch_lt_ph": 1.1e-13,    # measured 8.04e-14 (sequences 1.91e-14, cost 8.04e-14)
    "kin72": 2.1e-15,       # measured 1.52e-15 (sequences 8.88e-16, cost 1.52e-15)
    "nu1": 1.0e-13,         # measured 7.13e-14 (sequences 7.13e-14, cost 9.65e-15)
    "nu3": 7.5e-15,         # measured 5.33e-15 (sequences 5.33e-15, cost 2.02e-15)
    "nu5": 1.5e-14,         # measured 1.07e-14 (sequences 1.07e-14, cost 6.23e-16)
    "nx3": 3.6e-14,         # measured 2.55e-14 (sequences 2.55e-14, cost 2.25e-14)
    "ny_gt_nx": 2.7e-14,    # measured 1.92e-14 (sequences 1.64e-14, cost 1.92e-14)
    "ny_lt_nx": 2.8e-14,    # measured 2.00e-14 (sequences 2.00e-14, cost 6.02e-15)
    "nz47": 1.7e-11,        # measured 1.24e-11 (sequences 1.26e-12, cost 1.24e-11)
    "nz48": 4.1e-11,        # measured 2.93e-11 (sequences 1.97e-12, cost 2.93e-11)
    "nz49": 5.3e-11,        # measured 3.81e-11 (sequences 2.08e-12, cost 3.81e-11)
    "smallest": 1.9e-16,    # measured 1.34e-16 (sequences 1.34e-16, cost 1.73e-18)
    "full": 1.2e-14,        # measured 8.78e-15 (sequences 8.78e-15, cost 4.11e-15)
    "soft": 1.9e-14,        # measured 1.37e-14 (sequences 8.33e-15, cost 1.37e-14)
    "linear": 1.4e-14,      # measured 1.03e-14 (sequences 1.03e-14, cost 4.11e-15)
    "blocked": 3.6e-15,     # measured 2.58e-15 (sequences 2.58e-15, cost 7.77e-16)
    "terminal": 2.4e-14,    # measured 1.68e-14 (sequences 1.68e-14, cost 8.99e-15)
    "bank": 1.4e-13,        # measured 9.73e-14 (sequences 8.33e-14, cost 9.73e-14)
}
# worst |cmd - truth| / max(1, |cmd|) of the oracle's point over the instances it polished, measured the same way
ORACLE_WORST = {
    "classes": 7.3e-14,     # measured 6.88e-14
    "large": 5.2e-14,       # measured 4.91e-14
    "v2": 2.7e-13,          # measured 2.55e-13
    "v4": 1.4e-13,          # measured 1.31e-13
    "ldg": 4.0e-15,         # measured 3.77e-15
    "ch_lt_ph": 5.9e-16,    # measured 5.55e-16
    "kin72": 4.1e-16,       # measured 3.89e-16
    "nu1": 2.2e-14,         # measured 2.09e-14
    "nu3": 4.7e-16,         # measured 4.44e-16
    "nu5": 5.9e-16,         # measured 5.55e-16
    "nx3": 5.9e-17,         # measured 5.55e-17
    "ny_gt_nx": 2.6e-15,    # measured 2.44e-15
    "ny_lt_nx": 7.1e-16,    # measured 6.66e-16
    "nz47": 4.6e-14,        # measured 4.33e-14
    "nz48": 4.6e-14,        # measured 4.33e-14
    "nz49": 4.6e-14,        # measured 4.33e-14
    "smallest": 5.1e-17,    # measured 4.86e-17
    "full": 1.2e-15,        # measured 1.11e-15
    "soft": 4.7e-11,        # measured 4.39e-11
    "linear": 3.3e-14,      # measured 3.09e-14
    "blocked": 4.7e-16,     # measured 4.44e-16
    "terminal": 5.9e-16,    # measured 5.55e-16
    "bank": 4.9e-14,        # measured 4.58e-14
}


def kernel_tol(family):
    return max(8.0 * RESTATEMENT_WORST[family], 1e-12)


KERNEL_TOL = {family: kernel_tol(family) for family in RESTATEMENT_WORST}


# ---------------------------------------------------------------------------------------------
# the float64 proposer: one LU per controller, Schur complements per working set
# ---------------------------------------------------------------------------------------------
class _Structure:
    """what certified_optimum keeps per builder: the rows that are equalities (l == u), the candidate rows (a finite side, able to move), the LU
    of K0 = [[P, A_E'], [A_E, 0]], X = K0^-1 [A_I'; 0] and M = A_I X, and the non-zeros of P and A as mpmath numbers"""

    def __init__(self, pb, l, u):
        import scipy.linalg as sla
        P, A = np.asarray(pb.P, float), np.asarray(pb.A, float)
        self.n, self.m = n, m = P.shape[0], A.shape[0]
        self.E = np.nonzero(l == u)[0]
        fin = (np.isfinite(l) | np.isfinite(u)) & (l != u)
        mE = len(self.E)
        K0 = np.zeros((n + mE, n + mE))
        K0[:n, :n] = P; K0[:n, n:] = A[self.E].T; K0[n:, :n] = A[self.E]
        self.lu = sla.lu_factor(K0)
        cand = np.nonzero(fin)[0]
        rhs = np.zeros((n + mE, len(cand))); rhs[:n] = A[cand].T
        X = sla.lu_solve(self.lu, rhs)
        diag = np.einsum("ij,ji->i", A[cand], X[:n])
        # a row in the span of the equality rows (a bound on x0 or lastU, a hard step-0 row) cannot move: it is checked, never worked on
        move = diag > 1e-12 * np.maximum(1.0, (A[cand] ** 2).sum(axis=1))
        self.I = cand[move]
        self.X = np.ascontiguousarray(X[:, move])
        self.AI = A[self.I]
        self.M = self.AI @ self.X[:n]
        self.M = 0.5 * (self.M + self.M.T)
        self.pos = {int(r): k for k, r in enumerate(self.I)}
        self.A, self.P = A, P
        self.key = (l == u).tobytes()
        self._mp = None

    def mp_rows(self):
        """(rows of P, rows of A) as lists of (column, mpf): built once, at DPS digits"""
        if self._mp is None:
            import mpmath
            with mpmath.workdps(DPS):
                Pr = [[(int(j), mpmath.mpf(float(self.P[i, j]))) for j in np.nonzero(self.P[i])[0]] for i in range(self.n)]
                Ar = [[(int(j), mpmath.mpf(float(self.A[r, j]))) for j in np.nonzero(self.A[r])[0]] for r in range(self.m)]
            self._mp = (Pr, Ar)
        return self._mp

    def schur(self, S):
        """(indices into I, factor) of the working rows S; factor None where M[S, S] is not safely positive definite"""
        import scipy.linalg as sla
        k = np.array([self.pos[int(r)] for r in S], int)
        if len(k) == 0:
            return k, None
        Mss = self.M[np.ix_(k, k)]
        try:
            c = sla.cho_factor(Mss, lower=True)
            if (np.diag(c[0]) ** 2 <= 1e-11 * np.diag(Mss)).any():
                return k, None
            return k, c
        except np.linalg.LinAlgError:
            return k, None

    def solve(self, r1, rE, rS, S):
        """float64 solution (z, nu, y) of [[P, A_E', A_S'], [A_E, 0, 0], [A_S, 0, 0]] [z; nu; y] = [r1; rE; rS]"""
        import scipy.linalg as sla
        n = self.n
        base = sla.lu_solve(self.lu, np.concatenate([r1, rE]))
        if len(S) == 0:
            return base[:n], base[n:], np.zeros(0)
        k, c = self.schur(S)
        t = self.AI[k] @ base[:n] - rS
        y = sla.cho_solve(c, t) if c is not None else np.linalg.lstsq(self.M[np.ix_(k, k)], t, rcond=1e-12)[0]
        full = base - self.X[:, k] @ y
        return full[:n], full[n:], y


_STRUCT = {}


def structure(pb, l, u):
    st = _STRUCT.get(id(pb))
    if st is None or st[0] is not pb or st[1].key != (l == u).tobytes():
        st = (pb, _Structure(pb, np.asarray(l, float), np.asarray(u, float)))
        _STRUCT[id(pb)] = st
    return st[1]


def _working_set(st, q, l, u, seed):
    """float64 dual active-set iteration (Goldfarb and Idnani's, on the Schur complement M of the candidate rows): {row: side} (side +1: at u,
    -1: at l) or None at the iteration cap or where a violated row cannot be reached (infeasible).  The seed is first stripped of its
    wrong-signed rows, worst first, which leaves the optimum on a working set with multipliers of the right sign -- a state of the method;
    then the most violated row (relative to max(1, |bound|)) is brought to its bound, rows whose multiplier reaches zero on the way dropped."""
    import scipy.linalg as sla
    n = st.n
    base = sla.lu_solve(st.lu, np.concatenate([-q, l[st.E]]))
    t = st.AI @ base[:n]
    lo, hi = l[st.I], u[st.I]
    slo, shi = np.maximum(1.0, np.abs(np.where(np.isfinite(lo), lo, 0.0))), np.maximum(1.0, np.abs(np.where(np.isfinite(hi), hi, 0.0)))
    M = st.M

    def solve(k, rhs):
        Mkk = M[np.ix_(k, k)]
        try:
            return sla.cho_solve(sla.cho_factor(Mkk, lower=True), rhs)
        except np.linalg.LinAlgError:
            return np.linalg.lstsq(Mkk, rhs, rcond=1e-12)[0]

    W = [st.pos[r] for r in sorted(seed) if r in st.pos]
    side = [seed[int(st.I[i])] for i in W]
    y = np.zeros(0)
    while W:                                                   # strip the seed
        k = np.array(W, int); s = np.array(side, float)
        y = solve(k, t[k] - np.where(s > 0, hi[k], lo[k]))
        signed = y * s
        if signed.min() >= -1e-13 * max(1.0, np.abs(y).max()):
            break
        j = int(np.argmin(signed))
        del W[j]; del side[j]
        y = np.zeros(0)
    y = list(y)
    for _ in range(20 * len(st.I) + 200):
        k = np.array(W, int)
        v = t - (M[:, k] @ np.array(y) if len(k) else 0.0)
        with np.errstate(invalid="ignore"):
            viol_lo = np.where(np.isfinite(lo), (lo - v) / slo, -np.inf)
            viol_hi = np.where(np.isfinite(hi), (v - hi) / shi, -np.inf)
        viol = np.maximum(viol_lo, viol_hi)
        viol[k] = -np.inf
        p = int(np.argmax(viol)) if len(viol) else -1
        if p < 0 or viol[p] <= 1e-12:
            return {int(st.I[i]): s for i, s in zip(W, side)}
        sp_ = 1.0 if viol_hi[p] >= viol_lo[p] else -1.0
        bp = hi[p] if sp_ > 0 else lo[p]
        yp = 0.0
        for _inner in range(len(st.I) + 10):                   # bring row p to its bound
            k = np.array(W, int)
            if len(k):
                r = solve(k, M[k, p])
                kappa = M[p, p] - M[p, k] @ r
                vp = t[p] - M[p, k] @ np.array(y) - M[p, p] * yp
                s = np.array(side, float)
                grow = s * sp_ * r                             # lambda_j falls at this rate per unit step
                lam = np.array(y) * s
                with np.errstate(divide="ignore", invalid="ignore"):
                    tj = np.where(grow > 1e-14 * max(1.0, np.abs(r).max()), np.maximum(lam, 0.0) / grow, np.inf)
                j = int(np.argmin(tj)); tau1 = tj[j]
            else:
                r = np.zeros(0); kappa = M[p, p]; vp = t[p] - M[p, p] * yp; tau1 = np.inf; j = -1
            tau2 = abs(vp - bp) / kappa if kappa > 1e-12 * M[p, p] else np.inf
            if not np.isfinite(min(tau1, tau2)):
                return None
            tau = min(tau1, tau2)
            y = list(np.array(y) - r * sp_ * tau)
            yp += sp_ * tau
            if tau2 <= tau1:
                W.append(p); side.append(int(sp_)); y.append(yp)
                break
            del W[j]; del side[j]; del y[j]
        else:
            return None
    return None


def _signed_support(st, q, l, u, W):
    """for linearly dependent working rows: multipliers of the right sign by non-negative least squares on the Schur complement, and the rows
    that carry them -- ({row: side} of the support, residual / scale)"""
    import scipy.linalg as sla
    from scipy.optimize import nnls
    rows = sorted(W)
    k = np.array([st.pos[r] for r in rows], int)
    side = np.array([W[r] for r in rows], float)
    base = sla.lu_solve(st.lu, np.concatenate([-q, l[st.E]]))
    b = np.array([u[r] if W[r] > 0 else l[r] for r in rows])
    rhs = st.AI[k] @ base[:st.n] - b
    lam, res = nnls(st.M[np.ix_(k, k)] * side[None, :], rhs, maxiter=50 * len(k) + 100)
    keep = lam > 1e-12 * max(1.0, lam.max(initial=0.0))
    return {rows[i]: W[rows[i]] for i in np.nonzero(keep)[0]}, res / max(1.0, np.abs(rhs).max())


def _certify(st, q, l, u, S):
    """the KKT system on the rows S ({row: side}) refined in mpmath; dict(ok, z, nu, y, Az, violated, wrong, residual) -- everything mpmath"""
    import mpmath
    mpf = mpmath.mpf
    rows = sorted(S)
    Pr, Ar = st.mp_rows()
    E = [int(r) for r in st.E]
    n = st.n
    with mpmath.workdps(DPS):
        mq = [mpf(float(v)) for v in q]
        bE = [mpf(float(l[r])) for r in E]
        bS64 = np.array([u[r] if S[r] > 0 else l[r] for r in rows], float)
        bS = [mpf(float(v)) for v in bS64]
        scale = max(1.0, np.abs(q).max(initial=0.0), np.abs(l[st.E]).max(initial=0.0), np.abs(bS64).max(initial=0.0))
        z, nu, y = st.solve(-q, l[st.E], bS64, rows)
        Z = [mpf(float(v)) for v in z]; NU = [mpf(float(v)) for v in nu]; Y = [mpf(float(v)) for v in y]
        res = None
        for it in range(16):
            r1 = [-v for v in mq]
            for i in range(n):
                acc = r1[i]
                for j, p in Pr[i]:
                    acc -= p * Z[j]
                r1[i] = acc
            r2 = []
            for e, r in enumerate(E):
                acc = bE[e]
                for j, a in Ar[r]:
                    acc -= a * Z[j]
                    r1[j] -= a * NU[e]
                r2.append(acc)
            r3 = []
            for e, r in enumerate(rows):
                acc = bS[e]
                for j, a in Ar[r]:
                    acc -= a * Z[j]
                    r1[j] -= a * Y[e]
                r3.append(acc)
            res = float(max([abs(v) for v in r1] + [abs(v) for v in r2] + [abs(v) for v in r3])) / scale
            if res <= RES_TOL:
                break
            dz, dnu, dy = st.solve(np.array([float(v) for v in r1]), np.array([float(v) for v in r2]), np.array([float(v) for v in r3]), rows)
            for i in range(n):
                Z[i] += mpf(float(dz[i]))
            for e in range(len(E)):
                NU[e] += mpf(float(dnu[e]))
            for e in range(len(rows)):
                Y[e] += mpf(float(dy[e]))
        out = dict(ok=False, residual=res, z=Z, nu=NU, y=dict(zip(rows, Y)), violated={}, wrong=[])
        if res is None or res > RES_TOL:
            return out
        # every row inside its bounds, every working row's multiplier of its side's sign (y >= 0 at u, y <= 0 at l)
        Az = []
        for r in range(st.m):
            acc = mpf(0)
            for j, a in Ar[r]:
                acc += a * Z[j]
            Az.append(acc)
        out["Az"] = Az
        for r in range(st.m):
            if r in S:
                continue
            if np.isfinite(l[r]) and Az[r] < mpf(float(l[r])) - CHECK_TOL * max(1.0, abs(l[r])):
                out["violated"][r] = -1
            if np.isfinite(u[r]) and Az[r] > mpf(float(u[r])) + CHECK_TOL * max(1.0, abs(u[r])):
                out["violated"][r] = 1
        ymax = max([abs(v) for v in Y] + [mpf(1)])
        out["wrong"] = [r for e, r in enumerate(rows) if Y[e] * S[r] < -CHECK_TOL * ymax]
        out["ok"] = not out["violated"] and not out["wrong"]
        cost = mpf(0)
        for i in range(n):
            acc = mpf(0)
            for j, p in Pr[i]:
                acc += p * Z[j]
            cost += Z[i] * (acc / 2 + mq[i])
        out["cost"] = cost
        return out


def _search(st, q, l, u, seed):
    """working set by the float64 iteration, certificate in mpmath, repairs by what the certificate saw: (W, S, dependent, cert) or None"""
    W = _working_set(st, q, l, u, seed)
    if W is None:
        return None
    for _ in range(8):
        _, c = st.schur(sorted(W))
        dependent = bool(len(W)) and c is None
        S = W
        if dependent:
            S, nres = _signed_support(st, q, l, u, W)
            if nres > 1e-9:
                return None
        cert = _certify(st, q, l, u, S)
        if cert["ok"]:
            return W, S, dependent, cert
        if cert["residual"] is None or cert["residual"] > RES_TOL:
            return None
        # the 60-digit check saw what float64 could not: drop the wrong-signed rows, add the violated ones, certify again
        W = {r: s for r, s in S.items() if r not in cert["wrong"]}
        for r, s in cert["violated"].items():
            if r not in st.pos:
                return None                # a row that cannot move is violated: the QP is infeasible
            W[r] = s
    return None


def certified_optimum(pb, q, l, u, seed_lower=None, seed_upper=None, compared=None):
    """The optimum of min 0.5 z'Pz + q'z, l <= Az <= u (P, A of the builder `pb`), certified in mpmath, or None where no working set was found
    within the caps (the workloads are chosen so that this does not happen).  seed_*: [ncon] flags of a first working set (the oracle's), else
    the empty set.  compared: [ncon] mask of the rows whose active bits a test compares (default: all) -- 'margin_compared' and 'degenerate' are
    judged on those.  Returns, rounded to float64: z, cmd, cost, state / output / input (oracle.lmpc_numpy.unpack_solution needs dims and the
    disturbance: see truth_of), active_lower / active_upper [ncon] uint8, n_active, mult [ncon], margin, margin_compared, dependent,
    degenerate, degenerate_all, residual."""
    import mpmath
    q, l, u = np.asarray(q, float), np.asarray(l, float), np.asarray(u, float)
    st = structure(pb, l, u)
    seed = {}
    if seed_lower is not None:
        for r in np.nonzero(np.asarray(seed_lower))[0]:
            seed[int(r)] = -1
    if seed_upper is not None:
        for r in np.nonzero(np.asarray(seed_upper))[0]:
            seed[int(r)] = 1
    found = _search(st, q, l, u, seed)
    if found is None and seed:
        found = _search(st, q, l, u, {})         # (a seed with dependent rows in it can lead nowhere: start again from nothing)
    if found is None:
        return None
    W, S, _, cert = found
    m = st.m
    with mpmath.workdps(DPS):
        z = np.array([float(v) for v in cert["z"]])
        Az = cert["Az"]
        mult = np.zeros(m)
        for r, v in cert["y"].items():
            mult[r] = float(v)
        lower = np.zeros(m, np.uint8); upper = np.zeros(m, np.uint8)
        for r, s in S.items():
            (upper if s > 0 else lower)[r] = 1
        ymax = max(1.0, np.abs(mult).max(initial=0.0))
        per_row = np.full(m, np.inf)             # |multiplier| of an active row, slack of an inactive one, each relative to its scale
        for r in st.I:
            r = int(r)
            if r in S:
                per_row[r] = abs(mult[r]) / ymax
            else:
                s = np.inf
                if np.isfinite(l[r]):
                    s = min(s, float(Az[r] - mpmath.mpf(float(l[r]))) / max(1.0, abs(l[r])))
                if np.isfinite(u[r]):
                    s = min(s, float(mpmath.mpf(float(u[r])) - Az[r]) / max(1.0, abs(u[r])))
                per_row[r] = max(s, 0.0)
        cost = float(cert["cost"])
    comp = np.ones(m, bool) if compared is None else np.asarray(compared, bool)
    margin = float(per_row.min(initial=np.inf))
    margin_c = float(per_row[comp].min(initial=np.inf))
    # Judged from the point alone, not from the path to it: the tight rows are the working rows and every other row within MARGIN_MIN of its
    # bound.  They are dependent where M on them loses rank; the multipliers of the compared rows are unique all the same if the null space does
    # not reach those rows.
    tight = sorted(set(S) | {int(r) for r in st.I if per_row[int(r)] < MARGIN_MIN})
    touch = dependent = False
    if tight:
        k = np.array([st.pos[r] for r in tight], int)
        w_, V = np.linalg.eigh(st.M[np.ix_(k, k)])
        null = V[:, w_ <= 1e-11 * max(w_.max(), 1e-300)]
        dependent = bool(null.shape[1])
        touch = bool((np.abs(null[comp[tight]]) > 1e-8).any())
    return dict(z=z, cost=cost, active_lower=lower, active_upper=upper, n_active=int(lower.sum() + upper.sum()), mult=mult,
                margin=margin, margin_compared=margin_c, dependent=dependent, degenerate=bool(margin_c < MARGIN_MIN or touch),
                degenerate_all=bool(margin < MARGIN_MIN or dependent), residual=cert["residual"])


# ---------------------------------------------------------------------------------------------
# the kernels' formula in float64 numpy
# ---------------------------------------------------------------------------------------------
def arrays(c, sp):
    """what restate_condensed reads: sens_ref.arrays of a (host-only) controller, its bounds, the fused map's other rows and the model of `sp`"""
    import sens_ref as SF
    a = SF.arrays(c)
    df = c.debug_get("dims_fused")
    a.update(nsp=int(df[1]), ione=int(df[6]), ldg=int(c.debug_get("dims")[3]), cost_direct=int(c.debug_get("flags")[0]))
    for n in ("lw", "uw", "lg0", "ug0", "g_soft"):
        a[n] = c.debug_get(n)
    a["H"] = c.debug_get("H").reshape(a["ldz"], a["ldz"]).T
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    a.update(A=sp["A"], B=sp["B"], C=sp["C"], Bd=sp.get("Bd", np.zeros((nx, ndu))), Dd=sp.get("Dd", np.zeros((ny, ndu))),
             dmeas=sp.get("dmeas", np.zeros((ndu, ph))))
    return a


def _dot(M, v):
    """M v by numpy's own pairwise sums: no BLAS, so the figure the bound is derived from does not move with a library's blocking or threads"""
    return (np.asarray(M) * np.asarray(v)).sum(axis=-1)


def _spd_solve(S, r):
    """S^-1 r by a Cholesky factorisation written out (the same reason)"""
    n = len(r)
    L = np.zeros((n, n))
    for j in range(n):
        c = S[j:, j] - _dot(L[j:, :j], L[j, :j])
        L[j:, j] = c / np.sqrt(c[0])
    y = np.zeros(n)
    for j in range(n):
        y[j] = (r[j] - _dot(L[j, :j], y[:j])) / L[j, j]
    x = np.zeros(n)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - _dot(L[j + 1:, j], x[j + 1:])) / L[j, j]
    return x


def restate_condensed(a, x0, u0, yref, dmeas, active):
    """dict(cmd, cost, input, state, output, n) of one instance on the working set `active` = (lower, upper) flags in reference rows.  yref:
    [ny], constant along the horizon (the fused map MF1 is the one for that); dmeas: None, the controller's own"""
    import sens_ref as SF
    assert dmeas is None
    lower, upper = (np.asarray(f).astype(bool) for f in active)
    nz, mg, ldz, ldy, ldg, nu, nx, ph = a["nz"], a["mg"], a["ldz"], a["ldy"], a["ldg"], a["nu"], a["nx"], a["ph"]
    vin = np.zeros(a["kin"])
    vin[:nx] = x0; vin[a["nxp"]:a["nxp"] + nu] = u0; vin[a["nxp"] + a["nup"]:a["nxp"] + a["nup"] + a["ny"]] = yref; vin[a["ione"]] = 1.0
    out = _dot(a["MF1"], vin)
    r_f = ldy + ldg; r_q = r_f + ldz + a["nsp"]
    t = out[:ldy]                                                   # [t0; G t0] in unified indices
    goff = out[ldy:ldy + mg]
    f = out[r_f:r_f + nz]
    c0 = 0.5 * _dot(vin, out[r_q:r_q + a["kin"]])
    lo = np.full(ldy, -np.inf); hi = np.full(ldy, np.inf)
    lo[:nz] = a["lw"][:nz]; hi[:nz] = a["uw"][:nz]
    lo[ldz:ldz + mg] = a["lg0"][:mg] - goff; hi[ldz:ldz + mg] = a["ug0"][:mg] - goff
    Aset = SF.working_set(a, lower | upper)
    at_lower = set(SF.working_set(a, lower).tolist())
    w = t[:nz].copy()
    lam = np.zeros(0); b = np.zeros(0)
    if len(Aset):
        b = np.array([lo[i] if i in at_lower else hi[i] for i in Aset])
        lam = _spd_solve(a["Y"][np.ix_(Aset, Aset)], t[Aset] - b)
        w = t[:nz] - _dot(a["Y"][:nz][:, Aset], lam)
    if a["cost_direct"]:
        gen = Aset >= ldz
        pen = 0.5 * (a["g_soft"][Aset[gen] - ldz] * lam[gen] ** 2).sum() if len(Aset) else 0.0
        cost = 0.5 * _dot(w, _dot(a["H"][:nz, :nz], w)) + _dot(f, w) + pen + c0
    else:
        cost = 0.5 * (_dot(f, w) - _dot(lam, b)) + c0
    blk = a["blk"]
    inp = np.stack([w[blk[min(i + 1, ph)] * nu:(blk[min(i + 1, ph)] + 1) * nu] for i in range(ph + 1)])
    state, outp = rollout(a, x0, inp)
    return dict(cmd=inp[0].copy(), cost=float(cost), input=inp, state=state, output=outp, n=len(Aset))


def rollout(a, x0, inp):
    """states and outputs of an input sequence [ph + 1, nu] in float64: x_{i+1} = A x_i + B u_i + Bd d_i, y_i = C x_i + Dd d_{max(i-1, 0)}"""
    ph = inp.shape[0] - 1
    d = a["dmeas"]
    state = np.zeros((ph + 1, len(x0))); state[0] = x0
    for i in range(ph):
        state[i + 1] = _dot(a["A"], state[i]) + _dot(a["B"], inp[i]) + (_dot(a["Bd"], d[:, i]) if d.size else 0.0)
    outp = np.stack([_dot(a["C"], state[i]) + (_dot(a["Dd"], d[:, max(i - 1, 0)]) if d.size else 0.0) for i in range(ph + 1)])
    return state, outp


def errors(got, truth):
    """(worst of cmd and the sequences relative to max(1, max|.|), cost relative to max(1, |cost|)) of one instance; got, truth: mappings with
    cmd, cost, input, state, output"""
    e = 0.0
    for k in ("cmd", "input", "state", "output"):
        tk = np.asarray(truth[k], float)
        e = max(e, float(np.abs(np.asarray(got[k], float) - tk).max(initial=0.0)) / max(1.0, float(np.abs(tk).max(initial=0.0))))
    return e, abs(float(got["cost"]) - float(truth["cost"])) / max(1.0, abs(float(truth["cost"])))


# ---------------------------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------------------------
CLASSES_PER_CLASS = 4          # instances per size class of test_lmpc_round_classes.ROUND_CLASSES
CLASSES_PAST_16 = 12
LARGE_BATCH, LARGE_SEED = 64, 2024
VARIANT_BATCH, VARIANT_SEED = 8, 11
EDGE_BATCH, EDGE_SEED = 8, 5
# ch_lt_ph: a velocity that rides its bound across the end of the control horizon with the held input at zero leaves every later velocity row on
# its bound too, the multiplier free to sit on any of them -- a quarter of this controller's instances.  Its fixture takes, from the 64 instances
# test_lmpc_shapes_gpu.py draws, BLOCKED_PLAIN whose truth is not degenerate and one degenerate one (9 %: under SKIP_CAP), those the oracle did not polish first
BLOCKED_DRAW, BLOCKED_PLAIN, BLOCKED_DEGENERATE = 64, 10, 1
BANK_MODELS, BANK_BATCH, BANK_SEED = 8, 32, 3
AXES_FAMILIES = ("classes", "large", "v2", "v4", "ldg")
FEATURE_FAMILIES = ("smallest", "full", "soft", "linear", "blocked", "terminal")


def edge_families():
    from helpers import SHAPES_EDGES
    return tuple(sorted(SHAPES_EDGES))


def families():
    return AXES_FAMILIES + edge_families() + FEATURE_FAMILIES + ("bank",)


def _axes(sp):
    """an axes_spec as a rate_ref spec: zero references, which is what configure_axes sets"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    return dict(sp, yref=np.zeros((ny, ph)), uref=np.zeros((nu, ph)), duref=np.zeros((nu, ph)))


@functools.lru_cache(maxsize=None)
def workload(name):
    """dict(kind 'axes' | 'feature', sp (a rate_ref spec), x0, u0, yref [B, ny], and for 'bank': sps, model).  'classes' is the whole batch of
    test_lmpc_round_classes and 'ch_lt_ph' the whole draw (the fixture's 'pick' selects from them)."""
    from helpers import SHAPES_EDGES, SHAPES_MAIN, SHAPES_VARIANTS, axes_batch, axes_spec
    import sens_ref as SF
    if name in FEATURE_FAMILIES:
        sp, x0, u0, yref = SF.family(name)
        return dict(kind="feature", sp=sp, x0=x0, u0=u0, yref=yref)
    if name == "bank":
        sps = [_axes(axes_spec(3, 20, perturb=0.2, seed=1000 + k)) for k in range(BANK_MODELS)]
        x0, u0, yref = axes_batch(sps[0], BANK_BATCH, seed=BANK_SEED)
        return dict(kind="axes", sp=sps[0], sps=sps, model=np.arange(BANK_BATCH) % BANK_MODELS, x0=x0, u0=u0, yref=yref)
    if name == "classes":
        from test_lmpc_round_classes import ROUND_BATCH, ROUND_SEED, ROUND_SPEC
        sp, B, seed = axes_spec(**ROUND_SPEC), ROUND_BATCH, ROUND_SEED
    elif name == "large":
        sp, B, seed = axes_spec(*SHAPES_MAIN[:2]), LARGE_BATCH, LARGE_SEED
    elif name in ("v2", "v4", "ldg"):
        sp, B, seed = axes_spec(**SHAPES_VARIANTS[name][0]), VARIANT_BATCH, VARIANT_SEED
    else:
        sp, B, seed = axes_spec(**SHAPES_EDGES[name]), (BLOCKED_DRAW if name == "ch_lt_ph" else EDGE_BATCH), EDGE_SEED
    x0, u0, yref = axes_batch(sp, B, seed=seed)
    return dict(kind="axes", sp=_axes(sp), x0=x0, u0=u0, yref=yref)


def configure(c, sp):
    """the controller of a workload's spec on a libmpc_amd.LMPC (axes families: helpers.configure_axes' calls; the others: sens_ref.configure)"""
    import sens_ref as SF
    if "nax" in sp:
        from helpers import SHAPES_MAXIT, configure_axes
        return configure_axes(c, sp, SHAPES_MAXIT)
    return SF.configure(c, sp)


def compared_rows(sp):
    import linear_ref as LR
    return LR.compared_rows(sp)


def qlu(pb, sp, x0, u0, yref):
    """q, l, u of one instance (yref [ny], constant along the horizon; the controller's disturbance)"""
    import sens_ref as SF
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    return SF._qlu(pb, sp, x0, u0, np.tile(np.asarray(yref, float)[:, None], (1, ph)), sp.get("dmeas", np.zeros((ndu, ph))))


def truth_of(pb, sp, x0, u0, yref, seed_lower=None, seed_upper=None):
    """certified_optimum of one instance with cmd and the sequences unpacked (LN.unpack_solution), or None"""
    from oracle import lmpc_numpy as LN
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    q, l, u = qlu(pb, sp, x0, u0, yref)
    t = certified_optimum(pb, q, l, u, seed_lower, seed_upper, compared=compared_rows(sp))
    if t is None:
        return None
    state, out, inp = LN.unpack_solution(pb.d, t["z"], pb.ssC[:ny, :nx], pb.ssDv[:ny, :], sp.get("dmeas", np.zeros((ndu, ph))))
    t.update(cmd=inp[0].copy(), state=state, output=out, input=inp)
    return t


def oracle_solve(name):
    """the oracle's solve of a workload: dict with cmd, polished, active_lower / active_upper [B, ncon] (seeds of the truth, nothing more)"""
    from helpers import SHAPES_MAXIT, oracle_batch_parallel_spec
    import sens_ref as SF
    w = workload(name)
    if w["kind"] == "feature":
        return SF.solve_batch(w["sp"], w["x0"], w["u0"], w["yref"])
    if name == "bank":
        parts = [oracle_batch_parallel_spec(w["sps"][k], w["x0"][b:b + 1], w["u0"][b:b + 1], maximum_iteration=SHAPES_MAXIT, workers=1)
                 for b, k in enumerate(w["model"])]
        return {k: np.concatenate([p[k] for p in parts]) for k in ("cmd", "polished", "active_lower", "active_upper")}
    return oracle_batch_parallel_spec(w["sp"], w["x0"], w["u0"], maximum_iteration=SHAPES_MAXIT)


# ---------------------------------------------------------------------------------------------
# fixtures: tests/golden/qp_truth_<file>.npz holds (family, first, last) parts; the arrays of a part are named <family>__<key>
# ---------------------------------------------------------------------------------------------
FILES = {
    "classes": [("classes", 0, None)],
    "large_a": [("large", 0, 32)],
    "large_b": [("large", 32, 64)],
    "large_bank": [("bank", 0, None)],
    "variants": [("v2", 0, None), ("ldg", 0, None)],
    "v4": [("v4", 0, None)],
    "edges_a": [(n, 0, None) for n in ("nu1", "nu3", "nu5", "nx3", "ny_lt_nx", "ny_gt_nx")],
    "edges_b": [(n, 0, None) for n in ("ch_lt_ph", "nz47", "nz48", "nz49", "kin72")],
    "features_a": [(n, 0, None) for n in ("smallest", "full", "soft")],
    "features_b": [(n, 0, None) for n in ("linear", "blocked", "terminal")],
}
PER_INSTANCE = ("x0", "u0", "yref", "cmd", "cost", "seq_input", "seq_state", "seq_output", "active_lower", "active_upper", "n_active", "margin",
                "margin_compared", "dependent", "degenerate", "degenerate_all", "polished", "oracle_cmd", "pick", "model")
MAX_FIXTURE_BYTES = 139448          # the largest fixture committed before these (condense_truth_rows.npz)


def path(file):
    return os.path.join(GOLDEN, "qp_truth_%s.npz" % file)


@functools.lru_cache(maxsize=None)
def load(family):
    """the fixture of a family, its parts joined: per-instance arrays, 'dmeas' [ndu, ph], 'ncon', 'neq'; active_* unpacked to [B, ncon] uint8"""
    parts = []
    for file, members in FILES.items():
        for fam, first, last in members:
            if fam == family:
                with np.load(path(file)) as g:
                    parts.append((first, {k[len(fam) + 2:]: g[k] for k in g.files if k.startswith(fam + "__")}))
    assert parts, family
    parts.sort(key=lambda p: p[0])
    out = {}
    for k in parts[0][1]:
        out[k] = np.concatenate([p[k] for _, p in parts]) if k in PER_INSTANCE else parts[0][1][k]
    m = int(out["ncon"])
    for k in ("active_lower", "active_upper"):
        out[k] = np.unpackbits(out[k], axis=1, bitorder="little")[:, :m]
    return out


def inputs_of(family):
    """(sp or the bank's list, x0, u0, yref) of the fixture's instances, from the workload definition (the fixture's 'pick' selects for 'classes')"""
    w = workload(family)
    g = load(family)
    pick = g["pick"]
    return w, w["x0"][pick], w["u0"][pick], w["yref"][pick]
