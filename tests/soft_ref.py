"""Reference for the soft constraints: the reference QP of rate_ref.builder with one slack variable per soft row,

    minimise   0.5 z'Pz + q'z + 0.5 sum_r rho_r s_r^2      subject to   l_r <= a_r z - s_r <= u_r   (soft rows),   l <= A z <= u  (the others)

i.e. P' = blkdiag(P, diag rho), q' = [q; 0] and a -1 in row r of the new column; bounds and row numbering stay.  Solved by the numpy
restatement of OSQP exactly as rate_ref.solve_one does it (a "polished" point with a wrong-signed multiplier does not count as polished).
Also: an independent numpy condensing of the general rows of a soft-constrained controller for the host tests.

A controller is a rate_ref spec with sp["soft"] = dict(xw=[nx] | None, yw=[ny] | None, sw=float | None): the weights of the state, output
and scalar rows over the slice (sp["first"], ph) the bounds are set on; inf entries stay hard."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import rate_ref as RR
from oracle import lmpc_numpy as LN

INF = float("inf")


def with_soft(sp, xw=None, yw=None, sw=None):
    out = dict(sp)
    out["soft"] = dict(xw=None if xw is None else np.asarray(xw, float), yw=None if yw is None else np.asarray(yw, float),
                       sw=None if sw is None else float(sw))
    return out


def configure(c, sp, maximum_iteration=RR.MAXIT, soft=True, **kw):
    """rate_ref.configure, then the weights on the slice the bounds were set on"""
    RR.configure(c, sp, maximum_iteration, **kw)
    if soft and "soft" in sp:
        s = sp["soft"]
        assert c.setSoftConstraintWeights(s["xw"], s["yw"], s["sw"], (sp.get("first", 0), sp["dims"][4]))
    return c


def _steps(sp):
    """internal steps a slice (first, ph) writes: user index i -> step i + 1, and step 0 with index 0"""
    first, ph = sp.get("first", 0), sp["dims"][4]
    return ([0] if first == 0 else []) + list(range(first + 1, ph + 1))


def soft_rows(sp, pb):
    """[(row in the inequality block, rho)] of the soft rows: a finite weight on a row with a finite bound, in row order"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = pb.d
    s = sp.get("soft", {})
    rows = []
    for i in _steps(sp):
        for j in range(nx):
            if s.get("xw") is not None and np.isfinite(s["xw"][j]):
                rows.append((i * d.na + j, float(s["xw"][j])))
        for j in range(ny):
            if s.get("yw") is not None and np.isfinite(s["yw"][j]):
                rows.append((d.off_y + i * ny + j, float(s["yw"][j])))
        if s.get("sw") is not None and np.isfinite(s["sw"]):
            rows.append((d.off_s + i, float(s["sw"])))
    rows = [(r, w) for r, w in rows if np.isfinite(pb.lineq[r]) or np.isfinite(pb.uineq[r])]
    return sorted(rows)


class SoftBuilder:
    """rate_ref.builder(sp) with the slack columns: what rate_ref.solve_one reads of a builder (d, P, A, get, ssC, ssDv)"""

    def __init__(self, sp):
        self.pb = pb = RR.builder(sp)
        self.d = pb.d
        self.rows = soft_rows(sp, pb)
        n, m, k = pb.d.nvar, pb.d.ncon, len(self.rows)
        self.P = np.zeros((n + k, n + k)); self.P[:n, :n] = pb.P
        self.A = np.zeros((m, n + k)); self.A[:, :n] = pb.A
        for c, (r, rho) in enumerate(self.rows):
            self.P[n + c, n + c] = rho
            self.A[pb.d.neq + r, n + c] = -1.0
        self.ssC, self.ssDv = pb.ssC, pb.ssDv

    def get(self, *a):
        q, l, u = self.pb.get(*a)
        return np.concatenate([q, np.zeros(len(self.rows))]), l, u


def solve_batch(sp, x0, u0, yref=None, dmeas=None, maximum_iteration=RR.MAXIT, workers=None):
    """rate_ref.solve_batch on the slack-augmented QP; the active bits of the step-0 box rows are cleared for the hard ones only (a soft
    step-0 state row reports its violation).  Adds 'n_soft_active', 'slack' [B, soft rows] and 'soft_rows' (reference row numbers)."""
    pb = SoftBuilder(sp)
    d = pb.d
    B = len(x0)
    workers = workers or max(1, min(4, os.cpu_count() or 1))

    def job(b):
        return RR.solve_one(pb, sp, x0[b], u0[b], None if yref is None else yref[b], None if dmeas is None else dmeas[b], maximum_iteration)
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(job, range(B)))
    res = {"neq": d.neq, "ncon": d.ncon}
    res["cmd"] = np.stack([p["cmd"] for p in parts]); res["cost"] = np.array([p["cost"] for p in parts])
    res["input"] = np.stack([p["input"] for p in parts]); res["state"] = np.stack([p["state"] for p in parts])
    for k in ("status", "solver_status", "iters", "polished", "polished_raw", "is_feasible"):
        res[k] = np.array([int(p[k]) for p in parts], dtype=np.int32)
    soft = np.array([d.neq + r for r, _ in pb.rows], dtype=int)
    for k in ("active_lower", "active_upper"):
        res[k] = np.stack([p[k] for p in parts])
        keep = res[k][:, soft].copy()
        res[k][:, d.neq:d.neq + d.na] = 0
        res[k][:, soft] = keep
    act = (res["active_lower"] != 0) | (res["active_upper"] != 0)
    res["n_active"] = act[:, d.neq:].sum(axis=1)
    res["n_soft_active"] = act[:, soft].sum(axis=1)
    res["soft_rows"] = soft
    res["y"] = np.stack([p["y"] for p in parts])
    res["slack"] = res["y"][:, soft] / np.array([w for _, w in pb.rows])[None, :] if len(soft) else np.zeros((B, 0))
    return res


def hard_infeasible(sp, x0, u0, maximum_iteration=RR.MAXIT):
    """per instance: is the QP with every row hard primal infeasible (the numpy OSQP's certificate)"""
    hard = {k: v for k, v in sp.items() if k != "soft"}
    pb = RR.builder(hard)
    return np.array([RR.solve_one(pb, hard, x0[b], u0[b], maximum_iteration=maximum_iteration)["solver_status"] == RR.OSQP.OSQP_PRIMAL_INFEASIBLE
                     for b in range(len(x0))])


# ---------------------------------------------------------------------------------------------
# an independent condensing of the general rows (host tests)
# ---------------------------------------------------------------------------------------------
def condensed(sp):
    """numpy condensing, independent of the product: dict(H [nz x nz], G [m x nz], lo, hi, kind, step, comp, refrow, g_soft [m], fixed)
    with the general rows in the product's order -- the soft step-0 rows (state, output, scalar), then per step the state, output, scalar
    and rate rows; a row without coefficients is a general row if it is soft and counted in `fixed` otherwise"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    pb = RR.builder({k: v for k, v in sp.items() if k != "soft"})
    d = pb.d
    weight = dict(soft_rows(sp, pb))
    nf = min(ph, ch + 1)
    nz = nf * nu
    blk = [0] + [min(i, nf) - 1 for i in range(1, ph + 1)]
    A, Bm, C = sp["A"], sp["B"], sp["C"]

    def E(i):
        e = np.zeros((nu, nz)); e[:, blk[i] * nu:(blk[i] + 1) * nu] = np.eye(nu)
        return e
    Sx = [np.zeros((nx, nz))]
    for i in range(1, ph + 1):
        Sx.append(A @ Sx[-1] + Bm @ E(i))
    H = np.zeros((nz, nz))
    for i in range(1, ph + 1):
        CS = C @ Sx[i]
        H += CS.T @ np.diag(pb.wOutput[:, i]) @ CS + E(i).T @ np.diag(pb.wU[:, i]) @ E(i)
    for i in range(ph):
        D = E(i + 1) - (E(i) if i >= 1 else 0.0)
        H += D.T @ np.diag(pb.wDeltaU[:, i]) @ D
    rows = []

    def add(kind, i, j, ref, g):
        lo, hi = pb.lineq[ref], pb.uineq[ref]
        if np.isfinite(lo) or np.isfinite(hi):
            rows.append((kind, i, j, ref, lo, hi, g))
    for i in range(ph + 1):
        for j in range(nx):
            add(0, i, j, i * d.na + j, Sx[i][j])
        if i == 0:                              # (step 0: state, output, scalar; the input box of step 0 bounds lastU, no general row)
            for j in range(ny):
                add(1, 0, j, d.off_y + j, np.zeros(nz))
            add(2, 0, 0, d.off_s, np.zeros(nz))
            continue
        for j in range(ny):
            add(1, i, j, d.off_y + i * ny + j, C[j] @ Sx[i])
        add(2, i, 0, d.off_s + i, pb.sX @ Sx[i] + pb.sU @ E(i))
        if i - 1 <= ch:
            for j in range(nu):
                add(3, i, j, d.off_du + (i - 1) * nu + j, (E(i) - (E(i - 1) if i > 1 else 0.0))[j])
    keep, fixed = [], 0
    for kind, i, j, ref, lo, hi, g in rows:
        w = weight.get(ref)
        if np.abs(g).max(initial=0.0) < 1e-14 and w is None:
            fixed += i > 0                      # (hard step-0 rows are feasibility rows of their own, not counted among the fixed rows)
            continue
        keep.append((kind, i, j, d.neq + ref, lo, hi, g, 0.0 if w is None else 1.0 / w))
    col = lambda k: np.array([r[k] for r in keep])
    return dict(H=H, G=np.array([r[6] for r in keep]).reshape(len(keep), nz), lo=col(4), hi=col(5), kind=col(0).astype(int), step=col(1).astype(int),
                comp=col(2).astype(int), refrow=col(3).astype(int), g_soft=col(7), fixed=fixed)


# ---------------------------------------------------------------------------------------------
# the cases of the GPU tests
# ---------------------------------------------------------------------------------------------
def integrator_soft(ph=10, rho=10.0, vmax=0.3, ch=None, reach=True):
    """the double integrator of rate_ref (input box +-1, no rate bounds) with a soft velocity bound +-vmax on steps 0 .. ph; reach=False: the
    input does not reach the position within a step (B = [0; dt]), so that the position row of step 1 has no coefficients"""
    sp = RR.integrator_spec(ph=ph, rate=None, box=1.0)
    if ch is not None:
        sp["dims"] = (2, 1, 0, 1, ph, ch)
    if not reach:
        sp["B"] = np.array([[0.0], [0.1]])
    sp.update(xmin=np.array([-INF, -vmax]), xmax=np.array([INF, vmax]))
    return with_soft(sp, xw=[INF, rho])


def full_feature_soft():
    """rate_ref.full_feature_spec with its state, output and scalar rows soft at three different weights; box and rate rows hard"""
    return with_soft(RR.full_feature_spec(), xw=[100.0, INF, INF, INF], yw=[10.0, 10.0], sw=50.0)


LARGE_RHO = 10.0


def large_case():
    """ph = 40, ch = 2: three decision variables and 41 soft velocity rows, the velocity of x0 three times the bound -- more active rows than
    a working set could hold before there were soft rows.  Its yardstick solves take seconds each: recorded by
    tests/golden/make_soft_golden.py"""
    sp = integrator_soft(ph=40, rho=LARGE_RHO, ch=2)
    # (the reference is at position 1: an instance far from it on the side it moves towards keeps its velocity as high as the penalty lets it)
    x0 = np.array([[-5.0, 0.9], [7.0, -0.9], [-3.0, 0.9], [-8.0, 0.9]])
    return sp, x0, np.zeros((4, 1))


def singular_soft(rho=10.0):
    """integrator_soft without input and delta-u weights and without an output weight on the last step (helpers.axes_spec's zero_weight): the
    condensed Hessian is singular, the set-up regularises it and the cost is taken from its definition -- the penalty has to be added there"""
    sp = integrator_soft(rho=rho)
    sp["UW"] = np.zeros((1, 10)); sp["DUW"] = np.zeros((1, 10)); sp["OW"] = sp["OW"].copy(); sp["OW"][:, -1] = 0.0
    return sp
