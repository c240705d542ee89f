"""Reference for the sensitivities of a solved batch, numpy only.

kkt_jacobian differentiates the KKT system of the reference's sparse QP (oracle.lmpc_numpy.ProblemBuilderRef through the rate_ref, soft_ref,
terminal_ref and linear_ref builders) on an active set: with W the equality rows and the active rows,
    [[P, A_W'], [A_W, 0]] [dz; dy] = [-dq; db_W]
where dq and db_W are differences of the builder's own q, l, u at unit steps of x0, lastU and an output reference shifted by the same amount
at every step.  Those are affine in the three, so the differences are exact.  It knows nothing of the condensed problem.

condensed_jacobian restates the kernel's formula in float64 numpy on the arrays of mpcx_lmpc_debug_get of a host-only handle.

RESTATEMENT_WORST is the worst err / max(1, max|J|) of condensed_jacobian against kkt_jacobian over the families of tests/test_lmpc_sens.py
(measured there, on the CPU); the kernel is held to KERNEL_TOL = max(8 x that, 1e-12) everywhere -- a figure of the restatement against the
truth, not of the kernel (the convention of the condensing kernel's tests)."""
import numpy as np

import linear_ref as LR
import rate_ref as RR
import soft_ref as SR
import terminal_ref as TR

RESTATEMENT_WORST = 5.3e-12            # soft family (measured 5.24e-12); the others are at 3e-13 and below
KERNEL_TOL = max(8.0 * RESTATEMENT_WORST, 1e-12)
SKIP_CAP = 0.10                       # the most of a batch a test may leave out as unusable


def builder(sp):
    """the most general of the reference builders: rate rows, slack columns, linear rows, terminal weight"""
    pb = LR.LinearBuilder(sp)
    if sp.get("box_all"):
        # the input box on every step, past the control horizon too (rate_ref.builder stops at ch): with move blocking several reference
        # rows then bound one condensed variable.  Row block i takes input-bound column min(i, ph - 1), so every block gets the box
        base, na, nx = pb.base, pb.d.na, sp["dims"][0]
        for i in range(sp["dims"][4] + 1):
            base.lineq[i * na + nx:(i + 1) * na] = sp["umin"]; base.uineq[i * na + nx:(i + 1) * na] = sp["umax"]
    return pb


def solve_batch(sp, x0, u0, yref=None, dmeas=None, **kw):
    """the oracle's solve on that builder (with 'y', which usable() needs); LR.solve_batch builds its own, so box_all goes through here"""
    if not sp.get("box_all"):
        return LR.solve_batch(sp, x0, u0, yref, dmeas, **kw)
    pb = builder(sp)
    d = pb.d
    parts = [RR.solve_one(pb, sp, x0[b], u0[b], None if yref is None else yref[b], None if dmeas is None else dmeas[b]) for b in range(len(x0))]
    res = {"neq": d.neq, "ncon": d.ncon, "ncon_ref": pb.ncon_ref, "nc": pb.nc}
    for k in ("cmd", "input", "y", "active_lower", "active_upper"):
        res[k] = np.stack([p[k] for p in parts])
    res["cost"] = np.array([p["cost"] for p in parts])
    for k in ("status", "solver_status", "iters", "polished", "is_feasible"):
        res[k] = np.array([int(p[k]) for p in parts], dtype=np.int32)
    for k in ("active_lower", "active_upper"):
        res[k][:, d.neq:d.neq + d.na] = 0          # the box rows of step 0 bound data, not decisions
    res["n_active"] = ((res["active_lower"] != 0) | (res["active_upper"] != 0))[:, d.neq:].sum(axis=1)
    res["n_linear_active"] = np.zeros(len(x0), int)
    return res


def _qlu(pb, sp, x0, u0, yR, dM):
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    q, l, u = pb.get(np.asarray(x0, float), np.asarray(u0, float), yR, sp["uref"], sp["duref"], dM)
    if "P" in sp:
        o = ph * pb.d.na
        q = q.copy()
        q[o:o + nx] -= 0.5 * (sp["P"] + sp["P"].T) @ TR.target(sp, yR, dM)
    return q, l, u


def _diff(a, b):
    with np.errstate(invalid="ignore"):
        d = a - b
    return np.where(np.isfinite(d), d, 0.0)             # an infinite bound does not move


def kkt_jacobian(pb, sp, x0, u0, yref, active_lower, active_upper, dmeas=None):
    """dict(cmd [nu x nin], input [(ph + 1) x nu x nin], residual, full_rank) with nin = nx + nu + ny columns (x0 | lastU | yref).  yref: None
    (the controller's), [ny] or [ny, ph]; active_*: [ncon] flags in the builder's row numbering"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = pb.d
    na = d.na
    yR = sp["yref"] if yref is None else (np.tile(np.asarray(yref, float)[:, None], (1, ph)) if np.ndim(yref) == 1 else np.asarray(yref, float))
    dM = sp.get("dmeas", np.zeros((ndu, ph))) if dmeas is None else np.asarray(dmeas, float)
    x0 = np.asarray(x0, float); u0 = np.asarray(u0, float)
    nin = nx + nu + ny
    q0, l0, u0b = _qlu(pb, sp, x0, u0, yR, dM)
    dq = np.zeros((len(q0), nin)); dl = np.zeros((len(l0), nin)); du = np.zeros((len(l0), nin))
    for k in range(nin):
        x1, v1, y1 = x0.copy(), u0.copy(), yR.copy()
        if k < nx:
            x1[k] += 1.0
        elif k < nx + nu:
            v1[k - nx] += 1.0
        else:
            y1[k - nx - nu, :] += 1.0
        q1, l1, u1 = _qlu(pb, sp, x1, v1, y1, dM)
        dq[:, k] = q1 - q0; dl[:, k] = _diff(l1, l0); du[:, k] = _diff(u1, u0b)
    lo = np.asarray(active_lower).astype(bool); up = np.asarray(active_upper).astype(bool)
    act = lo | up
    act[:d.neq] = False
    W = np.concatenate([np.arange(d.neq), np.nonzero(act)[0]])
    db = np.where(lo[W, None] & ~up[W, None], dl[W], du[W])
    db[:d.neq] = dl[:d.neq]
    n = pb.P.shape[0]
    AW = pb.A[W]
    K = np.block([[pb.P, AW.T], [AW, np.zeros((len(W), len(W)))]])
    rhs = np.vstack([-dq, db])
    sol = np.linalg.lstsq(K, rhs, rcond=None)[0]
    residual = float(np.abs(K @ sol - rhs).max())
    full_rank = np.linalg.matrix_rank(np.vstack([pb.P, AW])) == n
    dz = sol[:n]
    # LN.unpack_solution's linear part: row i of the sequence is the x_u block of xi_{min(i + 1, ph)}; cmd is row 0
    dinput = np.stack([dz[min(i + 1, ph) * na + nx:(min(i + 1, ph) + 1) * na] for i in range(ph + 1)])
    return dict(cmd=dinput[0].copy(), input=dinput, residual=residual, full_rank=bool(full_rank))


def good(jac):
    return jac["full_rank"] and jac["residual"] <= 1e-10


def usable(res, b):
    """polished, SUCCESS, strict complementarity: every active multiplier at least 1e-6 max(1, |y|_inf)"""
    if not (res["polished"][b] == 1 and res["status"][b] == 0):
        return False
    y = res["y"][b]
    act = (res["active_lower"][b] != 0) | (res["active_upper"][b] != 0)
    act[:res["neq"]] = False
    return bool(np.all(np.abs(y[act]) >= 1e-6 * max(1.0, np.abs(y).max(initial=0.0))))


# ---------------------------------------------------------------------------------------------
# the kernel's formula on the product's own arrays
# ---------------------------------------------------------------------------------------------
def arrays(c):
    """what condensed_jacobian and the emulator runner read of a controller (a host-only handle serves)"""
    dm = c.debug_get("dims"); df = c.debug_get("dims_fused")
    a = dict(nx=c.nx, nu=c.nu, ny=c.ny, ph=c.ph, nz=int(dm[0]), mg=int(dm[1]), ldz=int(dm[2]), ldg=int(dm[3]), ldy=int(dm[4]),
             rowsF=int(df[0]), kin=int(df[2]), nxp=int(df[3]), nup=int(df[4]), nyp=int(df[5]))
    a["Y"] = c.debug_get("Y").reshape(a["ldy"], a["ldy"]).T                  # column-major
    a["MF1"] = c.debug_get("MF1").reshape(a["kin"], a["rowsF"]).T
    for n in ("g_refrow", "boxrow_ptr", "boxrow_ref", "blk"):
        a[n] = c.debug_get(n).astype(int)
    return a


def working_set(a, act):
    """unified indices (box variable e -> e, general row r -> ldz + r) of the rows whose bit is set in `act` [reference rows]"""
    act = np.asarray(act).astype(bool)
    bit = lambda r: 0 <= r < len(act) and act[r]
    A = [e for e in range(a["nz"]) if any(bit(r) for r in a["boxrow_ref"][a["boxrow_ptr"][e]:a["boxrow_ptr"][e + 1]])]
    A += [a["ldz"] + r for r in range(a["mg"]) if bit(a["g_refrow"][r])]
    return np.array(A, int)


def input_columns(a):
    return np.concatenate([np.arange(a["nx"]), a["nxp"] + np.arange(a["nu"]), a["nxp"] + a["nup"] + np.arange(a["ny"])])


def condensed_jacobian(a, active_lower, active_upper):
    """dict(cmd [nu x nin], input [(ph + 1) x nu x nin], n = rows of the working set, dependent)"""
    nz, ldz, ldy, nu, ph = a["nz"], a["ldz"], a["ldy"], a["nu"], a["ph"]
    A = working_set(a, np.asarray(active_lower).astype(bool) | np.asarray(active_upper).astype(bool))
    cols = input_columns(a)
    T0 = a["MF1"][:nz][:, cols]
    dw = T0.copy()
    dependent = False
    if len(A):
        gen = A >= ldz
        NT = a["MF1"][A][:, cols]
        NT[gen] += a["MF1"][ldy + (A[gen] - ldz)][:, cols]                  # the bounds of a general row move by -goff
        S = a["Y"][np.ix_(A, A)]                                             # (a soft row's 1 / weight is on Y's diagonal already)
        try:
            L = np.linalg.cholesky(S)
            dependent = bool((np.diag(L) ** 2 <= 1e-11 * np.diag(S)).any())
        except np.linalg.LinAlgError:
            dependent = True
        if not dependent:
            dw = T0 - a["Y"][:nz][:, A] @ np.linalg.solve(S, NT)
    blk = a["blk"]
    dinput = np.stack([dw[blk[min(i + 1, ph)] * nu:(blk[min(i + 1, ph)] + 1) * nu] for i in range(ph + 1)])
    if dependent:
        dinput = np.full_like(dinput, np.nan)
    return dict(cmd=dinput[0].copy(), input=dinput, n=len(A), dependent=dependent)


def split(J, nx, nu):
    """[.. x nin] -> the blocks of x0, lastU, yref"""
    return J[..., :nx], J[..., nx:nx + nu], J[..., nx + nu:]


def pack_bits(flags, words):
    """[B x rows] flags -> [B x words] int32 words as the solve writes them"""
    flags = np.asarray(flags).astype(bool)
    out = np.zeros((flags.shape[0], words), np.uint32)
    for r in range(flags.shape[1]):
        out[:, r >> 5] |= flags[:, r].astype(np.uint32) << np.uint32(r & 31)
    return out.view(np.int32)


# ---------------------------------------------------------------------------------------------
# the families of the tests: name -> (spec, x0, u0, yref [B, ny])
# ---------------------------------------------------------------------------------------------
def _batch(sp, B, seed, yscale, xscale):
    x0, u0, yref = RR.random_batch(sp, B, seed, yscale=yscale)
    return sp, xscale * x0, u0, yref


def family(name, B=32):
    if name == "smallest":                       # nz = 1, nothing active
        sp = RR.rate_spec(41, 1, 1, 0, 1, 1, 1, rate=100.0)
        return _batch(sp, 16, 3, 1.0, 1.0)
    if name in ("nz15", "nz16", "nz17"):         # the row-tile and k-step edges of the shared product: nz = 15, 16, 17; nx = 3, 4, 5
        nu, ph, nx = {"nz15": (3, 5, 3), "nz16": (4, 4, 4), "nz17": (17, 1, 5)}[name]     # (17 inputs: more seeds than a column tile as well)
        sp = RR.rate_spec(50 + nx, nx, nu, 0, 2, ph, ph, rate=0.3, box=0.6)
        return _batch(sp, 16, 4, 1.0, 0.5)
    if name == "full":
        # the batch the approach was checked on, and four instances whose last input lies near the box, so that a first move ends pinned on it
        sp, x0, u0, yref = _batch(RR.full_feature_spec(), B, 5, 1.5, 0.3)
        near = 0.47 * np.array([[-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0], [1.0, 1.0]])
        pick = [0, 2, 6, 7]
        return sp, np.vstack([x0, x0[pick]]), np.vstack([u0, near]), np.vstack([yref, yref[pick]])
    if name == "soft":
        return _batch(SR.full_feature_soft(), B, 6, 1.5, 0.6)
    if name == "linear":
        sp = LR.random_rows(RR.full_feature_spec(), 2, 33, size=1.0, steps=range(1, 11), onesided=False)
        return _batch(sp, B, 5, 1.5, 0.3)
    if name == "blocked":                        # ch < ph - 1: several reference rows on one variable
        sp = RR.rate_spec(61, 3, 2, 0, 2, 8, 3, rate=1.0, box=1.2)
        sp["box_all"] = True
        return _batch(sp, B, 9, 1.5, 0.5)
    if name == "terminal":
        return _batch(TR.full_feature_terminal(), B, 9, 1.5, 0.3)
    raise KeyError(name)


FAMILIES = ("smallest", "nz15", "nz16", "nz17", "full", "soft", "linear", "blocked", "terminal")


def configure(c, sp):
    LR.configure(c, sp)
    if sp.get("box_all"):
        ch = sp["dims"][5]                     # (the matrix form: its last column fills the steps past the control horizon)
        assert c.setInputBounds(np.tile(sp["umin"][:, None], (1, ch)), np.tile(sp["umax"][:, None], (1, ch)))
    return c


def reference(name):
    """the oracle's solve of a family and the KKT Jacobian of every usable instance: dict(sp, x0, u0, yref, res, jac [B] (None: unusable), pb)"""
    sp, x0, u0, yref = family(name)
    res = solve_batch(sp, x0, u0, yref)
    pb = builder(sp)
    jac = []
    for b in range(len(x0)):
        j = kkt_jacobian(pb, sp, x0[b], u0[b], yref[b], res["active_lower"][b], res["active_upper"][b]) if usable(res, b) else None
        jac.append(j if j is not None and good(j) else None)
    return dict(sp=sp, x0=x0, u0=u0, yref=yref, res=res, jac=jac, pb=pb)


def solve_one(pb, sp, x0, u0, yref):
    """one oracle solve on builder(sp), the step-0 box bits cleared as in solve_batch"""
    r = (TR.solve_one if "P" in sp else RR.solve_one)(pb, sp, x0, u0, yref)
    d = pb.d
    for k in ("active_lower", "active_upper"):
        r[k] = r[k].copy()
        soft = [d.neq + row for row, _ in pb.base.rows] if "soft" in sp else []
        keep = r[k][soft].copy()
        r[k][d.neq:d.neq + d.na] = 0
        r[k][soft] = keep
        r[k][[pb.row0 + c for c in range(pb.nc) if c not in {row for row, _ in pb.soft}]] = 0
    return r
