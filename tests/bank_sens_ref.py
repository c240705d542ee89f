"""Reference for the sensitivities of a solved batch of a bank, numpy only.

The truth is sens_ref.kkt_jacobian: the QP of a bank member is the QP of its own controller, so every instance is differentiated on the
reference builder of the controller it was solved with.

rollout_jacobian restates the kernel's formula in float64 numpy on the arrays of mpcx_lmpc_debug_get of a host-only handle.  A bank carries no
composed affine maps, so the formula is 4.8's without MF1: for a cotangent p on w and the working set A
    mu = S^-1 Y[A, 0:nz] p,  S = Y[A, A];    q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu
    g  = -F' q - OFF[A, :]' mu               F = df/dvin, OFF = d(offset of a general row)/dvin: its bounds are lg0 - off, ug0 - off
and both products are the adjoint of the linear part of the roll-out that assembles f and the offsets (lmpc_assemble_generic):
    dv_i = q[blk[i] nu + .],  dx_0 = 0,  dx_i = A dx_{i-1} + B dv_i,  dy_i = C dx_i                          i = 1 .. ph
    do_i  = Wy_i dy_i                                              (the cost's part; d_yref sums it)
    gam_i = C' (do_i + output rows' mu_r e_comp) + state rows' mu_r e_comp + scalar rows' mu_r sX + linear rows' mu_r Fx[c, :] + [i = ph] P dx_ph
    eta_ph = gam_ph,  eta_i = gam_i + A' eta_{i+1}
    d_x0   = -A' eta_1 - gam_0               (gam_0: the rows of step 0 that carry a slack variable; it has no cost term)
    d_yref = sum_i do_i + Tx[:, 0:ny]' P dx_ph
    d_u0   = Wdu[:, 0] * dv_1 + sum over the rate rows of step 1 of mu_r e_comp - sum over the scalar / linear rows of step 0 of mu_r sU / Fu[c, :]

BANK_RESTATEMENT_WORST is the worst err / max(1, max|J|) of rollout_jacobian against kkt_jacobian over the usable instances of FAMILIES
(measured by tests/test_lmpc_bank_sens.py, on the CPU); the kernel is held to BANK_KERNEL_TOL = max(8 x that, 1e-12) everywhere -- a figure of
the restatement against the truth, not of the kernel (the convention of sens_ref.py)."""
import functools

import numpy as np

import linear_ref as LR
import rate_ref as RR
import sens_ref as S
import soft_ref as SR
import terminal_ref as TR

BANK_RESTATEMENT_WORST = 1.7e-12       # soft family (measured 1.62e-12); linear 8.2e-13, the others at 1.6e-13 and below
BANK_KERNEL_TOL = max(8.0 * BANK_RESTATEMENT_WORST, 1e-12)
SKIP_CAP = S.SKIP_CAP

G_STATE, G_OUTPUT, G_SCALAR, G_RATE, G_LINEAR = range(5)
PER_CONTROLLER = 4                     # instances of every controller, in shuffled order

# The controllers' seeds, chosen on the CPU so that the oracle alone leaves at least 90 % of every family usable (polished, strictly
# complementary, a KKT solve that passes sens_ref.good): the obvious runs of seeds do not.
SEEDS = {
    "smallest": (41, 42, 43, 44),
    "nz15": (53, 54, 55, 56, 58, 59, 60, 61),
    "nz16": (54, 55, 56, 57, 58, 59, 60, 61),
    "nz17": (55, 56, 57, 58, 59, 60, 61, 62),
    "full": (300, 301, 303, 305, 306, 308, 309, 310),
    "soft": (300, 301, 303, 305, 306, 308, 310, 311),
    "linear": (300, 301, 306, 308, 309, 311, 315, 316),
    "blocked": (66, 69, 73, 77, 80, 82, 84, 90),
    "terminal": (300, 301, 303, 305, 306, 308, 309, 310),
}
FAMILIES = S.FAMILIES


def full_member(seed):
    """rate_ref.full_feature_spec's recipe with another seed"""
    sp = RR.rate_spec(seed, 4, 2, 1, 2, 10, 10, rate=0.15, vary=True, box=0.5, state=True, output=True, scalar=True)
    sp["xmin"][0] = -1.0; sp["xmax"][0] = 1.0; sp["ymin"][:] = -1.2; sp["ymax"][:] = 1.2; sp["smin"] = -1.0; sp["smax"] = 1.0
    sp["first"] = 1
    return sp


def member(name, seed):
    """controller `seed` of a family: equal dimensions and an equal pattern of finite bounds within the family"""
    if name == "smallest":
        return RR.rate_spec(seed, 1, 1, 0, 1, 1, 1, rate=100.0)
    if name in ("nz15", "nz16", "nz17"):
        nu, ph, nx = {"nz15": (3, 5, 3), "nz16": (4, 4, 4), "nz17": (17, 1, 5)}[name]
        return RR.rate_spec(seed, nx, nu, 0, 2, ph, ph, rate=0.3, box=0.6)
    if name == "full":
        return full_member(seed)
    if name == "soft":
        return SR.with_soft(full_member(seed), xw=[100.0, np.inf, np.inf, np.inf], yw=[10.0, 10.0], sw=50.0)
    if name == "linear":
        return LR.random_rows(full_member(seed), 2, 1000 + seed, size=1.0, steps=range(1, 11), onesided=False)
    if name == "blocked":
        sp = RR.rate_spec(seed, 3, 2, 0, 2, 8, 3, rate=1.0, box=1.2)
        sp["box_all"] = True
        return sp
    if name == "terminal":
        sp = full_member(seed)
        nx, nu, ndu, ny, ph, ch = sp["dims"]
        r = np.random.default_rng(2000 + seed)
        F = r.normal(size=(nx, nx - 1))
        return TR.with_terminal(sp, 2.0 * F @ F.T, xT=0.2 * r.normal(size=nx), Tx=0.3 * r.normal(size=(nx, ny + ndu)))
    raise KeyError(name)


_BATCH = {"smallest": (3, 1.0, 1.0), "nz15": (4, 1.0, 0.5), "nz16": (4, 1.0, 0.5), "nz17": (4, 1.0, 0.5), "full": (5, 1.5, 0.3), "soft": (6, 1.5, 0.6),
          "linear": (5, 1.5, 0.3), "blocked": (9, 1.5, 0.5), "terminal": (9, 1.5, 0.3)}      # batch seed, yref scale, x0 scale: sens_ref.family's


def family(name, seeds=None):
    """dict(specs [K], model [B] controller of every instance (each controller PER_CONTROLLER times, shuffled), x0, u0, yref [B, .])"""
    seeds = SEEDS[name] if seeds is None else tuple(seeds)
    specs = [member(name, s) for s in seeds]
    K = len(specs)
    model = np.random.default_rng(7).permutation(np.repeat(np.arange(K), PER_CONTROLLER))
    bseed, yscale, xscale = _BATCH[name]
    x0, u0, yref = RR.random_batch(specs[0], K * PER_CONTROLLER, bseed, yscale=yscale)
    return dict(specs=specs, model=model, x0=xscale * x0, u0=u0, yref=yref)


def reference_of(fam):
    """the oracle's solve of every instance on its own controller and the KKT Jacobian of every usable one: the family's dict plus
    active_lower, active_upper [B, rows], status [B], jac [B] (None: unusable), pbs [K]"""
    specs, model, x0, u0, yref = (fam[k] for k in ("specs", "model", "x0", "u0", "yref"))
    B = len(model)
    out = dict(fam)
    out["pbs"] = [S.builder(sp) for sp in specs]
    al, au, status, jac = [None] * B, [None] * B, np.zeros(B, np.int32), [None] * B
    for k, sp in enumerate(specs):
        idx = np.nonzero(model == k)[0]
        res = S.solve_batch(sp, x0[idx], u0[idx], yref[idx])
        for t, b in enumerate(idx):
            al[b], au[b], status[b] = res["active_lower"][t], res["active_upper"][t], res["status"][t]
            if S.usable(res, t):
                j = S.kkt_jacobian(out["pbs"][k], sp, x0[b], u0[b], yref[b], al[b], au[b])
                jac[b] = j if S.good(j) else None
    out.update(active_lower=np.stack(al), active_upper=np.stack(au), status=status, jac=jac)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(family(name))


def usable_share(R):
    return sum(j is not None for j in R["jac"]) / len(R["jac"])


def configure(c, sp):
    return S.configure(c, sp)


# ---------------------------------------------------------------------------------------------
# the kernel's formula on the product's own arrays
# ---------------------------------------------------------------------------------------------
def arrays(c):
    """what rollout_jacobian and the emulator runner read of a controller (a host-only handle serves; MF1 is there for condensed_jacobian only)"""
    a = S.arrays(c)
    nx, nu, ny, ph = a["nx"], a["nu"], a["ny"], a["ph"]
    ndu = a["ndu"] = c.ndu
    model = c.debug_get("model")                                                      # A | B | C | Bd | Dd, column-major
    o = 0
    for n, r, k in (("A", nx, nx), ("B", nx, nu), ("C", ny, nx)):
        a[n] = model[o:o + r * k].reshape(k, r).T.copy()
        o += r * k
    a["Wy"] = c.debug_get("wOutput").reshape(ph + 1, ny).T                            # internal columns: stage i
    a["Wdu"] = c.debug_get("wDeltaU").reshape(ph, nu).T
    sc = c.debug_get("scalar")                                                        # sX | row c: Fx(c, :), Fu(c, :)
    a["scalar"] = sc
    a["sX"] = sc[:nx]
    a["sU"] = c.debug_get("sU")
    nc = a["nc"] = (len(sc) - nx) // (nx + nu)
    F = sc[nx:].reshape(nc, nx + nu)
    a["Fx"], a["Fu"] = F[:, :nx], F[:, nx:]
    for n in ("g_kind", "g_step", "g_comp"):
        a[n] = c.debug_get(n).astype(int)
    a["g_soft"] = c.debug_get("g_soft")
    t = c.debug_get("terminal")
    a["terminal_raw"] = t
    a["terminal"] = None
    if len(t):
        a["terminal"] = (t[:nx * nx].reshape(nx, nx).T, t[nx * nx:nx * nx + nx], t[nx * nx + nx:].reshape(ny + ndu, nx).T)
    return a


def cotangent(a, seed_cmd=None, seed_input=None):
    """p on w of one seed pair, scattered through blk as OptSequence reads the sequence"""
    nu, ph, blk = a["nu"], a["ph"], a["blk"]
    p = np.zeros(a["nz"])
    si = np.zeros((ph + 1, nu)) if seed_input is None else np.array(seed_input, float)
    if seed_cmd is not None:
        si[0] += seed_cmd
    for i in range(ph + 1):
        b = blk[min(i + 1, ph)]
        p[b * nu:(b + 1) * nu] += si[i]
    return p


def rollout_vjp(a, A, p):
    """g [nin] over the columns of x0, lastU, yref for the cotangent p on w and the working set A (unified indices); None: dependent"""
    nz, ldz, nx, nu, ny, ph, blk = a["nz"], a["ldz"], a["nx"], a["nu"], a["ny"], a["ph"], a["blk"]
    Y, Am, Bm, Cm = a["Y"], a["A"], a["B"], a["C"]
    q = Y[:nz, :nz] @ p
    mu = np.zeros(0)
    if len(A):
        Sm = Y[np.ix_(A, A)]
        try:
            L = np.linalg.cholesky(Sm)
        except np.linalg.LinAlgError:
            return None
        if (np.diag(L) ** 2 <= 1e-11 * np.diag(Sm)).any():
            return None
        mu = np.linalg.solve(Sm, Y[A][:, :nz] @ p)
        q = q - Y[:nz][:, A] @ mu
    dv = np.vstack([np.zeros(nu)] + [q[blk[i] * nu:(blk[i] + 1) * nu] for i in range(1, ph + 1)])
    dx = np.zeros((ph + 1, nx))
    for i in range(1, ph + 1):
        dx[i] = Am @ dx[i - 1] + Bm @ dv[i]
    do = np.stack([a["Wy"][:, i] * (Cm @ dx[i]) if i else np.zeros(ny) for i in range(ph + 1)])
    d_yref = do.sum(axis=0)
    d_u0 = a["Wdu"][:, 0] * dv[1]
    gam = np.zeros((ph + 2, nx))
    for k, e in enumerate(A):
        if e < ldz:
            continue
        rr = e - ldz
        kind, st, cp = a["g_kind"][rr], a["g_step"][rr], a["g_comp"][rr]
        if kind == G_OUTPUT:
            if st >= 1:
                do[st, cp] += mu[k]
            else:
                gam[0] += mu[k] * Cm[cp]
        elif kind == G_STATE:
            gam[st, cp] += mu[k]
        elif kind == G_SCALAR:
            gam[st] += mu[k] * a["sX"]
            if st == 0:
                d_u0 -= mu[k] * a["sU"]
        elif kind == G_LINEAR:
            gam[st] += mu[k] * a["Fx"][cp]
            if st == 0:
                d_u0 -= mu[k] * a["Fu"][cp]
        elif st == 1:                                   # the rate row of the first increment: v_1 - lastU
            d_u0[cp] += mu[k]
    if a["terminal"] is not None:
        Pm, _, Tx = a["terminal"]
        pdx = Pm @ dx[ph]
        gam[ph] += pdx
        d_yref = d_yref + Tx[:, :ny].T @ pdx
    eta = np.zeros(nx)
    for i in range(ph, 0, -1):
        eta = Cm.T @ do[i] + gam[i] + Am.T @ eta
    d_x0 = -(Am.T @ eta) - gam[0]
    return np.concatenate([d_x0, d_u0, d_yref])


def rollout_jacobian(a, active_lower, active_upper):
    """dict(cmd [nu x nin], input [(ph + 1) x nu x nin], n = rows of the working set, dependent): sens_ref.condensed_jacobian's result, without MF1"""
    nu, ph, blk, nz = a["nu"], a["ph"], a["blk"], a["nz"]
    A = S.working_set(a, np.asarray(active_lower).astype(bool) | np.asarray(active_upper).astype(bool))
    nin = a["nx"] + nu + a["ny"]
    dw = np.zeros((nz, nin))
    dependent = False
    for e in range(nz):
        p = np.zeros(nz); p[e] = 1.0
        g = rollout_vjp(a, A, p)
        if g is None:
            dependent = True
            break
        dw[e] = g
    dinput = np.stack([dw[blk[min(i + 1, ph)] * nu:(blk[min(i + 1, ph)] + 1) * nu] for i in range(ph + 1)])
    if dependent:
        dinput = np.full_like(dinput, np.nan)
    return dict(cmd=dinput[0].copy(), input=dinput, n=len(A), dependent=dependent)


def error(J, truth):
    """err / max(1, max|J|) of a cmd Jacobian against the truth's"""
    return np.abs(J - truth).max() / max(1.0, np.abs(truth).max())
