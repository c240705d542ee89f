"""Reference for the gradients of a solved batch of a bank with respect to the weights, the bounds and the model of each instance's controller
(DESIGN.md 4.10b), numpy only.

The truth is param_sens_ref.Truth and model_sens_ref.Truth: the QP of a bank member is the QP of its own controller, so every instance is
differentiated on the reference builders of the controller it was solved with, one Truth pair per controller.

rollout_gradients restates the kernel's formulas in float64 numpy on the arrays of mpcx_lmpc_debug_get of a host-only handle and on the optimum's
own sequences.  A bank has no shared operand, so the formulas are 4.9's and 4.10's with the products Cq q and Xq q replaced by the roll-out of q
through the controller's own model, as bank_sens_ref.rollout_vjp restates the data gradients:
    mu = S^-1 Y[A, 0:nz] p,  S = Y[A, A];    q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu
    dv_i = q[blk[i] nu + .],  dx_0 = 0,  dx_i = A dx_{i-1} + B dv_i,  dy_i = C dx_i                          i = 1 .. ph

BANK_GRAD_RESTATEMENT_WORST is the worst |restatement - truth| / max(1, max|truth|) over the usable instances of FAMILIES (measured by
tests/test_lmpc_bank_grad.py, on the CPU); the kernel is held to BANK_GRAD_KERNEL_TOL = max(8 x that, 1e-12) everywhere -- a figure of the
restatement against the truth, not of the kernel (the convention of sens_ref.py)."""
import functools

import numpy as np

import bank_sens_ref as BR
import model_sens_ref as Mo
import param_sens_ref as P
import rate_ref as RR
import sens_ref as S

# measured by test_restatement_matches_the_truth, worst usable instance of each family (parameter outputs | model outputs):
#   smallest 8.3e-15 | 5.6e-15   nz15 1.4e-13 | 1.5e-13   nz16 3.3e-13 | 2.2e-12   nz17 5.1e-13 | 5.8e-13   full 7.1e-14 | 8.9e-14
#   soft 2.7e-12 | 8.2e-13       linear 8.4e-13 | 7.2e-13 blocked 2.7e-14 | 7.1e-14 terminal 7.2e-14 | 1.6e-13 refs 2.7e-14 | 5.8e-14
#   ndu2 5.5e-14 | 1.0e-13       nx33 5.2e-15 | 1.7e-14   ow63 1.3e-13 | 1.9e-13   ow64 3.9e-14 | 8.8e-14   ow65 2.4e-14 | 3.2e-14
BANK_GRAD_RESTATEMENT_WORST = 2.8e-12   # soft family, the parameter outputs (measured 2.71e-12); nz16's model outputs follow at 2.19e-12
BANK_GRAD_KERNEL_TOL = max(8.0 * BANK_GRAD_RESTATEMENT_WORST, 1e-12)
SKIP_CAP = S.SKIP_CAP
PER_CONTROLLER = BR.PER_CONTROLLER

G_STATE, G_OUTPUT, G_SCALAR, G_RATE, G_LINEAR = range(5)
PARAM = P.WEIGHTS + ("lower", "upper")
MODEL = Mo.MODEL

# lane-stride edges of the kernel's loops: rows of d_oweight of 63, 64 and 65 entries, (nx, nu, ny, ph)
EDGE = {"ow63": (3, 2, 7, 9), "ow64": (3, 2, 8, 8), "ow65": (3, 2, 5, 13)}
FAMILIES = BR.FAMILIES + ("refs", "ndu2", "nx33") + tuple(EDGE)

# The controllers' seeds: bank_sens_ref.SEEDS re-checked against this module's leave-out rule (the oracle's polish and strict complementarity,
# and both truths' own KKT solve), which they pass as they are; those of the new families chosen the same way, on the CPU.
SEEDS = dict(BR.SEEDS)
SEEDS.update(refs=(81, 82, 86, 87), ndu2=(143, 144, 145, 146), nx33=(133, 134), ow63=(77, 78, 79, 80), ow64=(79, 80, 81, 82), ow65=(75, 76))
# (instances the oracle alone leaves usable, instances with both truths) of every family, all of its K x PER_CONTROLLER everywhere
# (test_restatement_matches_the_truth re-checks them and the cap); nx33 and ow65 have two controllers: their truths are the costly ones
USABLE = {"smallest": (16, 16), "nz15": (32, 32), "nz16": (32, 32), "nz17": (32, 32), "full": (32, 32), "soft": (32, 32), "linear": (32, 32),
          "blocked": (32, 32), "terminal": (32, 32), "refs": (16, 16), "ndu2": (16, 16), "nx33": (8, 8), "ow63": (16, 16), "ow64": (16, 16),
          "ow65": (8, 8)}

_BATCH = dict(BR._BATCH, refs=(24, 1.0, 0.5), ndu2=(39, 1.0, 0.5), nx33=(34, 1.0, 0.5), ow63=(21, 1.0, 0.5), ow64=(22, 1.0, 0.5), ow65=(23, 1.0, 0.5))


def member(name, seed):
    """controller `seed` of a family: equal dimensions and an equal pattern of finite bounds within the family"""
    if name in BR.FAMILIES:
        return BR.member(name, seed)
    if name == "refs":                           # input and rate references that differ from step to step, and from controller to controller
        sp = RR.rate_spec(seed, 3, 2, 0, 2, 6, 6, rate=0.3, box=0.6)
        r = np.random.default_rng(1000 + seed)
        sp["uref"] = 0.2 * r.normal(size=(2, 6)); sp["duref"] = 0.05 * r.normal(size=(2, 6))
        return sp
    if name == "ndu2":                           # two exogenous inputs that differ from step to step
        return RR.rate_spec(seed, 3, 2, 2, 2, 6, 6, rate=0.3, box=0.6, output=True)
    if name == "nx33":                           # a state longer than half a wavefront
        return RR.rate_spec(seed, 33, 1, 0, 1, 2, 2, rate=0.3, box=0.6)
    nx, nu, ny, ph = EDGE[name]
    return RR.rate_spec(seed, nx, nu, 0, ny, ph, ph, rate=0.3, box=0.6)


def family(name, seeds=None):
    """dict(specs [K], model [B] controller of every instance (each controller PER_CONTROLLER times, shuffled), x0, u0, yref [B, .])"""
    seeds = SEEDS[name] if seeds is None else tuple(seeds)
    specs = [member(name, s) for s in seeds]
    K = len(specs)
    model = np.random.default_rng(7).permutation(np.repeat(np.arange(K), PER_CONTROLLER))
    bseed, yscale, xscale = _BATCH[name]
    x0, u0, yref = RR.random_batch(specs[0], K * PER_CONTROLLER, bseed, yscale=yscale)
    return dict(specs=specs, model=model, x0=xscale * x0, u0=u0, yref=yref)


class Truths:
    """the two truths of one controller, built once"""

    def __init__(self, sp):
        self.sp, self.param, self.model = sp, P.Truth(sp), Mo.Truth(sp)

    def gradients(self, x0, u0, yref, active_lower, active_upper, seed_cmd=None, seed_input=None):
        """the gradients of both truths in one dict, or None where either truth's own KKT solve fails its residual or full_rank check"""
        tp = self.param.gradients(x0, u0, yref, active_lower, active_upper, seed_cmd, seed_input)
        tm = self.model.gradients(x0, u0, yref, active_lower, active_upper, seed_cmd, seed_input)
        if not (S.good(tp) and S.good(tm)):
            return None
        out = {k: tp[k] for k in PARAM}
        out.update({k: tm[k] for k in MODEL if k in tm})
        return out


def sequences(sp, x0, inp):
    """seq_state, seq_output of the input sequence as the solve writes them"""
    return Mo.rollout(sp, x0, inp)


def reference_of(fam, seed=17):
    """the oracle's solve of every instance on its own controller, one random seed pair per instance and the truth of every usable one: the
    family's dict plus active_lower, active_upper [B, rows], status [B], input [B, ph + 1, nu], seq_state, seq_output, truth [B] (None: left
    out), usable_oracle (instances the oracle alone leaves usable), seed_cmd, seed_input, truths [K]"""
    specs, model, x0, u0, yref = (fam[k] for k in ("specs", "model", "x0", "u0", "yref"))
    B = len(model)
    nx, nu, ndu, ny, ph, ch = specs[0]["dims"]
    out = dict(fam)
    out["truths"] = [Truths(sp) for sp in specs]
    rg = np.random.default_rng(seed)
    sc, sq = rg.normal(size=(B, nu)), rg.normal(size=(B, ph + 1, nu))
    al, au, status, inp, truth = [None] * B, [None] * B, np.zeros(B, np.int32), [None] * B, [None] * B
    ok = 0
    for k, sp in enumerate(specs):
        idx = np.nonzero(model == k)[0]
        res = S.solve_batch(sp, x0[idx], u0[idx], yref[idx])
        for t, b in enumerate(idx):
            al[b], au[b], status[b], inp[b] = res["active_lower"][t], res["active_upper"][t], res["status"][t], res["input"][t]
            if S.usable(res, t):
                ok += 1
                truth[b] = out["truths"][k].gradients(x0[b], u0[b], yref[b], al[b], au[b], sc[b], sq[b])
    seqs = [sequences(specs[model[b]], x0[b], inp[b]) for b in range(B)]
    out.update(active_lower=np.stack(al), active_upper=np.stack(au), status=status, input=np.stack(inp), seq_state=np.stack([s[0] for s in seqs]),
               seq_output=np.stack([s[1] for s in seqs]), truth=truth, usable_oracle=ok, seed_cmd=sc, seed_input=sq)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(family(name))


def usable_counts(R):
    """(instances the oracle alone leaves usable, instances with a truth) of a reference"""
    return R["usable_oracle"], sum(t is not None for t in R["truth"])


configure = BR.configure


# ---------------------------------------------------------------------------------------------
# the kernel's formulas on the product's own arrays
# ---------------------------------------------------------------------------------------------
def arrays(c):
    """what rollout_gradients and the emulator runner read of a controller (a host-only handle serves): bank_sens_ref.arrays and the input
    weights, the disturbance matrices, the soft rows and their bounds, the rows the active words name"""
    a = BR.arrays(c)
    nx, nu, ny, ndu, ph = a["nx"], a["nu"], a["ny"], a["ndu"], a["ph"]
    model = c.debug_get("model")
    o = nx * nx + nx * nu + ny * nx
    a["Bd"] = model[o:o + nx * ndu].reshape(ndu, nx).T.copy()
    a["Dd"] = model[o + nx * ndu:o + nx * ndu + ny * ndu].reshape(ndu, ny).T.copy()
    a["Wu"] = c.debug_get("wU").reshape(ph + 1, nu).T
    a["lg0"], a["ug0"] = c.debug_get("lg0"), c.debug_get("ug0")
    a["m_rows"] = c.info()["m_ref"]
    return a


def own_references(sp):
    """yref is the instance's; the others are the controller's own, [n x ph]"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    return sp["uref"], sp["duref"], sp.get("dmeas", np.zeros((ndu, ph)))


def rollout_gradients(a, active_lower, active_upper, u0, seq_state, seq_output, seq_input, yref, uref, duref, dmeas, seed_cmd=None, seed_input=None,
                      want_model=True):
    """dict(OW, UW, DUW, lower, upper [m_rows], A, B, C, Bd, Dd, n, dependent); yref [ny x ph], uref, duref [nu x ph], dmeas [ndu x ph] are the
    references of the instance, column = step"""
    nz, ldz, nx, nu, ny, ndu, ph, blk = a["nz"], a["ldz"], a["nx"], a["nu"], a["ny"], a["ndu"], a["ph"], a["blk"]
    Am, Bm, Cm, Y = a["A"], a["B"], a["C"], a["Y"]
    m = a["m_rows"]
    lo = np.zeros(m, bool); up = np.zeros(m, bool)
    lo[:len(active_lower)] = np.asarray(active_lower).astype(bool)[:m]; up[:len(active_upper)] = np.asarray(active_upper).astype(bool)[:m]
    A = S.working_set(a, lo | up)
    p = BR.cotangent(a, seed_cmd, seed_input)
    q = Y[:nz, :nz] @ p
    out = dict(n=len(A), dependent=False)
    shapes = dict(OW=(ny, ph), UW=(nu, ph), DUW=(nu, ph), lower=(m,), upper=(m,), A=(nx, nx), B=(nx, nu), C=(ny, nx), Bd=(nx, ndu), Dd=(ny, ndu))
    mu = np.zeros(0)
    Sm = None
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
    if out["dependent"]:
        out.update({k: np.full(shp, np.nan) for k, shp in shapes.items()})
        return out
    # the roll-out of the direction through the controller's own model: what Cq q and Xq q are for one controller
    dv = np.vstack([np.zeros(nu)] + [q[blk[i] * nu:(blk[i] + 1) * nu] for i in range(1, ph + 1)])       # row i: v_i, v_0 = lastU is data
    dX = np.zeros((ph + 1, nx))
    for i in range(1, ph + 1):
        dX[i] = Am @ dX[i - 1] + Bm @ dv[i]
    dy = dX @ Cm.T
    # ---- weights and bounds (4.9)
    X, Yo = np.asarray(seq_state, float), np.asarray(seq_output, float)
    v = np.vstack([np.asarray(u0, float)] + [seq_input[i - 1] for i in range(1, ph + 1)])
    gl = np.zeros(m); gu = np.zeros(m)
    for k, e in enumerate(A):
        if e < nz:
            r = min(r for r in a["boxrow_ref"][a["boxrow_ptr"][e]:a["boxrow_ptr"][e + 1]] if 0 <= r < m and (lo[r] or up[r]))
        else:
            r = a["g_refrow"][e - ldz]
        (gu if up[r] else gl)[r] = mu[k]
    out["OW"] = np.stack([-dy[i + 1] * (Yo[i + 1] - yref[:, i]) for i in range(ph)], axis=1)
    out["UW"] = np.stack([-dv[i + 1] * (v[i + 1] - uref[:, i]) for i in range(ph)], axis=1)
    out["DUW"] = np.stack([-(dv[i + 1] - dv[i]) * (v[i + 1] - v[i] - duref[:, max(i - 1, 0)]) for i in range(ph)], axis=1)
    out.update(lower=gl, upper=gu)
    if not want_model:
        return out
    # ---- the model (4.10): the cost's stage gradients and its condensed gradient at the optimum, one backward pass
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
        grad[blk[i] * nu:(blk[i] + 1) * nu] += Bm.T @ c + a["Wu"][:, i] * (v[i] - uref[:, i - 1]) + r[i - 1] - (r[i] if i < ph else 0.0)
    lam = np.zeros(0)
    if len(A):
        # the optimum's multipliers: stationarity on the hard rows, a soft row's own relation (its 1 / weight is on S's diagonal)
        rhs = -(Y[A][:, :nz] @ grad)
        for k, eidx in enumerate(A):
            if eidx >= ldz and a["g_soft"][eidx - ldz] > 0.0:
                rr = eidx - ldz
                rhs[k] += Mo.row_value(a, rr, X, Yo, v) - (a["ug0"][rr] if up[a["g_refrow"][rr]] else a["lg0"][rr])
        lam = np.linalg.solve(Sm, rhs)
    o = e.copy()
    do = a["Wy"].T * dy
    do[0] = 0.0
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
    return out


def restatement(R, ctl, b, **kw):
    """rollout_gradients of instance b of a reference on the host-only handles `ctl` of its controllers"""
    k = R["model"][b]
    sp = R["specs"][k]
    ph = sp["dims"][4]
    uref, duref, dmeas = own_references(sp)
    return rollout_gradients(arrays(ctl[k]), R["active_lower"][b], R["active_upper"][b], R["u0"][b], R["seq_state"][b], R["seq_output"][b],
                             R["input"][b], np.tile(R["yref"][b][:, None], (1, ph)), uref, duref, dmeas, R["seed_cmd"][b], R["seed_input"][b], **kw)


def compare(a, t, g, blocked=False, model=True, param=True):
    """(parameters, model): worst |g - truth| / max(1, max|truth|) of the five outputs of each part, by param_sens_ref.compare (which also asserts
    that the bound rows the condensed problem has no bound for are zero) and model_sens_ref.compare"""
    ep = P.compare(a, t, g, blocked) if param else 0.0
    em = Mo.compare({k: t[k] for k in MODEL if k in t}, g) if model else 0.0
    return ep, em


def group_sums(rows, flags, order, offsets):
    """[K x ..]: the rows of every controller's instances whose flag is 0 added in the order of `order`, and how many those were"""
    K = len(offsets) - 1
    out = np.zeros((K,) + rows.shape[1:]); used = np.zeros(K, int)
    for k in range(K):
        for b in order[offsets[k]:offsets[k + 1]]:
            if flags[b] == 0:
                out[k] += rows[b]; used[k] += 1
    return out, used
