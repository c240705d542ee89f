"""Reference for the backward pass of the closed loop, numpy only: the loop and its adjoint in float64, no product code.

forward: tick by tick, the certified optimum of the reference QP (qp_truth.certified_optimum on sens_ref.builder(sp)) and the plant step
x <- A_p x + B_p cmd + Bd_p d_k + w_k in numpy.  backward: the adjoint recursion
    c_k = seed_u[k] + B_p' lam_{k+1} + mu_{k+1},  (gx, gu, gy) = J_k' c_k,  lam_k = seed_x[k] + A_p' lam_{k+1} + gx,  mu_k = gu
with J_k = sens_ref.kkt_jacobian on the truth's active sets, the weights and the model from the KKT truths of param_sens_ref and model_sens_ref
seeded with c_k, d_noise[k] = lam_{k+1}, d_plant += lam_{k+1} [x_k; cmd_k; d_k]'.

restate: the same chain over sens_ref.condensed_jacobian, param_sens_ref.condensed_gradients and model_sens_ref.condensed_gradients on the arrays of
a host-only handle -- the kernels' formulas.  RESTATEMENT_WORST is the worst disagreement of the two relative to max(1, max|.|) per output over
CASES, measured on the CPU by tests/test_lmpc_loop_grad.py; the GPU tests hold the kernels to KERNEL_TOL = max(8 x that, 1e-12) and to nothing
else (the convention of qp_truth).

A case is a family of the sensitivity tests (or one of the two new ones) with a loop around it: n distinct instances, `ticks`, a plant (the
controller's own, one other for the batch, one per instance), an output reference per instance or as a preview array, process noise or none.  The
GPU tests run batches of B >= n instances by repeating the n cyclically: the truth is computed once per distinct instance.  An instance is usable
when no tick is degenerate by the truth alone (margin >= qp_truth.MARGIN_MIN, independent tight rows) and every KKT system is well posed."""
import functools

import numpy as np

import model_sens_ref as Mo
import param_sens_ref as P
import qp_truth as QT
import rate_ref as RR
import sens_ref as S

RESTATEMENT_WORST = 1.4e-12           # soft, d_A (measured 1.35e-12); the others are at 1.5e-13 and below
KERNEL_TOL = max(8.0 * RESTATEMENT_WORST, 1e-12)
SKIP_CAP = S.SKIP_CAP

PER_INSTANCE = ("d_x0", "d_u0", "d_yref", "d_noise")
PLANT = ("d_plant_A", "d_plant_B", "d_plant_Bd")
WEIGHTS = ("d_oweight", "d_uweight", "d_duweight")
MODEL = ("d_A", "d_B", "d_C", "d_Bd", "d_Dd")
SUMMED = PLANT + WEIGHTS + MODEL

# name -> (family, n, ticks, plant, yref, noise, theta): plant in own | other | batch; yref in instance | preview; theta: weights and model too
# (left out where the model has a thousand entries: those families are there for the adjoint kernel's lane maps, the launches behind the weights and
# the model are the same everywhere)
CASES = {
    "smallest": ("smallest", 16, 5, "own", "instance", True, True),
    "full": ("full", 8, 5, "own", "instance", True, True),
    "full_t1": ("full", 4, 1, "own", "instance", True, True),
    "full_t2": ("full", 7, 2, "own", "instance", True, True),
    "full_other": ("full", 4, 2, "other", "instance", True, True),
    "full_batch": ("full", 7, 2, "batch", "instance", True, True),
    "full_preview": ("full", 4, 2, "own", "preview", True, True),
    "full_quiet": ("full", 4, 2, "own", "instance", False, True),
    "blocked": ("blocked", 6, 2, "own", "instance", True, True),
    "soft": ("soft", 6, 2, "own", "instance", True, True),
    "refs": ("refs", 6, 2, "own", "instance", True, True),
    "ndu2": ("ndu2", 4, 2, "batch", "instance", True, True),
    "nx33": ("nx33", 3, 2, "batch", "instance", True, False),
    "nx32": ("nx32", 3, 2, "batch", "instance", True, False),
    "nu_gt_nx": ("nu_gt_nx", 6, 2, "batch", "instance", True, True),
}
# where a case's instances start in its family's batch, and the factor on the family's x0 and yref: chosen so that the truth alone leaves out at most
# SKIP_CAP of a case (tests/test_lmpc_loop_grad.py checks it), every case but `smallest` has a tick with a non-empty active set and `full` an
# instance whose active set changes between ticks
START = {"ndu2": 5}
SCALE = {}
# the GPU batches of a case: B instances, the n distinct ones repeated cyclically
BATCHES = {"full_t2": (1, 63, 64, 65), "full_batch": (65,), "nx33": (65,), "nx32": (65,), "nu_gt_nx": (65,), "smallest": (16,)}


def family(name):
    if name == "nx32":                           # ipw = 2, no idle lane
        sp = RR.rate_spec(232, 32, 1, 0, 1, 2, 2, rate=0.3, box=0.6)
        return S._batch(sp, 16, 35, 1.0, 0.5)
    if name == "nu_gt_nx":                       # the rows of c (nu = 3) outnumber an instance's lanes (nx = 2)
        sp = RR.rate_spec(243, 2, 3, 0, 3, 4, 4, rate=0.3, box=0.6)
        return S._batch(sp, 16, 36, 1.0, 0.5)
    return Mo.family(name)


def inputs(name):
    """what a case's loop is given: dict(sp, n, ticks, x0, u0, yref ([n, ny], or [n, ticks + ph, ny] with preview), preview, plant (kind, A_p,
    B_p, Bd_p: [nx, .] or [n, nx, .]), noise ([ticks, n, nx] or None), seed_x, seed_u, theta)"""
    fam, n, ticks, plant, ymode, noisy, theta = CASES[name]
    sp, x0, u0, yref = family(fam)
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    first, scale = START.get(name, 0), SCALE.get(name, 1.0)
    x0, u0, yref = scale * x0[first:first + n], u0[first:first + n].copy(), scale * yref[first:first + n]
    rg = np.random.default_rng(1000 + sorted(CASES).index(name))
    preview = ymode == "preview"
    if preview:
        yref = yref[:, None, :] + 0.3 * rg.normal(size=(n, ticks + ph, ny))
    Bd = sp.get("Bd", np.zeros((nx, ndu)))
    lead = {"own": None, "other": (), "batch": (n,)}[plant]
    if lead is None:
        Ap, Bp, Bdp = sp["A"], sp["B"], Bd
    else:
        Ap = sp["A"] + 0.05 * rg.normal(size=lead + (nx, nx)); Bp = sp["B"] + 0.05 * rg.normal(size=lead + (nx, nu))
        Bdp = Bd + 0.05 * rg.normal(size=lead + (nx, ndu))
    noise = 0.02 * rg.normal(size=(ticks, n, nx)) if noisy else None
    return dict(name=name, sp=sp, n=n, ticks=ticks, x0=x0, u0=u0, yref=yref, preview=preview, plant=(plant, Ap, Bp, Bdp), noise=noise,
                seed_x=rg.normal(size=(ticks + 1, n, nx)), seed_u=rg.normal(size=(ticks, n, nu)), theta=theta)


def plant_of(I, b):
    kind, Ap, Bp, Bdp = I["plant"]
    return (Ap[b], Bp[b], Bdp[b]) if kind == "batch" else (Ap, Bp, Bdp)


def tick_refs(I, b, k):
    """yref [ny x ph] and dmeas [ndu x ph] the solve of tick k of instance b sees"""
    nx, nu, ndu, ny, ph, ch = I["sp"]["dims"]
    yR = I["yref"][b, k:k + ph].T if I["preview"] else np.tile(I["yref"][b][:, None], (1, ph))
    return yR, I["sp"].get("dmeas", np.zeros((ndu, ph)))


def forward_one(I, pb, b, x0=None, u0=None, yshift=None, noise=None, plant=None):
    """the closed loop of instance b, any input replaced where given: dict(x [ticks + 1, nx], u [ticks, nu], lower, upper [ticks, ncon],
    act [ticks, ncon - neq] (the truth's own active rows), seq (state, output, input per tick), degenerate)"""
    from oracle import lmpc_numpy as LN
    sp = I["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    Ap, Bp, Bdp = plant_of(I, b) if plant is None else plant
    x = np.array(I["x0"][b] if x0 is None else x0, float); u = np.array(I["u0"][b] if u0 is None else u0, float)
    w = I["noise"][:, b] if (noise is None and I["noise"] is not None) else noise
    X, U, lo, up, seq, act = [x.copy()], [], [], [], [], []
    degenerate, prev = False, (None, None)
    comp = QT.compared_rows(sp)
    for k in range(I["ticks"]):
        yR, dM = tick_refs(I, b, k)
        if yshift is not None:
            yR = yR + np.asarray(yshift)[:, None]
        q, l, ub = S._qlu(pb, sp, x, u, yR, dM)
        t = QT.certified_optimum(pb, q, l, ub, prev[0], prev[1], compared=comp)
        prev = (t["active_lower"], t["active_upper"])
        assert t is not None, (I["name"], b, k)
        state, out, inp = LN.unpack_solution(pb.d, t["z"], pb.ssC[:ny, :nx], pb.ssDv[:ny, :], dM)
        degenerate = degenerate or t["degenerate"]
        u = inp[0].copy()
        x = Ap @ x + Bp @ u + (Bdp @ dM[:, 0] if ndu else 0.0) + (w[k] if w is not None else 0.0)
        # rows the reference QP writes with equal bounds (the moves past the control horizon, fixed at zero) are equalities to the truth and carry no
        # active bit there; the KKT systems of the backward pass need them in their working set
        fixed = (l == ub) & np.isfinite(l)
        fixed[:pb.d.neq] = False
        X.append(x.copy()); U.append(u); lo.append(t["active_lower"] | fixed); up.append(t["active_upper"]); seq.append((state, out, inp))
        act.append((t["active_lower"] | t["active_upper"]).astype(bool)[pb.d.neq:])
    return dict(x=np.array(X), u=np.array(U), lower=np.array(lo), upper=np.array(up), act=np.array(act), seq=seq, degenerate=bool(degenerate))


def loss_of(I, b, f):
    return float((I["seed_x"][:, b] * f["x"]).sum() + (I["seed_u"][:, b] * f["u"]).sum())


def _empty(I):
    nx, nu, ndu, ny, ph, ch = I["sp"]["dims"]
    g = dict(d_x0=np.zeros(nx), d_u0=np.zeros(nu), d_yref=np.zeros(ny), d_noise=np.zeros((I["ticks"], nx)), d_plant_A=np.zeros((nx, nx)),
             d_plant_B=np.zeros((nx, nu)), d_plant_Bd=np.zeros((nx, ndu)))
    if I["theta"]:
        g.update(d_oweight=np.zeros((ny, ph)), d_uweight=np.zeros((nu, ph)), d_duweight=np.zeros((nu, ph)), d_A=np.zeros((nx, nx)),
                 d_B=np.zeros((nx, nu)), d_C=np.zeros((ny, nx)), d_Bd=np.zeros((nx, ndu)), d_Dd=np.zeros((ny, ndu)))
    return g


def _recursion(I, b, f, vjp, record=None):
    """the adjoint recursion of instance b over the logged run f; vjp(k, x_k, u_{k-1}, c_k) -> (gx, gu, gy, dict of weight and model gradients);
    record: a dict that is given tick k's (c_k, gx, gu, gy)"""
    sp = I["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    Ap, Bp, Bdp = plant_of(I, b)
    g = _empty(I)
    lam = I["seed_x"][I["ticks"], b].copy(); mu = np.zeros(nu)
    for k in range(I["ticks"] - 1, -1, -1):
        c = I["seed_u"][k, b] + Bp.T @ lam + mu
        xk, uprev = f["x"][k], (f["u"][k - 1] if k > 0 else I["u0"][b])
        gx, gu, gy, theta = vjp(k, xk, uprev, c)
        if record is not None:
            record[k] = (c, gx, gu, gy)
        g["d_noise"][k] = lam
        g["d_plant_A"] += np.outer(lam, xk); g["d_plant_B"] += np.outer(lam, f["u"][k])
        if ndu:
            g["d_plant_Bd"] += np.outer(lam, tick_refs(I, b, k)[1][:, 0])
        lam = I["seed_x"][k, b] + Ap.T @ lam + gx
        mu = gu
        g["d_yref"] += gy
        for n, v in theta.items():
            g[n] += v
    g["d_x0"], g["d_u0"] = lam, mu
    return g


_THETA_P = dict(d_oweight="OW", d_uweight="UW", d_duweight="DUW")
_THETA_M = dict(d_A="A", d_B="B", d_C="C", d_Bd="Bd", d_Dd="Dd")


def backward_one(I, pb, truths, b, f):
    """the truth's adjoint of instance b, or None where a tick's KKT system is not well posed"""
    sp = I["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    bad = []

    def vjp(k, xk, uprev, c):
        yR, dM = tick_refs(I, b, k)
        J = S.kkt_jacobian(pb, sp, xk, uprev, yR, f["lower"][k], f["upper"][k], dmeas=dM)
        if not S.good(J):
            bad.append(k)
        gx, gu, gy = S.split(J["cmd"].T @ c, nx, nu)
        theta = {}
        if I["theta"]:
            tp = truths[0].gradients(xk, uprev, yR, f["lower"][k], f["upper"][k], seed_cmd=c)
            tm = truths[1].gradients(xk, uprev, yR, f["lower"][k], f["upper"][k], seed_cmd=c)
            if not (S.good(tp) and S.good(tm)):
                bad.append(k)
            theta = {n: tp[w] for n, w in _THETA_P.items()}
            theta.update({n: tm[w] for n, w in _THETA_M.items() if w in tm})
        return gx, gu, gy, theta
    g = _recursion(I, b, f, vjp, f.setdefault("vjp", {}))
    return None if bad else g


def restate_one(I, a, b, f):
    """the same chain over the kernels' formulas on the arrays `a` of a host-only handle (model_sens_ref.arrays with param_sens_ref's Cq)"""
    sp = I["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]

    def vjp(k, xk, uprev, c):
        yR, dM = tick_refs(I, b, k)
        lo, up = f["lower"][k], f["upper"][k]
        J = S.condensed_jacobian(a, lo, up)
        gx, gu, gy = S.split(J["cmd"].T @ c, nx, nu)
        theta = {}
        if I["theta"]:
            state, out, inp = f["seq"][k]
            tp = P.condensed_gradients(a, lo, up, uprev, out, inp, yR, sp["uref"], sp["duref"], seed_cmd=c)
            tm = Mo.condensed_gradients(a, lo, up, uprev, state, out, inp, yR, sp["uref"], sp["duref"], dM, seed_cmd=c)
            theta = {n: tp[w] for n, w in _THETA_P.items()}
            theta.update({n: tm[w] for n, w in _THETA_M.items()})
        return gx, gu, gy, theta
    return _recursion(I, b, f, vjp)


def compare(t, g):
    """worst |g - truth| / max(1, max|truth|) per output, over the outputs the truth has"""
    worst = 0.0
    for n, v in t.items():
        if v.size:
            worst = max(worst, float(np.abs(np.asarray(g[n]) - v).max() / max(1.0, np.abs(v).max())))
    return worst


@functools.lru_cache(maxsize=None)
def reference(name):
    """inputs(name) and, per distinct instance, the forward run `fwd`, the adjoint `grad` (None: not usable), `usable` [n], and what the GPU tests need
    of the seeds: nonempty (a tick with a non-empty active set exists), changes (an instance whose active set differs between two ticks)"""
    I = inputs(name)
    sp = I["sp"]
    pb = S.builder(sp)
    truths = (P.Truth(sp), Mo.Truth(sp)) if I["theta"] else None
    fwd = [forward_one(I, pb, b) for b in range(I["n"])]
    grad = [None if f["degenerate"] else backward_one(I, pb, truths, b, f) for b, f in enumerate(fwd)]
    act = [f["act"] for f in fwd]
    I.update(pb=pb, fwd=fwd, grad=grad, usable=np.array([g is not None for g in grad]),
             nonempty=any(a.any() for a in act), changes=any((a[1:] != a[:-1]).any() for a in act if len(a) > 1))
    return I


def tiled(R, B):
    """the batch of B instances the GPU tests run for reference R: every per-instance input with instance b = distinct instance b mod n, and `of` [B]
    that map"""
    n = R["n"]
    of = np.arange(B) % n
    kind, Ap, Bp, Bdp = R["plant"]
    plant = (kind,) + tuple(m[of] for m in (Ap, Bp, Bdp)) if kind == "batch" else R["plant"]
    return dict(of=of, x0=R["x0"][of], u0=R["u0"][of], yref=R["yref"][of], plant=plant, noise=None if R["noise"] is None else R["noise"][:, of],
                seed_x=R["seed_x"][:, of], seed_u=R["seed_u"][:, of])


def stacked(R, of, names):
    """the truth of the usable ones among the instances `of`, stacked per output: (dict name -> [len(use), ..], use = their positions)"""
    use = [i for i, b in enumerate(of) if R["usable"][b]]
    out = {}
    for n in names:
        if n in R["grad"][of[use[0]]] and R["grad"][of[use[0]]][n].size:
            v = np.stack([R["grad"][of[i]][n] for i in use])
            out[n] = np.moveaxis(v, 0, 1) if n == "d_noise" else v
    return out, use
