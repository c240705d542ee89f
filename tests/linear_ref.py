"""Reference for the linear rows: the reference QP of rate_ref.builder with (ph + 1) nc rows appended to A, lineq, uineq,

    lo[c, i] <= [Fx | Fu][c, :] xi_i <= hi[c, i],      xi_i = [x_i; x_u(i)] the reference's stacked state of step i,

row i nc + c behind the reference's own (its row number is ncon(reference) + i nc + c), solved by the numpy restatement of OSQP exactly as
rate_ref.solve_one does it (a "polished" point with a wrong-signed multiplier does not count as polished).  A soft linear row gets a slack
column as the soft rows of tests/soft_ref.py do.  Also: an independent numpy condensing of the linear rows for the host tests.

A controller is a rate_ref spec (optionally with soft_ref's sp["soft"]) with sp["lin"] = dict(Fx [nc, nx], Fu [nc, nu], lo, hi [nc, ph + 1],
w [nc] | None): column i of the bounds is step i, w the soft weights of the rows over steps 0 .. ph (inf entries stay hard); terminal_ref's
sp["P"], sp["xT"], sp["Tx"] add its terminal cost.  `configure` applies
it to a libmpc_amd.LMPC, `builder` to oracle.lmpc_numpy.ProblemBuilderRef."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import rate_ref as RR
import soft_ref as SR
import terminal_ref as TR
from oracle import lmpc_numpy as LN

INF = float("inf")


def with_linear(sp, Fx, Fu, lo, hi, w=None, steps=None):
    """sp with linear rows; lo, hi [nc] (every step of `steps`, default 0 .. ph; the others unbounded) or [nc, ph + 1]"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    Fx = np.atleast_2d(np.asarray(Fx, float)); Fu = np.atleast_2d(np.asarray(Fu, float))
    nc = Fx.shape[0]
    assert Fx.shape == (nc, nx) and Fu.shape == (nc, nu)

    def full(v, fill):
        v = np.asarray(v, float)
        if v.ndim == 2:
            return v.copy()
        out = np.full((nc, ph + 1), fill)
        for i in (range(ph + 1) if steps is None else steps):
            out[:, i] = v
        return out
    out = dict(sp)
    out["lin"] = dict(Fx=Fx, Fu=Fu, lo=full(lo, -INF), hi=full(hi, INF), w=None if w is None else np.broadcast_to(np.asarray(w, float), (nc,)).copy())
    return out


def without_linear(sp):
    return {k: v for k, v in sp.items() if k != "lin"}


def configure(c, sp, maximum_iteration=RR.MAXIT, linear=True, **kw):
    """soft_ref.configure (rate_ref.configure and the soft weights), then the linear rows and their weights"""
    SR.configure(c, sp, maximum_iteration, **kw)
    if linear and "lin" in sp:
        L = sp["lin"]
        assert c.setLinearConstraints(L["Fx"], L["Fu"], L["lo"], L["hi"])
        if L.get("w") is not None:
            assert c.setLinearConstraintWeights(L["w"])
    if "P" in sp:                                        # terminal_ref's terminal cost
        assert c.setTerminalCost(sp["P"], sp.get("xT"), sp.get("Tx"))
    return c


class LinearBuilder:
    """rate_ref.builder(sp) (soft_ref.SoftBuilder with sp["soft"]) with the linear rows appended and a slack column per soft linear row: what
    rate_ref.solve_one reads of a builder (d, P, A, get, ssC, ssDv).  d is the reference's LmpcDims with ncon grown by the new rows; ncon_ref
    keeps the reference's count, row0 = ncon_ref is the first new row"""

    def __init__(self, sp):
        base = SR.SoftBuilder(sp) if "soft" in sp else RR.builder(sp)
        self.base = base
        d0 = base.d
        nx, nu, ndu, ny, ph, ch = sp["dims"]
        L = sp.get("lin")
        nc = 0 if L is None else L["Fx"].shape[0]
        self.nc, self.ncon_ref, self.row0 = nc, d0.ncon, d0.ncon
        nrow = (ph + 1) * nc
        n0 = base.P.shape[0]
        w = None if L is None else L.get("w")
        self.soft = []                                   # (new row index, rho)
        for i in range(ph + 1):
            for c in range(nc):
                if w is not None and np.isfinite(w[c]) and (np.isfinite(L["lo"][c, i]) or np.isfinite(L["hi"][c, i])):
                    self.soft.append((i * nc + c, float(w[c])))
        k = len(self.soft)
        self.P = np.zeros((n0 + k, n0 + k)); self.P[:n0, :n0] = base.P
        self.A = np.zeros((d0.ncon + nrow, n0 + k)); self.A[:d0.ncon, :n0] = base.A
        self.lo = np.zeros(nrow); self.hi = np.zeros(nrow)
        for i in range(ph + 1):
            for c in range(nc):
                r = d0.ncon + i * nc + c
                self.A[r, i * d0.na:i * d0.na + nx] = L["Fx"][c]
                self.A[r, i * d0.na + nx:(i + 1) * d0.na] = L["Fu"][c]
                self.lo[i * nc + c] = L["lo"][c, i]; self.hi[i * nc + c] = L["hi"][c, i]
        for s, (r, rho) in enumerate(self.soft):
            self.P[n0 + s, n0 + s] = rho
            self.A[d0.ncon + r, n0 + s] = -1.0
        if "P" in sp:                                    # terminal_ref.builder's term: P on the x-block of xi_ph (its solve_one adds -P x_T to q)
            o = ph * d0.na
            self.P[o:o + nx, o:o + nx] += 0.5 * (sp["P"] + sp["P"].T)
        self.d = LN.LmpcDims(nx, nu, ndu, ny, ph, ch)
        self.d.ncon = d0.ncon + nrow
        self.ssC, self.ssDv = base.ssC, base.ssDv

    def get(self, *a):
        q, l, u = self.base.get(*a)
        return np.concatenate([q, np.zeros(len(self.soft))]), np.concatenate([l, self.lo]), np.concatenate([u, self.hi])


def solve_batch(sp, x0, u0, yref=None, dmeas=None, maximum_iteration=RR.MAXIT, workers=None):
    """rate_ref.solve_batch on the QP with the linear rows (and slacks): the dict helpers.assert_matches_oracle takes, plus 'neq', 'ncon' (with
    the new rows), 'ncon_ref', 'nc', 'is_feasible', 'input', 'state', 'n_active', 'n_linear_active', 'y'"""
    pb = LinearBuilder(sp)
    d = pb.d
    B = len(x0)
    workers = workers or max(1, min(4, os.cpu_count() or 1))

    one = TR.solve_one if "P" in sp else RR.solve_one

    def job(b):
        return one(pb, sp, x0[b], u0[b], None if yref is None else yref[b], None if dmeas is None else dmeas[b], maximum_iteration)
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(job, range(B)))
    res = {"neq": d.neq, "ncon": d.ncon, "ncon_ref": pb.ncon_ref, "nc": pb.nc}
    res["cmd"] = np.stack([p["cmd"] for p in parts]); res["cost"] = np.array([p["cost"] for p in parts])
    res["input"] = np.stack([p["input"] for p in parts]); res["state"] = np.stack([p["state"] for p in parts])
    for k in ("status", "solver_status", "iters", "polished", "polished_raw", "is_feasible"):
        res[k] = np.array([int(p[k]) for p in parts], dtype=np.int32)
    soft = np.array([d.neq + r for r, _ in pb.base.rows], dtype=int) if "soft" in sp else np.zeros(0, int)
    for k in ("active_lower", "active_upper"):
        res[k] = np.stack([p[k] for p in parts])
        keep = res[k][:, soft].copy()
        res[k][:, d.neq:d.neq + d.na] = 0          # the hard box rows of step 0 bound data, not decisions
        res[k][:, soft] = keep
        # a hard linear row of step 0 bounds data too: the product reports no active bit for a feasibility row
        hard0 = [pb.row0 + c for c in range(pb.nc) if c not in {r for r, _ in pb.soft}]
        res[k][:, hard0] = 0
    act = (res["active_lower"] != 0) | (res["active_upper"] != 0)
    res["n_active"] = act[:, d.neq:].sum(axis=1)
    res["n_linear_active"] = act[:, pb.row0:].sum(axis=1)
    res["y"] = np.stack([p["y"] for p in parts])
    return res


def compared_rows(sp):
    """rate_ref.compared_rows and every linear row; with move blocking the linear rows past the control horizon are left out as the state
    and output rows there are"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    keep0 = RR.compared_rows(sp)
    nc = sp["lin"]["Fx"].shape[0] if "lin" in sp else 0
    keep = np.concatenate([keep0, np.ones((ph + 1) * nc, bool)])
    if ch < ph - 1:
        keep[len(keep0) + (ch + 1) * nc:] = False
    return keep


def row_values(sp, state, inputs, u0):
    """[B, nc, ph + 1]: Fx x_i + Fu v_i of a returned sequence (state [B, ph + 1, nx], inputs [B, ph + 1, nu] with inputs[:, i] = u_i,
    v_0 = lastU, v_i = u_{i-1})"""
    L = sp["lin"]
    v = np.concatenate([np.asarray(u0)[:, None, :], inputs[:, :-1, :]], axis=1)
    return np.einsum("cx,bix->bci", L["Fx"], state) + np.einsum("cu,biu->bci", L["Fu"], v)


def violation(sp, vals, rel=0.0):
    """largest amount by which row values [B, nc, ph + 1] leave [lo, hi] widened by rel max(1, |bound|)"""
    lo, hi = sp["lin"]["lo"][None], sp["lin"]["hi"][None]
    with np.errstate(invalid="ignore"):
        a = np.where(np.isfinite(lo), lo - rel * np.maximum(1.0, np.abs(lo)) - vals, -INF)
        b = np.where(np.isfinite(hi), vals - hi - rel * np.maximum(1.0, np.abs(hi)), -INF)
    return float(max(a.max(), b.max()))


# ---------------------------------------------------------------------------------------------
# an independent condensing of the linear rows (host tests)
# ---------------------------------------------------------------------------------------------
def condensed_linear_rows(sp):
    """numpy condensing of the linear rows, independent of the product: dict(G [m x nz], lo, hi, step, comp, refrow, g_soft, X0 [m x nx], U0 [m x nu]
    -- the coefficients of x0 and lastU in the row's offset (no disturbance) -- and `fixed`: [(step, comp, refrow, lo, hi)] of the hard rows without
    coefficients), the general rows in the product's order among themselves (by step, then row); a row exists for a finite side only"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = LN.LmpcDims(nx, nu, ndu, ny, ph, ch)
    L = sp["lin"]
    nc = L["Fx"].shape[0]
    nf = min(ph, ch + 1)
    nz = nf * nu
    blk = [0] + [min(i, nf) - 1 for i in range(1, ph + 1)]
    A, Bm = sp["A"], sp["B"]

    def E(i):
        e = np.zeros((nu, nz))
        if i > 0:
            e[:, blk[i] * nu:(blk[i] + 1) * nu] = np.eye(nu)
        return e
    Sx, Ai = [np.zeros((nx, nz))], [np.eye(nx)]
    for i in range(1, ph + 1):
        Sx.append(A @ Sx[-1] + Bm @ E(i)); Ai.append(A @ Ai[-1])
    w = L.get("w")
    keep, fixed = [], []
    for i in range(ph + 1):
        for c in range(nc):
            lo, hi = L["lo"][c, i], L["hi"][c, i]
            if not (np.isfinite(lo) or np.isfinite(hi)):
                continue
            g = L["Fx"][c] @ Sx[i] + L["Fu"][c] @ E(i)
            soft = 0.0 if w is None or not np.isfinite(w[c]) else 1.0 / w[c]
            ref = d.ncon + i * nc + c
            if np.abs(g).max(initial=0.0) < 1e-14 and soft == 0.0:
                fixed.append((i, c, ref, lo, hi))
                continue
            keep.append((g, lo, hi, i, c, ref, soft, L["Fx"][c] @ Ai[i], L["Fu"][c] if i == 0 else np.zeros(nu)))
    col = lambda k: np.array([r[k] for r in keep])
    m = len(keep)
    return dict(G=col(0).reshape(m, nz), lo=col(1), hi=col(2), step=col(3).astype(int), comp=col(4).astype(int), refrow=col(5).astype(int),
                g_soft=col(6), X0=col(7).reshape(m, nx), U0=col(8).reshape(m, nu), fixed=fixed)


# ---------------------------------------------------------------------------------------------
# the cases of the tests
# ---------------------------------------------------------------------------------------------
def smallest_spec():
    """(2, 1, 0, 1, 2, 2), nc = 2: row 0 reads only u, |v_1| <= 0.4 at step 1; row 1 reads x and u, |x_2 + 0.5 v_2| <= 0.6 at step 2 (x_2 the second
    state).  With one input a step has one row to lean on: bounded at different steps, both are active when the reference is far"""
    sp = RR.rate_spec(102, 2, 1, 0, 1, 2, 2, rate=0.1)
    sp = RR.without_rate(sp)
    Fx = np.array([[0.0, 0.0], [0.0, 1.0]]); Fu = np.array([[1.0], [0.5]])
    lo = np.array([[-INF, -0.4, -INF], [-INF, -INF, -0.6]])
    return with_linear(sp, Fx, Fu, lo, -lo)


def smallest_batch(B=65):
    sp = smallest_spec()
    r = np.random.default_rng(7)
    x0 = 0.2 * r.normal(size=(B, 2)); u0 = r.uniform(-0.3, 0.3, size=(B, 1))
    r = np.random.default_rng(8)
    yref = r.choice([-1.0, 1.0], size=(B, 1)) * r.uniform(3.0, 5.0, size=(B, 1))         # a reference far away: every instance pulls hard
    return sp, x0, u0, yref


def random_rows(sp, nc, seed, size=1.0, steps=None, w=None, onesided=True):
    """nc random rows on (x, v) with bounds +-size (every third row one-sided)"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    r = np.random.default_rng(seed)
    Fx = r.normal(size=(nc, nx)); Fu = r.normal(size=(nc, nu))
    lo = np.full(nc, -size); hi = np.full(nc, size)
    if onesided:
        lo[2::3] = -INF
    return with_linear(sp, Fx, Fu, lo, hi, w=w, steps=steps)


def case(name):
    """the GPU tests' controllers and batches: (sp, x0, u0, yref | None, dmeas | None).  The seeds were chosen on the CPU so that the yardstick alone
    polishes at least 90 % of every batch; its solves of these cases take seconds: recorded by tests/golden/make_linear_golden.py"""
    if name == "full":
        # rate_ref's full-feature controller (input box, state, output, scalar and rate rows, Bd / Dd) with two linear rows from step 1 on
        sp = random_rows(RR.full_feature_spec(), 2, 33, size=1.0, steps=range(1, 11), onesided=False)
        x0, u0, yref, dmeas = RR.full_feature_batch(24)
        return sp, x0, u0, yref, dmeas
    dims, model, seed = {"blocked": ((3, 2, 0, 2, 8, 3), 203, 44), "ch=ph": ((4, 2, 0, 2, 10, 10), 202, 41)}[name]
    base = RR.without_rate(RR.rate_spec(model, *dims, rate=0.1))
    base.update(umin=-1.0 * np.ones(2), umax=1.0 * np.ones(2))
    sp = random_rows(base, 3, seed, size=1.0, steps=range(1, dims[4] + 1))
    x0, u0, _ = RR.random_batch(sp, 24, 9)
    yref = 2.0 * np.random.default_rng(10).normal(size=(24, 2))
    return sp, 0.3 * x0, u0, yref, None


def next_tick(sp, x0, cmd, dmeas=None):
    """the state after one tick with the command `cmd`"""
    d0 = (sp["dmeas"][:, 0][None, :] if dmeas is None else dmeas[:, :, 0]) if "Bd" in sp else np.zeros((len(x0), 0))
    return x0 @ sp["A"].T + cmd @ sp["B"].T + (d0 @ sp["Bd"].T if "Bd" in sp else 0.0)


ORACLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_oracle.npz")
_oracle = {}


def recorded(name, **inputs):
    """the yardstick's recorded results of a case (solve_batch's dict, the active bits unpacked), after checking that they were computed for
    these inputs"""
    if not _oracle:
        with np.load(ORACLE) as z:
            for k in z.files:
                case_, key = k.split("/", 1)
                _oracle.setdefault(case_, {})[key] = z[k]
    g = _oracle[name]
    for k, v in inputs.items():
        assert (v is None and "in_" + k not in g) or np.array_equal(g["in_" + k], v), (name, k)
    ref = {k: (v if v.ndim else v.item()) for k, v in g.items() if not k.startswith("in_")}
    m = int(ref["ncon"])
    for k in ("active_lower", "active_upper"):
        ref[k] = np.unpackbits(g[k], axis=1, bitorder="little")[:, :m]
    return ref


LARGE_DIMS = (2, 2, 0, 1, 40, 40)       # 160 linear rows: the two-chunk kernel variant


def large_case(B=8):
    """the case whose oracle solves take a second each: its results are recorded (tests/golden/make_linear_golden.py)"""
    base = RR.without_rate(RR.rate_spec(401, *LARGE_DIMS, rate=0.1))
    sp = random_rows(base, 4, 43, size=1.5, steps=range(1, 41), onesided=False)
    r = np.random.default_rng(13)
    return sp, r.normal(size=(B, 2)), r.uniform(-0.1, 0.1, size=(B, 2)), 1.2 * r.normal(size=(B, 1))


def integrator_coupled(ph=10, c=0.25, box=1.0, w=None):
    """the double integrator of rate_ref (input box, no rate bounds) with the coupled row |x_2 + 0.5 v| <= c from step 1 on"""
    sp = RR.integrator_spec(ph=ph, rate=None, box=box)
    return with_linear(sp, [[0.0, 1.0]], [[0.5]], [-c], [c], w=w, steps=range(1, ph + 1))


def terminal_spec(ph=10):
    """the double integrator (input box +-1: the position moves by at most 0.5 in the horizon) with the terminal set x_1 >= 0.1, |x_2| <= 0.3,
    x_1 + x_2 <= 0.9 at the last step only, and a terminal cost on the distance to (1, 0): without the set the loop arrives at a velocity of 0.7"""
    sp = RR.integrator_spec(ph=ph, rate=None, box=1.0)
    Fx = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]); Fu = np.zeros((3, 1))
    sp = with_linear(sp, Fx, Fu, [0.1, -0.3, -INF], [INF, 0.3, 0.9], steps=[ph])
    return TR.with_terminal(sp, np.array([[40.0, 5.0], [5.0, 8.0]]), xT=np.array([1.0, 0.0]))


# ---------------------------------------------------------------------------------------------
# the condensing families with linear rows (tests/golden/condense_truth_linear.npz, written by tests/golden/make_linear_golden.py): what
# tests/condense_ref.py is for the other rows -- its bound, its constant and its padded layouts are imported, not restated
# ---------------------------------------------------------------------------------------------
import json                      # noqa: E402

import condense_ref as CR        # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "condense_truth_linear.npz")
# `linear`: four controllers of different structure -- nc = 1; nc = 3 with rows at the last step only; nc = 16; nc = 2 combined with state, output,
# scalar, rate and soft rows (a soft linear row among them) and a terminal cost.  `linear_bank`: three controllers of one structure (nc = 3) with
# Fx, Fu and bounds of their own: one bank
FAMILIES = {"linear": 4, "linear_bank": 3}
LINEAR_KEYS = ("Fx", "Fu", "flo", "fhi", "fw")


def layout(ctl):
    """condense_ref.layout with the linear rows of ctl (Fx [nc, nx], Fu [nc, nu], flo, fhi [nc, ph + 1], fw [nc] optional; bounds from step 1
    on): kind 4, behind the scalar row of their step and in front of its rate rows"""
    base = CR.layout({k: v for k, v in ctl.items() if k not in LINEAR_KEYS})
    nx, nu, ny, ph, ch = (int(v) for v in ctl["dims"])
    nc = ctl["Fx"].shape[0]
    assert not np.isfinite(ctl["flo"][:, 0]).any() and not np.isfinite(ctl["fhi"][:, 0]).any(), "a step-0 row has no coefficients: not among these families"
    rows = list(zip(base["kind"], base["step"], base["comp"], base["lo"], base["hi"], base["soft"]))
    out = []
    for i in range(1, ph + 1):
        mine = [r for r in rows if r[1] == i]
        out += [r for r in mine if r[0] != 3]
        for c in range(nc):
            lo, hi = ctl["flo"][c, i], ctl["fhi"][c, i]
            if np.isfinite(lo) or np.isfinite(hi):
                w = ctl["fw"][c] if "fw" in ctl else INF
                out.append((4, i, c, lo, hi, 1.0 / w if np.isfinite(w) else 0.0))
        out += [r for r in mine if r[0] == 3]
    col = lambda k, t: np.array([r[k] for r in out], dtype=t)
    return dict(base, kind=col(0, int), step=col(1, int), comp=col(2, int), lo=col(3, float), hi=col(4, float), soft=col(5, float))


_records = {}


def family(name):
    """[(ctl, layout, truth)] of a family, as condense_ref.family gives them"""
    if not _records:
        with np.load(GOLDEN) as z:
            data, at = z["data"], 0
            for k, shape in json.loads(z["index"].tobytes().decode()):
                rec, key = k.rsplit(".", 1)
                n = int(np.prod(shape))
                _records.setdefault(rec, {})[key] = data[at:at + n].reshape(shape).copy()
                at += n
    out = []
    for k in range(FAMILIES[name]):
        raw = _records["%s.%d" % (name, k)]
        ctl = {key: v for key, v in raw.items() if not key.startswith("t_")}
        ctl["dims"] = tuple(int(v) for v in ctl["dims"])
        for key in ("first", "smin", "smax", "sw"):
            if key in ctl:
                ctl[key] = int(ctl[key]) if key == "first" else float(ctl[key])
        lay = layout(ctl)
        nz, mg = lay["nz"], len(lay["kind"])
        tr = {key[2:]: CR._unpack(key[2:], v, mg if key == "t_GHG" else nz) for key, v in raw.items() if key.startswith("t_")}
        tr["reg"] = bool(tr["reg"])
        out.append((ctl, lay, tr))
    return out


def restate(ctl, lay):
    """condense_ref.restate for a controller with linear rows: the kernel's algorithm in float64 numpy.  The linear rows of G are written here as
    the kernel writes them (Fx(c, :) S_i accumulated over the states in its order, then Fu(c, :) added at the step's block); the rest is
    condense_ref.restate's arithmetic"""
    nx, nu, ny, ph, ch = ctl["dims"]
    nz = lay["nz"]
    blk = lay["blk"]
    plain = {k: v for k, v in ctl.items() if k not in LINEAR_KEYS}
    S = np.zeros((nx, nz)); G4 = {}
    for i in range(1, ph + 1):
        Sn = ctl["A"] @ S
        Sn[:, blk[i] * nu:(blk[i] + 1) * nu] += ctl["B"]
        S = Sn
        for r in np.nonzero((lay["step"] == i) & (lay["kind"] == 4))[0]:
            g = np.zeros(nz)
            for c in range(nx):
                g = g + ctl["Fx"][lay["comp"][r], c] * S[c]
            g[blk[i] * nu:(blk[i] + 1) * nu] += ctl["Fu"][lay["comp"][r]]
            G4[int(r)] = g
    return _restate_with_rows(plain, lay, G4)


def _restate_with_rows(ctl, lay, G4):
    """condense_ref.restate's arithmetic with the rows G4 {row: coefficients} in place of what its ladder would write for them"""
    nx, nu, ny, ph, ch = ctl["dims"]
    nz, mg, ldz, ldg, ldy = CR.pad_dims(lay)
    blk = lay["blk"]
    A, B, Cm = ctl["A"], ctl["B"], ctl["C"]
    S = np.zeros((nx, nz)); H = np.zeros((nz, nz)); G = np.zeros((mg, nz))
    for i in range(1, ph + 1):
        Sn = A @ S
        Sn[:, blk[i] * nu:(blk[i] + 1) * nu] += B
        S = Sn
        CS = Cm @ S
        for r in np.nonzero(lay["step"] == i)[0]:
            kind, cp = lay["kind"][r], lay["comp"][r]
            if kind == 0:
                G[r] = S[cp]
            elif kind == 1:
                G[r] = CS[cp]
            elif kind == 2:
                G[r] = ctl["sX"] @ S
                G[r, blk[i] * nu:(blk[i] + 1) * nu] += ctl["sU"]
            elif kind == 4:
                G[r] = G4[int(r)]
            else:
                G[r, blk[i] * nu + cp] = 1.0
                if i > 1:
                    G[r, blk[i - 1] * nu + cp] = -1.0
        H += (CS * ctl["OW"][:, i - 1][:, None]).T @ CS
        if "P" in ctl and i == ph:
            H += S.T @ (0.5 * (ctl["P"] + ctl["P"].T) @ S)
    H = np.triu(H) + np.triu(H, 1).T
    for i in range(1, ph + 1):
        for j in range(nu):
            H[blk[i] * nu + j, blk[i] * nu + j] += ctl["UW"][j, i - 1]
    for i in range(ph):
        bn = blk[i + 1]
        for j in range(nu):
            w = ctl["DUW"][j, i]
            if i == 0:
                H[bn * nu + j, bn * nu + j] += w
                continue
            bp = blk[i]
            if bp == bn:
                continue
            H[bn * nu + j, bn * nu + j] += w; H[bp * nu + j, bp * nu + j] += w
            H[bp * nu + j, bn * nu + j] -= w; H[bn * nu + j, bp * nu + j] -= w
    maxd = np.abs(np.diag(H)).max()
    L = CR._chol(H, 1e-13 * max(1.0, maxd))
    assert L is not None
    Q = CR._tri_inverse(L)
    Hinv = Q.T @ Q
    cost_direct = int(np.abs(H @ Hinv - np.eye(nz)).max() > 1e-9)
    GH = G @ Hinv
    GHG = GH @ G.T + np.diag(lay["soft"])
    bounded = np.isfinite(lay["lw"]) | np.isfinite(lay["uw"])
    rb = np.where(bounded, np.clip(CR.KAPPA / np.maximum(np.diag(Hinv), 1e-300) * np.where(lay["lw"] == lay["uw"], CR.EQ_SCALE, 1.0), CR.RHO_MIN, CR.RHO_MAX), 0.0)
    rg = np.clip(CR.KAPPA / np.maximum(np.diag(GHG), 1e-300) * np.where(lay["lo"] == lay["hi"], CR.EQ_SCALE, 1.0), CR.RHO_MIN, CR.RHO_MAX)
    Km = (G.T * rg) @ G + H + np.diag(CR.SIGMA + rb)
    Qk = CR._tri_inverse(CR._chol(Km, 0.0))
    Kinv = Qk.T @ Qk

    def sq(a, ld):
        p = np.zeros((ld, ld)); p[:a.shape[0], :a.shape[1]] = a
        return p
    Gr = np.zeros((ldg, ldz)); Gr[:mg, :nz] = G
    Y = np.zeros((ldy, ldy))
    Y[:nz, :nz] = Hinv; Y[ldz:ldz + mg, :nz] = GH; Y[:nz, ldz:ldz + mg] = GH.T; Y[ldz:ldz + mg, ldz:ldz + mg] = GHG
    rbp = np.zeros(ldz); rbp[:nz] = rb
    rgp = np.ones(ldg); rgp[:mg] = rg
    return dict(H=sq(H, ldz).ravel(), Kinv=sq(Kinv, ldz).ravel(), Gr=Gr.ravel(), Gc=Gr.T.copy().ravel(), Y=Y.ravel(), rho_b=rbp, rho_g=rgp,
                cost_direct=cost_direct, regularised=False)


def check_family(name, gots, where="", c=None):
    """condense_ref.check_family for a family of this module: gots[k] the arrays of controller k; the bound and C_BOUND are condense_ref's"""
    c = CR.C_BOUND if c is None else c
    fam = family(name)
    assert len(gots) == len(fam)
    worst = {}
    for (ctl, lay, tr), got in zip(fam, gots):
        for k, v in CR.ratios(lay, tr, got).items():
            worst[k] = max(worst.get(k, 0.0), v / c)
    print("condense %s%s: worst error / bound: %s" % (name, where, "  ".join("%s %.4f" % (k, worst[k]) for k in CR.ARRAYS)))
    assert all(v <= 1.0 for v in worst.values()), (name, where, worst)
    return worst


def configure_family(c, ctl, seed=0):
    """condense_ref.configure, then the linear rows of ctl"""
    CR.configure(c, {k: v for k, v in ctl.items() if k not in LINEAR_KEYS}, seed=seed)
    assert c.setLinearConstraints(ctl["Fx"], ctl["Fu"], ctl["flo"], ctl["fhi"])
    if "fw" in ctl:
        assert c.setLinearConstraintWeights(ctl["fw"])
    return c


def host_controllers(name):
    """the host-only controllers of a family, their layout held to `layout` entry by entry"""
    from libmpc_amd import LMPC
    out = []
    for k, (ctl, lay, tr) in enumerate(family(name)):
        nx, nu, ny, ph, ch = ctl["dims"]
        c = configure_family(LMPC(nx, nu, 0, ny, ph, ch, device=-1), ctl, seed=k)
        nz, mg, ldz, ldg, ldy = CR.pad_dims(lay)
        assert [int(v) for v in c.debug_get("dims")[:5]] == [nz, mg, ldz, ldg, ldy], (name, k, c.debug_get("dims")[:5], (nz, mg, ldz, ldg, ldy))
        for key, want in (("g_kind", lay["kind"]), ("g_step", lay["step"]), ("g_comp", lay["comp"]), ("lg0", lay["lo"]), ("ug0", lay["hi"]),
                          ("g_soft", lay["soft"])):
            assert np.array_equal(c.debug_get(key)[:mg], want), (name, k, key)
        assert np.array_equal(c.debug_get("lw")[:nz], lay["lw"]) and np.array_equal(c.debug_get("uw")[:nz], lay["uw"]), (name, k)
        assert int(c.debug_get("dims")[11]) == 0, (name, k)
        out.append(c)
    return out
