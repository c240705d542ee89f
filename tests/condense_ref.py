"""TEST INFRASTRUCTURE -- what tests/test_lmpc_condense.py, tests/test_lmpc_condense_gpu.py and tests/test_emu_condense.py share: the 60-digit
truths of tests/golden/condense_truth_{shape,rows,edges}.npz (tests/golden/make_condense_golden.py), the families, and the bound the
bank's condensing kernel (libmpc_amd/csrc/lmpc_hetero.hip, lmpc_condense_models) and the host set-up (LmpcController::condense) are held to.

A controller is a dict `ctl`: dims (nx, nu, ny, ph, ch), A, B, C, OW [ny, ph], UW, DUW [nu, ph] and, each optional, umin / umax [nu] (the
input box over the control horizon), xmin / xmax [nx], ymin / ymax [ny] and sX, sU, smin, smax (state, output and scalar rows over the steps
first + 1 .. ph), dumin / dumax [nu, ph] (rate rows), xw [nx], yw [ny], sw (soft weights, inf = hard), P [nx, nx] (terminal weight).
`layout` derives what the host lays out for the kernel from it -- the block of every step, the rows of G in the product's order with their
bounds and soft entries, the box of every decision variable; the tests hold the product's own layout to it entry by entry.

The truths are computed from the definitions (the header of lmpc_hetero.hip, terminal_ref.condensed_hessian):

    S_i = A S_{i-1} + B E_i,   H = sum_i (C S_i)' diag(OW[:, i-1]) (C S_i) + E_i' diag(UW[:, i-1]) E_i + sum_i D_i' diag(DUW[:, i]) D_i + S_ph' P S_ph
    Hinv = H^-1 (of H + delta I, delta = 1e-8 max(1, max diag H), for the regularised family),  G Hinv,  G Hinv G' + diag(g_soft)
    rho = clip(2 / diagonal entry, [1e-6, 1e6]), 1e3 x for an equality, 0 for a variable without a bound
    K = H + 1e-6 I + diag(rho_b) + G' diag(rho_g) G,  Kinv

A controller of 96 or more variables has no dense truth in the fixture: it is built from independent channels (`combine`), each a small
controller with a truth of its own; every array of the large one is the interleaving of the channels' (`family`), exact zeros elsewhere.

The bound, element-wise against the truth in the padded layouts debug_get returns, u = 2^-52, n = nz:

    H, Gr, Gc:                                   C n u max|truth|
    Hinv, G Hinv, G Hinv G' (Y's blocks), Kinv:  C n u kappa_2 max|truth|        (kappa_2 of H; of K for Kinv)
    rho_b, rho_g:                                relative, the bound of the diagonal entry they derive from over that entry

C is not taken from the kernel or from the host set-up: `restate` below is a float64 numpy restatement of the kernel's algorithm (the
roll-out step by step, a right-looking Cholesky, the triangular inverse column by column, Q'Q), and C is 8 times the worst ratio
error / (n u [kappa_2] max|truth|) that the restatement reaches over the families (dare's margin: the order of an MFMA accumulation differs
from numpy's by no more than the doubling steps do there).  The restatement's ratios per family, worst over controllers
(python tests/condense_ref.py prints them):

    shape_nz1         H  0.62  Gr  0.00  Gc  0.00  Y  1.24  rho_b  1.10  rho_g  1.18  Kinv  1.15
    shape_nz3         H  0.31  Gr  0.00  Gc  0.00  Y  0.07  rho_b  0.03  rho_g  0.02  Kinv  0.09
    shape_nz15        H  0.10  Gr  0.04  Gc  0.04  Y  0.01  rho_b  0.01  rho_g  0.00  Kinv  0.03
    shape_nz16        H  0.12  Gr  0.10  Gc  0.10  Y  0.01  rho_b  0.01  rho_g  0.00  Kinv  0.02
    shape_nz17        H  0.10  Gr  0.05  Gc  0.05  Y  0.01  rho_b  0.01  rho_g  0.00  Kinv  0.02
    shape_nz20        H  0.09  Gr  0.02  Gc  0.02  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.02
    shape_nz33        H  0.05  Gr  0.02  Gc  0.02  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.01
    shape_nz48        H  0.03  Gr  0.01  Gc  0.01  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.00
    rows_mg0          H  0.29  Gr  0.00  Gc  0.00  Y  0.02  rho_b  0.02  rho_g  0.00  Kinv  0.07
    rows_mg1          H  0.27  Gr  0.00  Gc  0.00  Y  0.05  rho_b  0.05  rho_g  0.04  Kinv  0.02
    rows_mg15         H  0.17  Gr  0.12  Gc  0.12  Y  0.07  rho_b  0.07  rho_g  0.03  Kinv  0.06
    rows_mg16         H  0.26  Gr  0.14  Gc  0.14  Y  0.03  rho_b  0.02  rho_g  0.03  Kinv  0.03
    rows_mg17         H  0.32  Gr  0.06  Gc  0.06  Y  0.11  rho_b  0.09  rho_g  0.08  Kinv  0.10
    rows_mg20         H  0.17  Gr  0.16  Gc  0.16  Y  0.07  rho_b  0.06  rho_g  0.05  Kinv  0.14
    rows_mg28         H  0.28  Gr  0.24  Gc  0.24  Y  0.09  rho_b  0.05  rho_g  0.07  Kinv  0.04
    features          H  0.18  Gr  0.19  Gc  0.19  Y  0.03  rho_b  0.03  rho_g  0.02  Kinv  0.01
    edge_lds96        H  0.02  Gr  0.00  Gc  0.00  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.00
    edge_big98        H  0.02  Gr  0.01  Gc  0.01  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.00
    edge_bytes84      H  0.05  Gr  0.04  Gc  0.04  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.00
    cond_well         H  0.08  Gr  0.13  Gc  0.13  Y  0.01  rho_b  0.01  rho_g  0.01  Kinv  0.03
    cond_chain        H  0.18  Gr  0.00  Gc  0.00  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.01
    cond_regularised  H  0.23  Gr  0.14  Gc  0.14  Y  0.00  rho_b  0.00  rho_g  0.00  Kinv  0.00

The worst is the 1 x 1 controller (n = 1 and kappa_2 = 1 leave the bound nothing but the roundings of a few scalar operations): 1.243 on
Hinv, taken as 1.25; C = 8 x 1.25 = 10.
"""
import json
import os

import numpy as np

U = 2.0 ** -52
C_BOUND = 8 * 1.25
INF = float("inf")
KAPPA, RHO_MIN, RHO_MAX, EQ_SCALE, SIGMA = 2.0, 1e-6, 1e6, 1e3, 1e-6
_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = [os.path.join(_HERE, "golden", "condense_truth_%s.npz" % part) for part in ("shape", "rows", "edges")]
K = 4                                                                  # controllers per family
ARRAYS = ("H", "Gr", "Gc", "Y", "rho_b", "rho_g", "Kinv")
SYMMETRIC = ("H", "Hinv", "GHG", "Kinv")                            # stored as their upper triangles
OPTIONAL = ("umin", "umax", "xmin", "xmax", "ymin", "ymax", "first", "sX", "sU", "smin", "smax", "dumin", "dumax", "xw", "yw", "sw", "P")

# name -> the records of its K controllers: one record each (a dense truth) or the channels a controller is built from
SHAPE = ["shape_nz1", "shape_nz3", "shape_nz15", "shape_nz16", "shape_nz17", "shape_nz20", "shape_nz33", "shape_nz48"]
ROWS = ["rows_mg0", "rows_mg1", "rows_mg15", "rows_mg16", "rows_mg17", "rows_mg20", "rows_mg28"]
FEATURES = ["features"]
EDGES = ["edge_lds96", "edge_big98", "edge_bytes84"]
CONDITIONING = ["cond_well", "cond_chain", "cond_regularised"]
FAMILIES = SHAPE + ROWS + FEATURES + EDGES + CONDITIONING
# (pool size, channels per controller): controller k takes the channels k, k + 1, ... of the pool, cyclically -- four different dense problems
CHANNELS = {"shape_nz20": (5, 2), "shape_nz33": (6, 3), "shape_nz48": (7, 4), "edge_lds96": (5, 4), "edge_big98": (8, 7), "edge_bytes84": (13, 12),
            "assembly_nz8": (2, 2)}


def file_of(name):
    """which of GOLDEN holds a family's records"""
    return 0 if name in SHAPE + ["assembly_nz8"] else 2 if name in EDGES else 1


def members(name):
    """the record names of the K controllers of a family: [[record], ...] or [[channel, channel, ...], ...]"""
    if name in CHANNELS:
        pool, per = CHANNELS[name]
        return [["%s.c%d" % (name, (k + c) % pool) for c in range(per)] for k in range(1 if name == "assembly_nz8" else K)]
    return [["%s.%d" % (name, k)] for k in range(K)]


# ---------------------------------------------------------------------------------------------
# what the host lays out for the kernel
# ---------------------------------------------------------------------------------------------
def layout(ctl):
    """dict(nf, nz, blk [ph + 1], kind, step, comp, lo, hi, soft [mg], lw, uw [nz]): the rows of G in the product's order -- per step the
    state, output, scalar and rate rows that have a finite bound"""
    nx, nu, ny, ph, ch = (int(v) for v in ctl["dims"])
    nf = min(ph, ch + 1)
    nz = nf * nu
    blk = [0] + [min(i, nf) - 1 for i in range(1, ph + 1)]
    first = int(ctl.get("first", 0))
    soft_any = any(k in ctl and np.isfinite(np.asarray(ctl[k], float)).any() for k in ("xw", "yw", "sw"))
    assert not (soft_any and first == 0), "a soft step-0 row is a general row without coefficients: not among these families"
    fin = lambda lo, hi: bool(np.isfinite(lo) or np.isfinite(hi))
    inv = lambda key, j: (1.0 / float(np.atleast_1d(ctl[key])[j]) if key in ctl and np.isfinite(np.atleast_1d(ctl[key])[j]) else 0.0)
    rows = []
    for i in range(1, ph + 1):
        bounded = i >= first + 1              # a slice (first, ph) of user columns: user column i - 1 is step i
        if bounded and "xmin" in ctl:
            rows += [(0, i, j, ctl["xmin"][j], ctl["xmax"][j], inv("xw", j)) for j in range(nx) if fin(ctl["xmin"][j], ctl["xmax"][j])]
        if bounded and "ymin" in ctl:
            rows += [(1, i, j, ctl["ymin"][j], ctl["ymax"][j], inv("yw", j)) for j in range(ny) if fin(ctl["ymin"][j], ctl["ymax"][j])]
        if bounded and "sX" in ctl and fin(ctl["smin"], ctl["smax"]):
            rows.append((2, i, 0, float(ctl["smin"]), float(ctl["smax"]), inv("sw", 0)))
        if "dumin" in ctl and i - 1 <= ch:
            rows += [(3, i, j, ctl["dumin"][j, i - 1], ctl["dumax"][j, i - 1], 0.0) for j in range(nu) if fin(ctl["dumin"][j, i - 1], ctl["dumax"][j, i - 1])]
    lw, uw = np.full(nz, -INF), np.full(nz, INF)
    if "umin" in ctl:
        for i in range(1, ph + 1):
            if min(i, ph - 1) < ch:           # step i takes column min(i, ph - 1) of the box, set on the columns 0 .. ch - 1
                for j in range(nu):
                    q = blk[i] * nu + j
                    lw[q] = max(lw[q], ctl["umin"][j]); uw[q] = min(uw[q], ctl["umax"][j])
    col = lambda k, t: np.array([r[k] for r in rows], dtype=t)
    return dict(nf=nf, nz=nz, blk=np.array(blk), kind=col(0, int), step=col(1, int), comp=col(2, int), lo=col(3, float), hi=col(4, float),
                soft=col(5, float), lw=lw, uw=uw)


def combine(chans):
    """one controller of independent channels: block-diagonal A, B, C and P, everything else side by side; its decision vector is
    [block][input], so the channels' variables interleave"""
    ph, ch = chans[0]["dims"][3:]
    assert all(tuple(c["dims"][3:]) == (ph, ch) and c.get("first", 0) == chans[0].get("first", 0) and "sX" not in c for c in chans)

    def bd(key):
        out = np.zeros((sum(c[key].shape[0] for c in chans), sum(c[key].shape[1] for c in chans)))
        r = s = 0
        for c in chans:
            m = c[key]
            out[r:r + m.shape[0], s:s + m.shape[1]] = m
            r += m.shape[0]; s += m.shape[1]
        return out
    big = dict(dims=tuple(int(sum(c["dims"][k] for c in chans)) for k in range(3)) + (int(ph), int(ch)), A=bd("A"), B=bd("B"), C=bd("C"))
    for key in ("OW", "UW", "DUW") + OPTIONAL:
        has = [key in c for c in chans]
        if not any(has):
            continue
        assert all(has), key
        big[key] = chans[0][key] if key == "first" else bd("P") if key == "P" else np.concatenate([np.atleast_1d(c[key]) for c in chans], axis=0)
    return big


def _channel_maps(chans, big_lay):
    """per channel: the large controller's indices of its decision variables and of its rows"""
    offs = np.cumsum([[0, 0, 0]] + [list(c["dims"][:3]) for c in chans], axis=0)          # nx, nu, ny offsets
    nu_all = int(offs[-1][1])
    where = {(int(k), int(s), int(c)): r for r, (k, s, c) in enumerate(zip(big_lay["kind"], big_lay["step"], big_lay["comp"]))}
    out = []
    for c, ctl in enumerate(chans):
        lay = layout(ctl)
        nu = int(ctl["dims"][1])
        var = np.array([b * nu_all + offs[c][1] + j for b in range(lay["nf"]) for j in range(nu)], dtype=int)
        off = {0: offs[c][0], 1: offs[c][2], 3: offs[c][1]}
        row = np.array([where[(int(k), int(s), int(j) + int(off[int(k)]))] for k, s, j in zip(lay["kind"], lay["step"], lay["comp"])], dtype=int)
        out.append((var, row))
    return out


# ---------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------
_records = {}


def _tri(n):
    return np.triu_indices(n)


def pack(name, a):
    return a[_tri(a.shape[0])] if name in SYMMETRIC else a


def _unpack(name, a, n):
    if name not in SYMMETRIC:
        return a
    out = np.zeros((n, n))
    out[_tri(n)] = a
    return out + np.triu(out, 1).T


def record(name):
    """(ctl, truth) of one stored record; truth: H, G, Hinv, GH, GHG (with g_soft on its diagonal), Kinv, rho_b, rho_g, lam (smallest and largest
    eigenvalue of H -- of H + delta I where regularised -- and of K), reg"""
    if not _records:
        for path in GOLDEN:
            with np.load(path) as z:                  # one vector of doubles and the index of the arrays in it
                data, at = z["data"], 0
                for k, shape in json.loads(z["index"].tobytes().decode()):
                    rec, key = k.rsplit(".", 1)
                    n = int(np.prod(shape))
                    _records.setdefault(rec, {})[key] = data[at:at + n].reshape(shape).copy()
                    at += n
    raw = _records[name]
    ctl = {k: v for k, v in raw.items() if not k.startswith("t_")}
    ctl["dims"] = tuple(int(v) for v in ctl["dims"])
    for k in ("first", "smin", "smax", "sw"):
        if k in ctl:
            ctl[k] = int(ctl[k]) if k == "first" else float(ctl[k])
    nz, mg = layout(ctl)["nz"], len(layout(ctl)["kind"])
    tr = {k[2:]: _unpack(k[2:], v, mg if k == "t_GHG" else nz) for k, v in raw.items() if k.startswith("t_")}
    tr["reg"] = bool(tr["reg"])
    for v in list(ctl.values()) + list(tr.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ctl, tr


_families = {}


def family(name):
    """[(ctl, layout, truth)] of the K controllers of a family, the channel-built ones assembled"""
    if name in _families:
        return _families[name]
    out = []
    for recs in members(name):
        parts = [record(r) for r in recs]
        if name not in CHANNELS:
            ctl, tr = parts[0]
            out.append((ctl, layout(ctl), tr))
            continue
        chans = [p[0] for p in parts]
        ctl = combine(chans)
        lay = layout(ctl)
        nz, mg = lay["nz"], len(lay["kind"])
        tr = dict(H=np.zeros((nz, nz)), Hinv=np.zeros((nz, nz)), Kinv=np.zeros((nz, nz)), G=np.zeros((mg, nz)), GH=np.zeros((mg, nz)),
                  GHG=np.zeros((mg, mg)), rho_b=np.zeros(nz), rho_g=np.zeros(mg), reg=False)
        for (var, row), (_, t) in zip(_channel_maps(chans, lay), parts):
            assert not t["reg"]
            for key in ("H", "Hinv", "Kinv"):
                tr[key][np.ix_(var, var)] = t[key]
            for key in ("G", "GH"):
                tr[key][np.ix_(row, var)] = t[key]
            tr["GHG"][np.ix_(row, row)] = t["GHG"]
            tr["rho_b"][var] = t["rho_b"]; tr["rho_g"][row] = t["rho_g"]
        lam = np.array([p[1]["lam"] for p in parts])
        tr["lam"] = np.array([lam[:, 0].min(), lam[:, 1].max(), lam[:, 2].min(), lam[:, 3].max()])
        out.append((ctl, lay, tr))
    _families[name] = out
    return out


# ---------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------
def pad_dims(lay):
    """(nz, mg, ldz, ldg, ldy) of the padded layouts (LmpcController::condense)"""
    nz, mg = lay["nz"], len(lay["kind"])
    ldz = max(2, (nz + 1) // 2 * 2)
    ldg = max(2, (mg + 1) // 2 * 2)
    return nz, mg, ldz, ldg, ldz + ldg


LDS_LIMIT = 160 * 1024


def condense_lds(nx, ny, nz, mg):
    """(bytes of LDS, scratch form?) of the kernel for these dimensions: lmpc_condense_lds restated (P [NP x ld] | Q [NQ x ld] | Sx [2][nx x ld] |
    CS [max(ny, 1) x ld] | small vectors; P and Q leave the LDS beyond NP = 96 or where the sum exceeds the limit).  More than the limit less 64
    bytes: the bank condenses on the host"""
    NP, MP = (nz + 15) // 16 * 16, (mg + 15) // 16 * 16
    NQ, ld = max(NP, MP), NP + 1
    rest = 2 * nx * ld + max(ny, 1) * ld + ((ny + 3) & ~3) + 4 + NP + NQ + 8
    pq = NP * ld + NQ * ld
    big = NP > 96 or (pq + rest) * 8 > LDS_LIMIT - 64
    return ((0 if big else pq) + rest) * 8, big


def expected(lay, tr):
    """{(array, part): (truth in the padded layout, absolute bound per element / C)}: H, Gr, Gc, the blocks of Y, Kinv, rho_b, rho_g"""
    nz, mg, ldz, ldg, ldy = pad_dims(lay)
    n = nz * U
    kH, kK = tr["lam"][1] / tr["lam"][0], tr["lam"][3] / tr["lam"][2]
    mx = lambda a: float(np.abs(a).max(initial=0.0))
    out = {}

    def sq(a, ld):
        p = np.zeros((ld, ld)); p[:nz, :nz] = a
        return p
    out["H", ""] = (sq(tr["H"], ldz), n * mx(tr["H"]))
    out["Kinv", ""] = (sq(tr["Kinv"], ldz), n * kK * mx(tr["Kinv"]))
    Gr = np.zeros((ldg, ldz)); Gr[:mg, :nz] = tr["G"]
    out["Gr", ""] = (Gr, n * mx(tr["G"]))
    out["Gc", ""] = (Gr.T.copy(), n * mx(tr["G"]))
    zero = np.zeros((ldy, ldy))
    for part, a, r0, c0 in (("Hinv", tr["Hinv"], 0, 0), ("GHinv", tr["GH"], ldz, 0), ("GHinv'", tr["GH"].T, 0, ldz), ("GHinvG'", tr["GHG"], ldz, ldz)):
        p = zero.copy(); p[r0:r0 + a.shape[0], c0:c0 + a.shape[1]] = a
        mask = np.zeros((ldy, ldy), bool); mask[r0:r0 + a.shape[0], c0:c0 + a.shape[1]] = True
        out["Y", part] = (p, n * kH * mx(a), mask)
    # rho = kappa / d: the relative error of d, bounded by bound(d's array) / |d|
    dH, dG = np.abs(np.diag(tr["Hinv"])), np.abs(np.diag(tr["GHG"]))
    rb = np.zeros(ldz); rb[:nz] = tr["rho_b"]
    rg = np.ones(ldg); rg[:mg] = tr["rho_g"]
    bb = np.zeros(ldz); bb[:nz] = tr["rho_b"] * n * kH * mx(tr["Hinv"]) / dH
    bg = np.zeros(ldg); bg[:mg] = tr["rho_g"] * n * kH * mx(tr["GHG"]) / np.maximum(dG, 1e-300)
    out["rho_b", ""] = (rb, bb)
    out["rho_g", ""] = (rg, bg)
    return out


def ratios(lay, tr, got):
    """{array: worst |error| / (bound / C)} of one controller; got: the flat arrays of debug_get (H, Gr, Gc, Y, rho_b, rho_g, Kinv)"""
    out = {}
    for (name, part), ex in expected(lay, tr).items():
        want, bound = ex[0], ex[1]
        a = np.asarray(got[name], float)
        assert a.size == want.size, (name, a.size, want.shape)
        err = np.abs(a.reshape(want.shape) - want)
        err = np.where(np.isfinite(err), err, np.inf)
        if len(ex) == 3:
            err = np.where(ex[2], err, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / bound)                       # (an error where the bound is zero -- a zero truth -- is inf)
        out[name] = max(out.get(name, 0.0), float(r.max(initial=0.0)))
    return out


def written(lay):
    """{array: flat mask of the elements the condensing writes} in the padded layouts; the rest is padding: zeros, ones in rho_g"""
    nz, mg, ldz, ldg, ldy = pad_dims(lay)
    sq = np.zeros((ldz, ldz), bool); sq[:nz, :nz] = True
    gr = np.zeros((ldg, ldz), bool); gr[:mg, :nz] = True
    y = np.zeros((ldy, ldy), bool)
    y[:nz, :nz] = True; y[ldz:ldz + mg, :nz] = True; y[:nz, ldz:ldz + mg] = True; y[ldz:ldz + mg, ldz:ldz + mg] = True
    return {"H": sq.ravel(), "Kinv": sq.ravel(), "Gr": gr.ravel(), "Gc": gr.T.ravel(), "Y": y.ravel(), "rho_b": np.arange(ldz) < nz, "rho_g": np.arange(ldg) < mg}


def relative_bound(tr, lay):
    """the bound's relative size for the inverses of this controller (the generator holds it to 1e-6)"""
    return C_BOUND * lay["nz"] * U * max(tr["lam"][1] / tr["lam"][0], tr["lam"][3] / tr["lam"][2])


def check_family(name, gots, where="", c=None):
    """the accuracy check of one family: gots[k] the arrays of controller k; prints and returns the worst error / bound per array"""
    c = C_BOUND if c is None else c
    fam = family(name)
    assert len(gots) == len(fam)
    worst = {}
    for (ctl, lay, tr), got in zip(fam, gots):
        for k, v in ratios(lay, tr, got).items():
            worst[k] = max(worst.get(k, 0.0), v / c)
    print("condense %s%s: worst error / bound: %s" % (name, where, "  ".join("%s %.4f" % (k, worst[k]) for k in ARRAYS)))
    assert all(v <= 1.0 for v in worst.values()), (name, where, worst)
    return worst


# ---------------------------------------------------------------------------------------------
# the kernel's algorithm in float64 numpy
# ---------------------------------------------------------------------------------------------
def _chol(S, tol):
    """right-looking, as chol_lds; None where a pivot is not above tol"""
    S = S.copy()
    for k in range(S.shape[0]):
        d = S[k, k]
        if not d > tol:
            return None
        sd = np.sqrt(d)
        S[k + 1:, k] *= 1.0 / sd
        S[k, k] = sd
        S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k], S[k + 1:, k])
    return np.tril(S)


def _tri_inverse(L):
    """Q = L^-1 column by column, as tri_inverse_lds"""
    n = L.shape[0]
    Q = np.zeros((n, n))
    for j in range(n):
        Q[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, n):
            Q[i, j] = -(L[i, j:i] @ Q[j:i, j]) / L[i, i]
    return Q


def restate(ctl, lay, drop_cross_term=False):
    """one controller: the flat padded arrays of debug_get plus cost_direct, by the kernel's algorithm in float64.  drop_cross_term leaves the -w
    entries of an increment weight across a block edge out: a defect the check has to notice"""
    nx, nu, ny, ph, ch = ctl["dims"]
    nz, mg, ldz, ldg, ldy = pad_dims(lay)
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
            if not drop_cross_term:
                H[bp * nu + j, bn * nu + j] -= w; H[bn * nu + j, bp * nu + j] -= w
    maxd = np.abs(np.diag(H)).max()
    reg = False
    L = _chol(H, 1e-13 * max(1.0, maxd))
    if L is None:
        reg = True
        L = _chol(H + 1e-8 * max(1.0, maxd) * np.eye(nz), 0.0)
        assert L is not None
    Q = _tri_inverse(L)
    Hinv = Q.T @ Q
    cost_direct = int(reg or np.abs(H @ Hinv - np.eye(nz)).max() > 1e-9)
    GH = G @ Hinv
    GHG = GH @ G.T + np.diag(lay["soft"])
    bounded = np.isfinite(lay["lw"]) | np.isfinite(lay["uw"])
    rb = np.where(bounded, np.clip(KAPPA / np.maximum(np.diag(Hinv), 1e-300) * np.where(lay["lw"] == lay["uw"], EQ_SCALE, 1.0), RHO_MIN, RHO_MAX), 0.0)
    rg = np.clip(KAPPA / np.maximum(np.diag(GHG), 1e-300) * np.where(lay["lo"] == lay["hi"], EQ_SCALE, 1.0), RHO_MIN, RHO_MAX) if mg else np.zeros(0)
    Km = (G.T * rg) @ G + H + np.diag(SIGMA + rb)
    Qk = _tri_inverse(_chol(Km, 0.0))
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
                cost_direct=cost_direct, regularised=reg)


def restatement_ratios():
    """{family: {array: worst ratio error / (n u [kappa_2] max|truth|)}} of the restatement against the truths"""
    out = {}
    for name in FAMILIES:
        worst = {}
        for ctl, lay, tr in family(name):
            for k, v in ratios(lay, tr, restate(ctl, lay)).items():
                worst[k] = max(worst.get(k, 0.0), v)
        out[name] = worst
    return out


# ---------------------------------------------------------------------------------------------
# the controllers on the product
# ---------------------------------------------------------------------------------------------
def configure(c, ctl, seed=0, maximum_iteration=2000):
    """the controller of `ctl` on a libmpc_amd.LMPC (ndu = 0), with references of its own (they do not enter the condensing)"""
    from libmpc_amd import LParameters
    nx, nu, ny, ph, ch = ctl["dims"]
    first = int(ctl.get("first", 0))
    assert c.setStateSpaceModel(ctl["A"], ctl["B"], ctl["C"])
    assert c.setObjectiveWeights(np.array(ctl["OW"]), np.array(ctl["UW"]), np.array(ctl["DUW"]))
    if "umin" in ctl:
        assert c.setInputBounds(np.array(ctl["umin"]), np.array(ctl["umax"]), (0, ch))
    if "xmin" in ctl:
        assert c.setStateBounds(np.array(ctl["xmin"]), np.array(ctl["xmax"]), (first, ph))
    if "ymin" in ctl:
        assert c.setOutputBounds(np.array(ctl["ymin"]), np.array(ctl["ymax"]), (first, ph))
    if "sX" in ctl:
        assert c.setScalarConstraint(ctl["smin"], ctl["smax"], np.array(ctl["sX"]), np.array(ctl["sU"]), (first, ph))
    r = np.random.default_rng(1000 + seed)
    assert c.setReferences(0.3 * r.normal(size=(ny, ph)), np.zeros((nu, ph)), np.zeros((nu, ph)))
    if "dumin" in ctl:
        assert c.setInputRateBounds(np.array(ctl["dumin"]), np.array(ctl["dumax"]))
    if any(k in ctl for k in ("xw", "yw", "sw")):
        assert c.setSoftConstraintWeights(ctl.get("xw"), ctl.get("yw"), ctl.get("sw"), (first, ph))
    if "P" in ctl:
        assert c.setTerminalCost(np.array(ctl["P"]))
    c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration))
    return c


def host_controllers(name):
    """the K host-only controllers of a family, their layout held to `layout` entry by entry"""
    from libmpc_amd import LMPC
    out = []
    for k, (ctl, lay, tr) in enumerate(family(name)):
        nx, nu, ny, ph, ch = ctl["dims"]
        c = configure(LMPC(nx, nu, 0, ny, ph, ch, device=-1), ctl, seed=k)
        nz, mg, ldz, ldg, ldy = pad_dims(lay)
        assert [int(v) for v in c.debug_get("dims")[:5]] == [nz, mg, ldz, ldg, ldy], (name, k, c.debug_get("dims")[:5], (nz, mg, ldz, ldg, ldy))
        for key, want in (("g_kind", lay["kind"]), ("g_step", lay["step"]), ("g_comp", lay["comp"]), ("lg0", lay["lo"]), ("ug0", lay["hi"]),
                          ("g_soft", lay["soft"])):
            assert np.array_equal(c.debug_get(key)[:mg], want), (name, k, key)
        assert np.array_equal(c.debug_get("lw")[:nz], lay["lw"]) and np.array_equal(c.debug_get("uw")[:nz], lay["uw"]), (name, k)
        assert int(c.debug_get("dims")[11]) == int(tr["reg"]), (name, k)
        out.append(c)
    return out


def arrays_of(get):
    return {n: get(n) for n in ARRAYS}


if __name__ == "__main__":
    r = restatement_ratios()
    for name, w in r.items():
        print("    %-17s %s" % (name, "  ".join("%s %5.2f" % (k, w[k]) for k in ARRAYS)))
    worst = max(max(w.values()) for w in r.values())
    print("worst %.3f, 8 x worst = %.2f (C = %.2f)" % (worst, 8 * worst, C_BOUND))
