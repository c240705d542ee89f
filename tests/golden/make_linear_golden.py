"""Writes tests/golden/condense_truth_linear.npz -- the 60-digit truths of the condensing families with linear rows (tests/linear_ref.py: `linear`,
`linear_bank`), in the record format of tests/golden/make_condense_golden.py -- and tests/golden/linear_oracle.npz, the yardstick's results of the
cases whose solves take seconds (linear_ref.case, linear_ref.large_case).  Needs mpmath; run from the repository root:

    python tests/golden/make_linear_golden.py

A record is one controller: its inputs (condense_ref's dict and Fx, Fu, flo, fhi, fw) and H, G, Hinv, G Hinv, G Hinv G' + diag(g_soft), rho_b,
rho_g, Kinv from their definitions in 60-digit arithmetic, a linear row being Fx(c, :) S_i + Fu(c, :) E_i.  Checked here, as there: the bound's
relative size C n u kappa_2 is at most 1e-6, the smallest Cholesky pivot of H at least 1e-9 max diag H, no row of G without coefficients; and
the float64 restatement of the kernel's algorithm (linear_ref.restate) stays under C_BOUND / 8 on the new families."""
import os
import sys
import zlib

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
import condense_ref as R          # noqa: E402
import linear_ref as LR           # noqa: E402
import make_condense_golden as MC  # noqa: E402

mp.mp.dps = 60
INF = float("inf")


def truth(ctl):
    lay = LR.layout(ctl)
    nx, nu, ny, ph, ch = ctl["dims"]
    nz, blk = lay["nz"], lay["blk"]
    mg = len(lay["kind"])
    M = lambda a: mp.matrix(np.asarray(a, float).tolist())
    A, B, C = M(ctl["A"]), M(ctl["B"]), M(ctl["C"])
    Fx, Fu = M(ctl["Fx"]), M(ctl["Fu"])

    def E(i):
        e = mp.zeros(nu, nz)
        for j in range(nu):
            e[j, int(blk[i]) * nu + j] = 1
        return e
    diag = lambda v: mp.diag([mp.mpf(float(x)) for x in v])
    S = mp.zeros(nx, nz)
    H = mp.zeros(nz, nz)
    G = mp.zeros(mg, nz)
    for i in range(1, ph + 1):
        S = A * S + B * E(i)
        CS = C * S
        FS = Fx * S + Fu * E(i)
        H += CS.T * diag(ctl["OW"][:, i - 1]) * CS + E(i).T * diag(ctl["UW"][:, i - 1]) * E(i)
        for r in range(mg):
            if lay["step"][r] != i:
                continue
            kind, cp = int(lay["kind"][r]), int(lay["comp"][r])
            if kind == 0:
                row = S[cp, :]
            elif kind == 1:
                row = CS[cp, :]
            elif kind == 2:
                row = M(np.atleast_2d(ctl["sX"])) * S + M(np.atleast_2d(ctl["sU"])) * E(i)
            elif kind == 4:
                row = FS[cp, :]
            else:
                row = E(i)[cp, :] - (E(i - 1)[cp, :] if i > 1 else mp.zeros(1, nz))
            G[r, :] = row
    for i in range(ph):
        D = E(i + 1) - (E(i) if i > 0 else mp.zeros(nu, nz))
        H += D.T * diag(ctl["DUW"][:, i]) * D
    if "P" in ctl:
        P = M(ctl["P"])
        H += S.T * ((P + P.T) / 2) * S
    H = (H + H.T) / 2
    maxd = max(abs(H[q, q]) for q in range(nz))
    L = H.copy()
    minpiv = None
    for k in range(nz):
        d = L[k, k]
        minpiv = d if minpiv is None else min(minpiv, d)
        assert d > 0
        for i in range(k + 1, nz):
            f = L[i, k] / d
            for j in range(k + 1, i + 1):
                L[i, j] -= f * L[j, k]
    assert minpiv >= mp.mpf(10) ** -9 * maxd, ("smallest pivot", float(minpiv / maxd))
    Hinv = mp.inverse(H)
    Hinv = (Hinv + Hinv.T) / 2
    clip = lambda v: min(max(v, mp.mpf(R.RHO_MIN)), mp.mpf(R.RHO_MAX))
    rb = []
    for q in range(nz):
        lo, hi = lay["lw"][q], lay["uw"][q]
        if not (np.isfinite(lo) or np.isfinite(hi)):
            rb.append(mp.mpf(0))
            continue
        rb.append(clip(mp.mpf(R.KAPPA) / Hinv[q, q] * (mp.mpf(R.EQ_SCALE) if lo == hi else 1)))
    GH = G * Hinv
    GHG = GH * G.T + diag(lay["soft"])
    GHG = (GHG + GHG.T) / 2
    rg = [clip(mp.mpf(R.KAPPA) / GHG[r, r] * (mp.mpf(R.EQ_SCALE) if lay["lo"][r] == lay["hi"][r] else 1)) for r in range(mg)]
    Kk = H + G.T * mp.diag(rg) * G
    for q in range(nz):
        Kk[q, q] += mp.mpf(R.SIGMA) + rb[q]
    Kinv = mp.inverse(Kk)
    Kinv = (Kinv + Kinv.T) / 2
    f = lambda X, r, c: np.array([[float(X[i, j]) for j in range(c)] for i in range(r)], dtype=float).reshape(r, c)
    out = dict(H=f(H, nz, nz), G=f(G, mg, nz), Hinv=f(Hinv, nz, nz), Kinv=f(Kinv, nz, nz), rho_b=np.array([float(v) for v in rb]),
               rho_g=np.array([float(v) for v in rg], dtype=float), GH=f(GH, mg, nz), GHG=f(GHG, mg, mg))
    eh = np.linalg.eigvalsh(out["H"]); ek = np.linalg.eigvalsh(f(Kk, nz, nz))
    out["lam"] = np.array([eh[0], eh[-1], ek[0], ek[-1]])
    out["reg"] = np.array(0)
    assert all(np.abs(out["G"][r]).max() > 1e-6 for r in range(mg))
    return lay, out


def with_rows(rng, ctl, nc, steps, size=1.0, fw=None, equality=None):
    """nc random linear rows bounded by +-size (every third one-sided) at `steps`; equality: a row with lo == hi"""
    nx, nu, ny, ph, ch = ctl["dims"]
    lo = np.full((nc, ph + 1), -INF); hi = np.full((nc, ph + 1), INF)
    for i in steps:
        lo[:, i] = -size * rng.uniform(0.8, 1.2, size=nc); hi[:, i] = size * rng.uniform(0.8, 1.2, size=nc)
        lo[2::3, i] = -INF
        if equality is not None:
            lo[equality, i] = hi[equality, i]
    ctl.update(Fx=rng.normal(size=(nc, nx)), Fu=rng.normal(size=(nc, nu)), flo=lo, fhi=hi)
    if fw is not None:
        ctl["fw"] = np.asarray(fw, float)
    return ctl


def records():
    recs = {}
    rng = np.random.default_rng([20250117, zlib.crc32(b"linear")])
    # nc = 1, every step from 1 on
    recs["linear.0"] = with_rows(rng, MC.rand_ctl(rng, 3, 2, 2, 4, 4), 1, range(1, 5))
    # nc = 3, rows at the last step only: a terminal set (one an equality), with move blocking
    recs["linear.1"] = with_rows(rng, MC.rand_ctl(rng, 4, 1, 2, 6, 3), 3, [6], equality=1)
    # nc = 16, three steps: 48 rows on 6 variables, more row tiles than column tiles
    recs["linear.2"] = with_rows(rng, MC.rand_ctl(rng, 4, 2, 2, 3, 3), 16, range(1, 4))
    # combined: state, output, scalar, rate and soft rows (one linear row soft) and a terminal cost, move blocking
    c = MC.rand_ctl(rng, 5, 2, 3, 6, 3, xb=(0,), yb=(1,), first=1, scalar=True,
                    rate=[(0, i, -0.3, 0.3) for i in range(4)] + [(1, 0, -0.2, 0.2), (1, 3, -INF, 0.25)],
                    soft=dict(xw=np.array([10.0] + [INF] * 4), sw=5.0), terminal=True)
    recs["linear.3"] = with_rows(rng, c, 2, range(1, 7), fw=[INF, 20.0])
    # one bank: three controllers of one structure, Fx, Fu and bounds of their own
    rng = np.random.default_rng([20250117, zlib.crc32(b"linear_bank")])
    for k in range(3):
        recs["linear_bank.%d" % k] = with_rows(rng, MC.rand_ctl(rng, 3, 2, 2, 5, 5, xb=(0,)), 3, range(1, 6), size=0.6 + 0.2 * k)
    return recs


def oracle_cases():
    """the yardstick's results of the cases whose solves take seconds (linear_ref.case at two ticks, linear_ref.large_case), the active bits
    packed, each with the inputs it was computed for"""
    out = {}

    def put(name, ref, **inputs):
        print("%-14s polished %.2f  active linear rows up to %d  working sets up to %d  iterations up to %d" %
              (name, (ref["polished"] == 1).mean(), ref["n_linear_active"].max(), ref["n_active"].max(), ref["iters"].max()))
        assert (ref["polished"] == 1).mean() >= 0.9, name
        for k, v in ref.items():
            if k in ("y",):
                continue
            out["%s/%s" % (name, k)] = np.packbits(v.astype(np.uint8), axis=1, bitorder="little") if k.startswith("active_") else np.asarray(v)
        for k, v in inputs.items():
            if v is not None:
                out["%s/in_%s" % (name, k)] = v
    for name in ("blocked", "ch=ph", "full"):
        sp, x0, u0, yref, dmeas = LR.case(name)
        ref = LR.solve_batch(sp, x0, u0, yref, dmeas)
        put(name, ref, x0=x0, u0=u0, yref=yref, dmeas=dmeas)
        x1 = LR.next_tick(sp, x0, ref["cmd"], dmeas)
        put(name + " tick 1", LR.solve_batch(sp, x1, ref["cmd"], yref, dmeas), x0=x1, u0=ref["cmd"])
    sp, x0, u0, yref = LR.large_case()
    put("large", LR.solve_batch(sp, x0, u0, yref), x0=x0, u0=u0, yref=yref)
    np.savez_compressed(LR.ORACLE, **out)
    print(LR.ORACLE, os.path.getsize(LR.ORACLE), "bytes")


def main():
    out = {}
    for name, ctl in records().items():
        lay, tr = truth(ctl)
        rel = R.C_BOUND * lay["nz"] * R.U * max(tr["lam"][1] / tr["lam"][0], tr["lam"][3] / tr["lam"][2])
        print("%-16s nz %3d mg %3d  kappa_2(H) %.2e  kappa_2(K) %.2e" % (name, lay["nz"], len(lay["kind"]), tr["lam"][1] / tr["lam"][0], tr["lam"][3] / tr["lam"][2]))
        assert rel <= 1e-6, (name, rel)
        for k, v in ctl.items():
            out["%s.%s" % (name, k)] = np.asarray(v)
        for k, v in tr.items():
            out["%s.t_%s" % (name, k)] = R.pack(k, v)
    MC.save(LR.GOLDEN, out)
    print(LR.GOLDEN, os.path.getsize(LR.GOLDEN), "bytes")
    LR._records.clear()
    worst = 0.0
    for fam in LR.FAMILIES:
        for ctl, lay, tr in LR.family(fam):
            w = R.ratios(lay, tr, LR.restate(ctl, lay))
            print("restatement %-12s %s" % (fam, "  ".join("%s %5.2f" % (k, w[k]) for k in R.ARRAYS)))
            worst = max(worst, max(w.values()))
    print("restatement: worst ratio %.3f (C_BOUND / 8 = %.3f)" % (worst, R.C_BOUND / 8))
    assert worst <= R.C_BOUND / 8
    if "--no-oracle" not in sys.argv:
        oracle_cases()


if __name__ == "__main__":
    main()
