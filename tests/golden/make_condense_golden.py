"""Writes tests/golden/condense_truth_shape.npz, condense_truth_rows.npz and condense_truth_edges.npz: the 60-digit truths that the bank's condensing kernel
(libmpc_amd/csrc/lmpc_hetero.hip, lmpc_condense_models) and the host set-up (LmpcController::condense) are held to, read by tests/condense_ref.py
for tests/test_lmpc_condense.py, tests/test_lmpc_condense_gpu.py and tests/test_emu_condense.py.  Needs mpmath; run from the repository root:

    python tests/golden/make_condense_golden.py

Every record is one controller (tests/condense_ref.py describes the dict): its inputs, and H, G, Hinv, G Hinv, G Hinv G' + diag(g_soft), rho_b, rho_g
and Kinv from their definitions in 60-digit arithmetic -- the roll-out S_i = A S_{i-1} + B E_i, the sums of the cost's terms, inverses by
mpmath -- rounded to double at the end; symmetric matrices as their upper triangles.  The extreme eigenvalues of H and K (for kappa_2) come
from numpy on the rounded truths: three digits of a condition number are enough for a bound.  Controllers of 96 and more variables are stored
as the independent channels they are built from.  Three files, so that each stays at the size of the other truths here.  The conditions of the families are checked here:

  * the bound's relative size C n u kappa_2 is at most 1e-6 in every family but the regularised one;
  * the smallest Cholesky pivot of H is at least 1e-9 max diag H -- four decades from the regularisation threshold 1e-13;
  * the regularised family has an exactly zero row and column of H, and its truth is that of H + delta I, delta = 1e-8 max(1, max diag H)."""
import io
import json
import os
import sys
import zipfile
import zlib

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import condense_ref as R          # noqa: E402

mp.mp.dps = 60
INF = float("inf")


def truth(ctl, regularised=False):
    lay = R.layout(ctl)
    nx, nu, ny, ph, ch = ctl["dims"]
    nz, blk = lay["nz"], lay["blk"]
    mg = len(lay["kind"])
    M = lambda a: mp.matrix(np.asarray(a, float).tolist())
    A, B, C = M(ctl["A"]), M(ctl["B"]), M(ctl["C"])

    def E(i):
        e = mp.zeros(nu, nz)
        for j in range(nu):
            e[j, int(blk[i]) * nu + j] = 1
        return e
    diag = lambda v: mp.diag([mp.mpf(float(x)) for x in v])
    S = mp.zeros(nx, nz)
    H = mp.zeros(nz, nz)
    G = mp.zeros(max(mg, 1), nz)
    for i in range(1, ph + 1):
        S = A * S + B * E(i)
        CS = C * S
        H += CS.T * diag(ctl["OW"][:, i - 1]) * CS + E(i).T * diag(ctl["UW"][:, i - 1]) * E(i)      # user column i - 1 weighs step i
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
    # Cholesky pivots of the truth
    L = H.copy()
    minpiv = None
    for k in range(nz):
        d = L[k, k]
        minpiv = d if minpiv is None else min(minpiv, d)
        if not d > 0:
            break
        for i in range(k + 1, nz):
            f = L[i, k] / d
            for j in range(k + 1, i + 1):
                L[i, j] -= f * L[j, k]
    if regularised:
        zero = [q for q in range(nz) if all(H[q, p] == 0 for p in range(nz))]
        assert zero, "the regularised family needs an exactly zero row and column of H"
        assert minpiv == 0
        Hr = H + mp.mpf(10) ** -8 * max(mp.mpf(1), maxd) * mp.eye(nz)
    else:
        assert minpiv >= mp.mpf(10) ** -9 * maxd, ("smallest pivot", float(minpiv / maxd))
        Hr = H
    Hinv = mp.inverse(Hr)
    Hinv = (Hinv + Hinv.T) / 2
    clip = lambda v: min(max(v, mp.mpf(R.RHO_MIN)), mp.mpf(R.RHO_MAX))
    rb = []
    for q in range(nz):
        lo, hi = lay["lw"][q], lay["uw"][q]
        if not (np.isfinite(lo) or np.isfinite(hi)):
            rb.append(mp.mpf(0))
            continue
        rb.append(clip(mp.mpf(R.KAPPA) / Hinv[q, q] * (mp.mpf(R.EQ_SCALE) if lo == hi else 1)))
    if mg:
        GH = G * Hinv
        GHG = GH * G.T + diag(lay["soft"])
        GHG = (GHG + GHG.T) / 2
        rg = [clip(mp.mpf(R.KAPPA) / GHG[r, r] * (mp.mpf(R.EQ_SCALE) if lay["lo"][r] == lay["hi"][r] else 1)) for r in range(mg)]
        Kk = H + G.T * mp.diag(rg) * G
    else:
        rg, Kk = [], H.copy()
    for q in range(nz):
        Kk[q, q] += mp.mpf(R.SIGMA) + rb[q]
    Kinv = mp.inverse(Kk)
    Kinv = (Kinv + Kinv.T) / 2
    f = lambda X, r, c: np.array([[float(X[i, j]) for j in range(c)] for i in range(r)], dtype=float).reshape(r, c)
    out = dict(H=f(H, nz, nz), G=f(G, mg, nz), Hinv=f(Hinv, nz, nz), Kinv=f(Kinv, nz, nz), rho_b=np.array([float(v) for v in rb]),
               rho_g=np.array([float(v) for v in rg], dtype=float))
    out["GH"] = f(GH, mg, nz) if mg else np.zeros((0, nz))
    out["GHG"] = f(GHG, mg, mg) if mg else np.zeros((0, 0))
    eh = np.linalg.eigvalsh(f(Hr, nz, nz)); ek = np.linalg.eigvalsh(f(Kk, nz, nz))
    out["lam"] = np.array([eh[0], eh[-1], ek[0], ek[-1]])
    out["reg"] = np.array(int(regularised))
    # a hard row without coefficients would be a feasibility row on the host, not a row of G
    assert all(np.abs(out["G"][r]).max() > 1e-6 for r in range(mg))
    return lay, out


def rand_ctl(rng, nx, nu, ny, ph, ch, box=0.6, xb=(), yb=(), first=0, scalar=False, rate=(), soft=None, terminal=False, radius=0.9, equal_box=None):
    """a random stable controller.  box: the input box' size or None; xb, yb: the bounded state and output components; rate: [(input, step, lo, hi)];
    soft: dict(xw, yw, sw)"""
    A = rng.normal(size=(nx, nx))
    A *= radius / max(abs(np.linalg.eigvals(A)))
    ctl = dict(dims=(nx, nu, ny, ph, ch), A=A, B=rng.normal(size=(nx, nu)), C=rng.normal(size=(ny, nx)), OW=rng.uniform(0.5, 2.0, size=(ny, ph)),
               UW=rng.uniform(0.05, 0.2, size=(nu, ph)), DUW=rng.uniform(0.01, 0.1, size=(nu, ph)))
    if box is not None:
        b = box * rng.uniform(0.8, 1.2, size=nu)
        ctl.update(umin=-b, umax=b.copy())
        if equal_box is not None:
            ctl["umin"][equal_box] = ctl["umax"][equal_box] = 0.1
    if len(xb):
        lo, hi = np.full(nx, -INF), np.full(nx, INF)
        for j in xb:
            lo[j], hi[j] = -rng.uniform(1.5, 2.5), rng.uniform(1.5, 2.5)
        ctl.update(xmin=lo, xmax=hi)
    if len(yb):
        lo, hi = np.full(ny, -INF), np.full(ny, INF)
        for j in yb:
            lo[j], hi[j] = -rng.uniform(2.5, 3.5), rng.uniform(2.5, 3.5)
        ctl.update(ymin=lo, ymax=hi)
    if first:
        ctl["first"] = first
    if scalar:
        ctl.update(sX=rng.normal(size=nx), sU=rng.normal(size=nu), smin=-4.0, smax=4.0)
    if len(rate):
        lo, hi = np.full((nu, ph), -INF), np.full((nu, ph), INF)
        for j, i, a, b in rate:
            lo[j, i], hi[j, i] = a, b
        ctl.update(dumin=lo, dumax=hi)
    if soft:
        ctl.update(soft)
    if terminal:
        F = rng.normal(size=(nx, nx))
        ctl["P"] = F @ F.T / nx
    return ctl


def chain_ctl(rng, ph):
    """a long-horizon integrator chain (position, velocity; the position weighted, the input almost free): kappa_2(H) about 1e6"""
    dt = rng.uniform(0.08, 0.12)
    A = np.array([[1.0, dt], [0.0, 1.0]]); B = np.array([[0.5 * dt * dt], [dt]]); C = np.array([[1.0, 0.0]])
    b = rng.uniform(0.8, 1.2, size=1)
    return dict(dims=(2, 1, 1, ph, ph), A=A, B=B, C=C, OW=rng.uniform(0.8, 1.2, size=(1, ph)), UW=CHAIN_UW * rng.uniform(0.8, 1.2, size=(1, ph)),
                DUW=np.zeros((1, ph)), umin=-b, umax=b.copy())


CHAIN_UW = 4.4e-7


def regularised_ctl(rng):
    """an input with a zero column of B and zero weights: an exactly zero row and column of H"""
    ctl = rand_ctl(rng, 3, 3, 2, 2, 2, xb=(0,))
    ctl["B"][:, 2] = 0.0; ctl["UW"][2, :] = 0.0; ctl["DUW"][2, :] = 0.0
    return ctl


def records():
    """{record name: (ctl, regularised)} of every family of tests/condense_ref.py"""
    rng = None
    recs = {}

    def fam(name, make):
        nonlocal rng
        rng = np.random.default_rng([20250117, zlib.crc32(name.encode())])          # a stream per family: one family's change leaves the others alone
        for recnames in R.members(name):
            for rn in recnames:
                if rn not in recs:
                    recs[rn] = (make(len([k for k in recs if k.startswith(name + ".")])), name == "cond_regularised")
    # shape: nz and ny on either side of the tiles' and the k-steps' edges; ph = 1 and nx = 1 among them.  A state bound on the last two steps
    for name, dims in (("shape_nz1", (1, 1, 1, 1, 1)), ("shape_nz3", (2, 3, 17, 1, 1)), ("shape_nz15", (4, 3, 4, 5, 5)), ("shape_nz16", (3, 2, 5, 8, 8)),
                       ("shape_nz17", (1, 1, 3, 17, 17))):
        fam(name, lambda k, d=dims: rand_ctl(rng, *d, xb=(0,), first=max(d[3] - 2, 0)))
    fam("shape_nz20", lambda k: rand_ctl(rng, 2, 1, 1, 10, 10, xb=(0,), first=8))
    fam("shape_nz33", lambda k: rand_ctl(rng, 2, 1, 1, 11, 11, xb=(0,), first=9))
    fam("shape_nz48", lambda k: rand_ctl(rng, 2, 1, 1, 12, 12, xb=(1,), first=10))
    # rows (mg = 1: the one rate row, and an input held by an equality box): mg = 0, 1, 15, 16, 17, 20 and mg = 28 with nz = 4 (more row tiles
    # than column tiles)
    fam("rows_mg0", lambda k: rand_ctl(rng, 3, 2, 2, 3, 3))
    fam("rows_mg1", lambda k: rand_ctl(rng, 3, 2, 2, 3, 3, rate=[(1, 1, -0.3, 0.2)], equal_box=0))
    fam("rows_mg15", lambda k: rand_ctl(rng, 3, 1, 2, 5, 5, xb=(0, 1, 2)))
    fam("rows_mg16", lambda k: rand_ctl(rng, 3, 1, 2, 5, 5, xb=(0, 1, 2), rate=[(0, 2, -0.3, INF)]))
    fam("rows_mg17", lambda k: rand_ctl(rng, 3, 1, 2, 5, 5, xb=(0, 1, 2), rate=[(0, 2, -0.3, INF), (0, 0, -0.2, 0.2)]))
    fam("rows_mg20", lambda k: rand_ctl(rng, 3, 1, 1, 5, 5, xb=(0, 1, 2), yb=(0,)))
    fam("rows_mg28", lambda k: rand_ctl(rng, 4, 1, 2, 4, 4, xb=(0, 1, 2, 3), yb=(0, 1), rate=[(0, i, -0.3, 0.3) for i in range(4)]))
    # features: move blocking, increment weights, rate rows across the block edge (one an equality), a scalar row, output rows, two kinds of
    # soft row with weights of the controller's own, a full terminal weight with nx = 17
    def features(k):
        c = rand_ctl(rng, 17, 2, 3, 6, 3, xb=(0,), yb=(1,), first=1, scalar=True,
                     rate=[(0, i, -0.3, 0.3) for i in range(4)] + [(1, 0, -0.2, 0.2), (1, 1, 0.0, 0.0), (1, 3, -INF, 0.25)],
                     soft=dict(xw=np.array([10.0 * (k + 1)] + [INF] * 16), sw=3.0 + 7.0 * k), terminal=True)
        c["DUW"] = rng.uniform(0.05, 0.3, size=(2, 6))
        return c
    fam("features", features)
    # form edges, channel-built: nz = 96 in LDS (four channels: with P and Q in it the LDS has room for 2 nx + ny <= 16 more rows), nz = 98 the first scratch shape, nz = 84 with 144 rows (scratch by bytes)
    fam("edge_lds96", lambda k: rand_ctl(rng, 1, 1, 1, 24, 24, xb=(0,), first=21))
    fam("edge_big98", lambda k: rand_ctl(rng, 1, 1, 1, 14, 14, xb=(0,), first=11))
    fam("edge_bytes84", lambda k: rand_ctl(rng, 2, 1, 1, 7, 7, xb=(0, 1), first=1))
    fam("assembly_nz8", lambda k: rand_ctl(rng, 2, 1, 1, 4, 4, xb=(0,), rate=[(0, 1, -0.3, 0.3)]))
    # conditioning
    fam("cond_well", lambda k: rand_ctl(rng, 3, 2, 2, 4, 4, xb=(0,)))
    fam("cond_chain", lambda k: chain_ctl(rng, 16))
    fam("cond_regularised", lambda k: regularised_ctl(rng))
    return recs


def save(path, arrays):
    """one vector of doubles and the index of the arrays in it (a zip member per array would cost more than the numbers); written as
    numpy.savez_compressed writes, with a fixed time stamp on every member: the same bytes on every run"""
    keys = sorted(arrays)
    index = [[k, list(np.shape(arrays[k]))] for k in keys]
    data = np.concatenate([np.asarray(arrays[k], float).ravel() for k in keys])
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in (("data", data), ("index", np.frombuffer(json.dumps(index).encode(), dtype=np.uint8))):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(path, data.size, "doubles")


def main():
    recs = records()
    out = [{}, {}, {}]
    for name, (ctl, reg) in recs.items():
        lay, tr = truth(ctl, reg)
        rel = R.C_BOUND * lay["nz"] * R.U * max(tr["lam"][1] / tr["lam"][0], tr["lam"][3] / tr["lam"][2])
        # (for a channel the large controller's n and the worst channel's kappa_2 count: condense_ref.relative_bound, checked below)
        print("%-20s nz %3d mg %3d  kappa_2(H) %.2e  kappa_2(K) %.2e%s" % (name, lay["nz"], len(lay["kind"]), tr["lam"][1] / tr["lam"][0],
                                                                           tr["lam"][3] / tr["lam"][2], "  regularised" if reg else ""))
        assert reg or rel <= 1e-6, (name, rel)
        dst = out[R.file_of(name.split(".")[0])]
        for k, v in ctl.items():
            dst["%s.%s" % (name, k)] = np.asarray(v)
        for k, v in tr.items():
            dst["%s.t_%s" % (name, k)] = R.pack(k, v)
    # the dense truth of the assembly check: the two channels of assembly_nz8 as one controller
    chans = [recs[r][0] for r in R.members("assembly_nz8")[0]]
    big = R.combine(chans)
    lay, tr = truth(big)
    for k, v in big.items():
        out[0]["assembly_nz8.dense.%s" % k] = np.asarray(v)
    for k, v in tr.items():
        out[0]["assembly_nz8.dense.t_%s" % k] = R.pack(k, v)
    for path, d in zip(R.GOLDEN, out):
        save(path, d)
        print(path, os.path.getsize(path), "bytes")
    R._records.clear(); R._families.clear()
    for name in R.FAMILIES:
        for ctl, lay, tr in R.family(name):
            assert tr["reg"] or R.relative_bound(tr, lay) <= 1e-6, (name, R.relative_bound(tr, lay))


if __name__ == "__main__":
    main()
