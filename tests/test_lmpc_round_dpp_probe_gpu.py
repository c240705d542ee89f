"""Round 12 of the lean polish round, at the level of one working-set solve: the Gauss-Jordan elimination of ws_solve_reg (csrc/lmpc_fast.hip) with the pivot
row and the right-hand side taken by the FMA itself as a DPP row broadcast (fmac_row_bcast, v_fmac_f64_dpp row_newbcast:K), against the form with two
v_readlane_b32 per entry, through mpcx_lmpc_debug_ws_solve: one wavefront per problem, both forms on the same inputs, every result field returned.  No
floating-point operation differs between the forms, so every field must carry the same bits: dep_at, lmax, lam[0..16), w and G w of all 64 lanes.

Problems: n = 24 (16 decision variables and 8 general rows in the unified index, leading dimension 26), Y = L L' + I from a seeded factor, a working set of
na distinct rows, na = 1..16 -- every size class (4, 6, ..., 16 rows) with its smallest and its largest set.  Non-finite inputs are not compared here
(lane K's row turns NaN where it stayed inf: test_lmpc_round_dpp_gpu.py holds what becomes of such an instance)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NZ, LDY, CAP, LEN = 24, 16, 26, 16, 274
SIZES = list(range(1, 17))


def _base(r, na):
    L = r.standard_normal((N, N))
    Y = L @ L.T + np.eye(N)
    Y = 0.5 * (Y + Y.T)
    idx = r.permutation(N)[:na]
    wsb = r.standard_normal(na)
    t0 = r.standard_normal(N)
    return Y, idx, wsb, t0


def _plain(r, na):
    return _base(r, na)


def _scaled(r, na):
    """D Y D with D = 10^U(-75, 75): the entries span 1e-150 .. 1e150, the Schur matrix stays positive definite with the same relative pivots"""
    Y, idx, wsb, t0 = _base(r, na)
    d = 10.0 ** r.uniform(-75, 75, size=N)
    return Y * d[:, None] * d[None, :], idx, wsb * d[idx], t0 * d


def _blocks(r, na):
    """Y[A, A] block diagonal (two blocks, rows dealt at random), the entries between the blocks exact zeros of either sign: multipliers +0 and -0"""
    Y, idx, wsb, t0 = _base(r, na)
    side = r.integers(0, 2, size=na)
    for i in range(na):
        for j in range(i):
            if side[i] != side[j]:
                z = -0.0 if r.random() < 0.5 else 0.0
                Y[idx[i], idx[j]] = z
                Y[idx[j], idx[i]] = z
    return Y, idx, wsb, t0


def _negzero_rhs(r, na):
    """right-hand side entries t0[q] - b that are -0.0 ((-0) - (+0)) and +0.0, at least one of each sign where na allows; na = 1 alternates"""
    Y, idx, wsb, t0 = _base(r, na)
    pick = r.random(na) < 0.6
    pick[0] = True
    for k in np.nonzero(pick)[0]:
        neg = (k % 2 == 0) if na > 1 else (r.random() < 0.5)
        t0[idx[k]] = -0.0 if neg else 0.0
        wsb[k] = 0.0
    return Y, idx, wsb, t0


def _repeated(r, na):
    """one row twice in the working set: its second occurrence has a vanishing pivot (na = 1 has no second row and stays regular)"""
    Y, idx, wsb, t0 = _base(r, na)
    if na > 1:
        a, b = sorted(r.choice(na, size=2, replace=False))
        idx[b] = idx[a]
    return Y, idx, wsb, t0


KINDS = [("plain", _plain, 32), ("scaled", _scaled, 8), ("blocks", _blocks, 8), ("negzero_rhs", _negzero_rhs, 8), ("repeated", _repeated, 8)]


def _problems():
    probs = []
    for kind, make, seeds in KINDS:
        for na in SIZES:
            for s in range(seeds):
                r = np.random.default_rng([1212, len(kind), na, s])
                probs.append((kind, na) + make(r, na))
    return probs


@pytest.fixture(scope="module")
def probe():
    """every problem once, one launch: the inputs and out [count][form][LEN]"""
    import torch
    from libmpc_amd import _capi
    lib = _capi.lib()
    probs = _problems()
    cnt = len(probs)
    Y = np.zeros((cnt, N, LDY)); idx = np.zeros((cnt, CAP), dtype=np.int32); wsb = np.zeros((cnt, CAP)); t0 = np.zeros((cnt, N))
    na = np.zeros(cnt, dtype=np.int32)
    for p, (_, n_a, y, i, b, t) in enumerate(probs):
        Y[p, :, :N] = y; idx[p, :n_a] = i; wsb[p, :n_a] = b; t0[p] = t; na[p] = n_a
    d = [torch.from_numpy(a).cuda() for a in (Y, idx, wsb, na, t0)]
    out = torch.zeros((cnt, 2, LEN), dtype=torch.float64, device="cuda")
    _capi.check(lib.mpcx_lmpc_debug_ws_solve(C.c_void_p(d[0].data_ptr()), N, LDY, NZ, C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()),
                                             C.c_void_p(d[3].data_ptr()), C.c_void_p(d[4].data_ptr()), C.c_void_p(out.data_ptr()), cnt, None))
    torch.cuda.synchronize()
    return probs, out.cpu().numpy()


def _rows(probs, kind):
    return np.array([p for p, q in enumerate(probs) if q[0] == kind])


def test_the_symbol_is_exported():
    from libmpc_amd import _capi
    assert "mpcx_lmpc_debug_ws_solve" in _capi.EXPORTS


@pytest.mark.parametrize("kind", [k[0] for k in KINDS])
def test_both_forms_bit_for_bit(probe, kind):
    probs, out = probe
    rows = _rows(probs, kind)
    assert sorted(set(probs[p][1] for p in rows)) == SIZES
    a, b = out[rows, 0], out[rows, 1]
    assert not np.isnan(a).any() and not np.isnan(b).any()                  # finite inputs: nothing to match loosely
    same = a.view(np.uint64) == b.view(np.uint64)
    assert same.all(), (kind, "problem (na), field", [(int(rows[i]), probs[rows[i]][1], int(f)) for i, f in np.argwhere(~same)[:8]])
    dep = a[:, 0]
    if kind == "repeated":
        multi = np.array([probs[p][1] > 1 for p in rows])
        assert (dep[multi] >= 0).all() and (dep[~multi] == -1).all(), dep.tolist()
        # the dependent row is the second occurrence of the repeated index
        for i in np.nonzero(multi)[0]:
            idx = probs[rows[i]][3]
            second = [k for k in range(len(idx)) if idx[k] in idx[:k]]
            assert int(dep[i]) == second[0], (int(rows[i]), idx.tolist(), dep[i])
    else:
        assert (dep == -1).all(), (kind, dep.tolist())


def test_the_scalar_form_solves_the_system(probe):
    """the forms agree with each other above; here form 0 is the solve this test believes it is.  lambda = Y[A, A]^-1 (t0[A] - b) and w = t0 - Y[:, A] lambda,
    against numpy: Gauss-Jordan without pivoting on a positive definite matrix is backward stable, so the error of lambda is bounded by a small multiple of
    na eps cond(Y[A, A]) |lambda| (64 na eps cond is taken), and w's by that times |Y[:, A]| summed, plus the rounding of its na FMAs"""
    probs, out = probe
    eps = np.finfo(float).eps
    for p in _rows(probs, "plain"):
        _, na, Y, idx, wsb, t0 = probs[p]
        S = Y[np.ix_(idx, idx)]
        lam = np.linalg.solve(S, t0[idx] - wsb)
        got = out[p, 0, 2:2 + CAP]
        tol = 64 * na * eps * np.linalg.cond(S) * np.abs(lam).max()
        assert np.abs(got[:na] - lam).max() <= tol and (got[na:] == 0).all(), (p, na)
        assert out[p, 0, 1] == np.abs(got[:na]).max()                        # lmax
        w = t0 - Y[:, idx] @ got[:na]
        wtol = np.abs(Y[:, idx]).sum(axis=1).max() * tol + 4 * (na + 1) * eps * (np.abs(t0).max() + (np.abs(Y[:, idx]) @ np.abs(got[:na])).max())
        wv = out[p, 0, 2 + CAP:2 + CAP + 128][:NZ]
        gw = out[p, 0, 2 + CAP + 128:][:N - NZ]
        assert np.abs(wv - w[:NZ]).max() <= wtol and np.abs(gw - w[NZ:]).max() <= wtol, (p, na)


def test_the_cases_reach_the_edges(probe):
    """what the special cases are there for does occur: multipliers and right-hand sides of both zero signs, entries at both ends of the range"""
    probs, out = probe
    neg = pos = 0
    for p in _rows(probs, "negzero_rhs"):
        _, na, Y, idx, wsb, t0 = probs[p]
        y = t0[idx] - wsb
        neg += int(((y == 0) & np.signbit(y)).sum()); pos += int(((y == 0) & ~np.signbit(y)).sum())
    assert neg >= 16 and pos >= 16, (neg, pos)
    # na = 1 with y = -0: the multiplier is -0 x 1 / pivot = -0, the one place where the sign of lane K's own zero reaches a result
    ones = [p for p in _rows(probs, "negzero_rhs") if probs[p][1] == 1]
    signs = [bool(np.signbit(out[p, 0, 2])) for p in ones]
    assert all(out[p, 0, 2] == 0 for p in ones) and any(signs) and not all(signs), signs
    zneg = zpos = 0
    for p in _rows(probs, "blocks"):
        _, na, Y, idx, wsb, t0 = probs[p]
        S = Y[np.ix_(idx, idx)]
        zneg += int(((S == 0) & np.signbit(S)).sum()); zpos += int(((S == 0) & ~np.signbit(S)).sum())
    assert zneg >= 64 and zpos >= 64, (zneg, zpos)
    mags = np.concatenate([np.abs(probs[p][2]).ravel() for p in _rows(probs, "scaled")])
    assert mags.min() < 1e-140 and mags.max() > 1e140, (mags.min(), mags.max())
