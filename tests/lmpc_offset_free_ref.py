"""The tick of an offset-free loop (mpcx_lmpc_loop_create_offset_free) in float64 numpy, the bounds that go with it, and a host loop around it.

    y_k      = C x_k + Dd delta_k + v_k
    e_k      = y_k - (C xhat_k + Dd dhat_k)
    x_k+1    = A_p x_k + B_p cmd_k + Bd_p delta_k + w_k
    xhat_k+1 = A xhat_k + B cmd_k + Bd dhat_k + Lx e_k
    dhat_k+1 = dhat_k + Ld e_k

Everything is batched: matrices [B, rows, cols] (a 2-D matrix is broadcast), vectors [B, n].  The bounds are componentwise and of the form
(terms + 2) 2^-52 sum|a||b|: a chain of n fused multiply-adds from 0 is off by at most n 2^-53 sum|a||b| (1 + O(2^-53)), an add by 2^-53 times its
result, numpy's own products and sums of the same terms by no more, and one more 2^-52 sum|a||b| covers the terms of second order."""
import numpy as np

EPS = 2.0 ** -52


def mv(M, v):
    """M_b v_b"""
    return np.einsum("bij,bj->bi", M, v)


def batchwise(M, B):
    M = np.asarray(M, dtype=np.float64)
    return np.broadcast_to(M, (B,) + M.shape) if M.ndim == 2 else M


def split_gain(L, nx):
    """[.., nx + ndu, ny] -> Lx [.., nx, ny], Ld [.., ndu, ny]"""
    L = np.asarray(L, dtype=np.float64)
    return L[..., :nx, :], L[..., nx:, :]


def measure(Cm, Dd, x, delta, v=None):
    y = mv(Cm, x) + mv(Dd, delta)
    return y if v is None else y + v


def measure_bound(Cm, Dd, x, delta, v=None):
    """|y_k - numpy|: nx + ndu products and the add of v_k"""
    nx, ndu = Cm.shape[2], Dd.shape[2]
    mag = mv(np.abs(Cm), np.abs(x)) + mv(np.abs(Dd), np.abs(delta)) + (0.0 if v is None else np.abs(v))
    return (nx + ndu + 1 + 2) * EPS * mag


def plant(Ap, Bp, Bdp, x, u, delta, w=None):
    x1 = mv(Ap, x) + mv(Bp, u) + mv(Bdp, delta)
    return x1 if w is None else x1 + w


def plant_bound(Ap, Bp, Bdp, x, u, delta, w=None):
    """|x_k+1 - numpy|: nx + nu + ndu products (the add of w_k is within the + 2)"""
    n = Ap.shape[2] + Bp.shape[2] + Bdp.shape[2]
    mag = mv(np.abs(Ap), np.abs(x)) + mv(np.abs(Bp), np.abs(u)) + mv(np.abs(Bdp), np.abs(delta)) + (0.0 if w is None else np.abs(w))
    return (n + 2) * EPS * mag


def innovation(Cm, Dd, xh, dh, y):
    return y - (mv(Cm, xh) + mv(Dd, dh))


def innovation_gap(Cm, Dd, xh, dh, e):
    """how far the kernel's innovation and numpy's, both from the logged y, can be apart: yhat is a chain of nx + ndu fused multiply-adds
    there, two products and an add here, (nx + ndu + 2) 2^-52 (|C||xhat| + |Dd||dhat|) between them; each subtraction from y adds
    2^-53 |e|.  Twice the first term is allowed, as tests/test_lmpc_observer_gpu.py does."""
    nx, ndu = Cm.shape[2], Dd.shape[2]
    dyh = (nx + ndu + 2) * EPS * (mv(np.abs(Cm), np.abs(xh)) + mv(np.abs(Dd), np.abs(dh)))
    return 2 * dyh + EPS * np.abs(e)


def estimate(A, Bm, Bd, Lx, xh, u, dh, e):
    return mv(A, xh) + mv(Bm, u) + mv(Bd, dh) + mv(Lx, e)


def estimate_bound(A, Bm, Bd, Cm, Dd, Lx, xh, u, dh, e):
    """|xhat_k+1 - numpy|, numpy's e from the logged y: nx + nu + ndu + ny products, and |Lx| times the gap of the two innovations"""
    n = A.shape[2] + Bm.shape[2] + Bd.shape[2] + Lx.shape[2]
    mag = mv(np.abs(A), np.abs(xh)) + mv(np.abs(Bm), np.abs(u)) + mv(np.abs(Bd), np.abs(dh)) + mv(np.abs(Lx), np.abs(e))
    return (n + 2) * EPS * mag + mv(np.abs(Lx), innovation_gap(Cm, Dd, xh, dh, e))


def disturbance(Ld, dh, e):
    return dh + mv(Ld, e)


def disturbance_bound(Cm, Dd, Ld, xh, dh, e):
    """|dhat_k+1 - numpy|: ny products summed from 0 and one add of dhat_k (ny + 1 terms), and |Ld| times the gap of the two innovations"""
    ny = Ld.shape[2]
    mag = mv(np.abs(Ld), np.abs(e)) + np.abs(dh)
    return (ny + 1 + 2) * EPS * mag + mv(np.abs(Ld), innovation_gap(Cm, Dd, xh, dh, e))


def tick(plant_mats, model, L, x, xh, dh, u, delta, v=None, w=None):
    """one tick of the five equations: (y, e, x_k+1, xhat_k+1, dhat_k+1).  plant_mats (A_p, B_p, Bd_p), model (A, B, Bd, C, Dd), L [.., nx+ndu, ny]"""
    B = x.shape[0]
    Ap, Bp, Bdp = (batchwise(M, B) for M in plant_mats)
    A, Bm, Bd, Cm, Dd = (batchwise(M, B) for M in model)
    Lx, Ld = (batchwise(M, B) for M in split_gain(L, x.shape[1]))
    y = measure(Cm, Dd, x, delta, v)
    e = innovation(Cm, Dd, xh, dh, y)
    return y, e, plant(Ap, Bp, Bdp, x, u, delta, w), estimate(A, Bm, Bd, Lx, xh, u, dh, e), disturbance(Ld, dh, e)


def host_loop(solve, plant_mats, model, L, x0, u0, ticks, xhat0=None, dhat0=None, delta=None, v=None, w=None):
    """A closed loop on the host: cmd_k = solve(xhat_k, u_{k-1}, dhat_k) ([B, nu]), then `tick`.  L [.., nx+ndu, ny] is an offset-free loop's
    gain; L [.., nx, ny] is a plain state observer's: dhat then stays at dhat0 (zeros), the loops of mpcx_lmpc_loop_create_observed with
    nothing measured.  delta [B, ndu] or [ticks, B, ndu] (None: zeros), v [ticks, B, ny], w [ticks, B, nx].  Returns x, xhat, dhat
    ([ticks+1, B, .]), u and y ([ticks, B, .])."""
    x = np.array(x0, dtype=np.float64); u = np.array(u0, dtype=np.float64)
    B, nx = x.shape
    ndu = np.shape(model[2])[-1]
    xh = x.copy() if xhat0 is None else np.array(xhat0, dtype=np.float64)
    dh = np.zeros((B, ndu)) if dhat0 is None else np.array(dhat0, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    if L.shape[-2] == nx:            # a state observer: no disturbance rows
        L = np.concatenate([L, np.zeros(L.shape[:-2] + (ndu, L.shape[-1]))], axis=-2)
    X, XH, DH, U, Y = [x], [xh], [dh], [], []
    for k in range(ticks):
        dk = np.zeros((B, ndu)) if delta is None else (delta if np.ndim(delta) == 2 else delta[k])
        u = np.asarray(solve(xh, u, dh), dtype=np.float64)
        y, _, x, xh, dh = tick(plant_mats, model, L, x, xh, dh, u, dk, None if v is None else v[k], None if w is None else w[k])
        X.append(x); XH.append(xh); DH.append(dh); U.append(u); Y.append(y)
    return tuple(np.stack(a) for a in (X, XH, DH, U, Y))
