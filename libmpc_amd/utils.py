"""Set-up utilities of libmpc++ on the device (reference include/mpc/Utils.hpp)."""
import ctypes as C

from . import _capi
from ._capi import check


def discretization(A, B, Ts, device=0, stream=None):
    """mpc::discretization (Utils.hpp:23-47) for a batch: A [Bn, nx, nx], B [Bn, nx, nu] (row-major tensors as usual in
    torch), Ts one value for the batch (a float, a 0-d or 1-element tensor or array) or Bn values (a tensor, a numpy array or a
    list); any other length is a ValueError.  Returns (Ad, Bd) on the device.  A disturbance matrix Be (Utils.hpp:63-89) is
    discretised by concatenating it to B's columns."""
    import torch
    dev = torch.device("cuda", device)
    A = torch.as_tensor(A, dtype=torch.float64).to(dev); B = torch.as_tensor(B, dtype=torch.float64).to(dev)
    if A.dim() == 2:
        A, B = A[None], B[None]
    if A.dim() != 3 or B.dim() != 3 or A.shape[1] != A.shape[2] or B.shape[:2] != A.shape[:2]:
        raise ValueError(f"A {tuple(A.shape)} and B {tuple(B.shape)} are not [Bn, nx, nx] and [Bn, nx, nu]")
    n, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    ts = torch.as_tensor(Ts, dtype=torch.float64).reshape(-1).to(dev).contiguous()
    if ts.numel() != 1 and ts.numel() != n:          # (the kernel reads Ts[b] of every instance b: a shorter one is read past its end)
        raise ValueError(f"Ts has {ts.numel()} values: one for the batch or one per instance ({n}) expected")
    per = ts.numel() > 1
    # the C ABI takes Eigen's column-major layout: transpose the last two axes
    Ac = A.transpose(1, 2).contiguous(); Bc = B.transpose(1, 2).contiguous()
    Ad = torch.empty_like(Ac); Bd = torch.empty_like(Bc)
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    check(_capi.lib().mpcx_discretize_batch(device, nx, nu, n, Ac.data_ptr(), Bc.data_ptr(), ts.data_ptr(), int(per),
                                            Ad.data_ptr(), Bd.data_ptr(), s))
    return Ad.transpose(1, 2), Bd.transpose(1, 2)


def _as_f64(a):
    import numpy as np
    import torch
    return a.to(torch.float64) if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))      # (a copy: arrays may be read-only)


def dare(A, B, Q, R, form="control", device=0, stream=None, want_iterations=False):
    """A batch of discrete algebraic Riccati equations on the device (mpcx_dare_batch, no reference counterpart), row-major tensors or
    arrays: A [Bn, n, n]; form "control": B [Bn, n, m], X = A'XA - A'XB (R + B'XB)^-1 B'XA + Q and the gain K = (R + B'XB)^-1 B'XA
    [Bn, m, n]; form "estimator": B is the output matrix C [Bn, m, n], P = APA' - APC' (CPC' + R)^-1 CPA' + Q and the predictor gain
    L = APC' (CPC' + R)^-1 [Bn, n, m].  Q [n, n] and R [m, m] for the batch, or [Bn, ., .] per instance.  2-D A and B are a batch of one.
    1 <= n, m <= 32.  Returns (gain, X, flags) on the device (and the doublings taken, with want_iterations); flags [Bn] int32: 0
    converged, 1 R not positive definite, 2 no convergence, 3 a non-finite value or a failed factorisation on the way -- X and the gain
    of such an instance are NaN.  Shape errors are a ValueError before any device call."""
    import torch
    if form not in ("control", "estimator"):
        raise ValueError(f"form is 'control' or 'estimator', got {form!r}")
    est = form == "estimator"
    A, B, Q, R = _as_f64(A), _as_f64(B), _as_f64(Q), _as_f64(R)
    if A.dim() == 2 and B.dim() == 2:
        A, B = A[None], B[None]
    second = "C" if est else "B"
    if A.dim() != 3 or B.dim() != 3 or A.shape[1] != A.shape[2] or B.shape[0] != A.shape[0] or B.shape[2 if est else 1] != A.shape[1]:
        want = "[Bn, m, n]" if est else "[Bn, n, m]"
        raise ValueError(f"A {tuple(A.shape)} and {second} {tuple(B.shape)} are not [Bn, n, n] and {want}")
    bn, n, m = A.shape[0], A.shape[1], B.shape[1 if est else 2]
    if not (1 <= n <= 32 and 1 <= m <= 32):
        raise ValueError(f"n = {n}, m = {m}: 1 <= n <= 32 and 1 <= m <= 32 expected")
    for name, M, k in (("Q", Q, n), ("R", R, m)):
        if tuple(M.shape) not in ((k, k), (bn, k, k)):
            raise ValueError(f"{name} {tuple(M.shape)} is neither [{k}, {k}] nor [{bn}, {k}, {k}]")
    dev = torch.device("cuda", device)
    # the C ABI takes Eigen's column-major layout: transpose the last two axes
    Ac, Bc, Qc, Rc = (M.to(dev).transpose(-1, -2).contiguous() for M in (A, B, Q, R))
    X = torch.empty((bn, n, n), dtype=torch.float64, device=dev)
    G = torch.empty((bn, n, m) if not est else (bn, m, n), dtype=torch.float64, device=dev)       # column-major [m x n] / [n x m]
    flags = torch.empty(bn, dtype=torch.int32, device=dev)
    its = torch.empty(bn, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    check(_capi.lib().mpcx_dare_batch(device, _capi.DARE_ESTIMATOR if est else _capi.DARE_CONTROL, n, m, bn, Ac.data_ptr(), Bc.data_ptr(),
                                      Qc.data_ptr(), Rc.data_ptr(), int(Q.dim() == 3), int(R.dim() == 3), X.data_ptr(), G.data_ptr(),
                                      flags.data_ptr(), its.data_ptr(), s))
    out = (G.transpose(1, 2), X.transpose(1, 2), flags)
    return out + (its,) if want_iterations else out


def kalman_gains(A, C, Qw, Rv, device=0, stream=None):
    """Steady-state Kalman predictor gains for a batch: (L [Bn, n, m], P [Bn, n, n], flags) of dare(A, C, Qw, Rv, "estimator").  L is a
    view of the layout mpcx_lmpc_observer_desc.gain_batch takes: an observed loop's observer= accepts it as it is."""
    return dare(A, C, Qw, Rv, "estimator", device, stream)


def lqr_gains(A, B, Q, R, device=0, stream=None):
    """Infinite-horizon LQR for a batch: (K [Bn, m, n] with u = -K x, X [Bn, n, n] the cost-to-go -- a terminal weight --, flags) of
    dare(A, B, Q, R, "control")."""
    return dare(A, B, Q, R, "control", device, stream)


def disturbance_gains(A, Bd, C, Dd, Qw, Qd, Rv, device=0, stream=None):
    """Steady-state Kalman predictor gains of models augmented with an integrating disturbance, for offset-free loops
    (disturbance_observer=): per instance Aa = [[A, Bd], [0, I]], Ca = [C, Dd], Q = blkdiag(Qw, Qd), and (L [Bn, nx+ndu, ny] -- rows
    0 .. nx-1 are Lx, the others Ld --, P [Bn, nx+ndu, nx+ndu], flags) of dare(Aa, Ca, Q, Rv, "estimator").  A [Bn, nx, nx], Bd
    [Bn, nx, ndu], C [Bn, ny, nx], Dd [Bn, ny, ndu] (2-D: a batch of one); Qw, Qd, Rv one for the batch or one per instance.  L is a view
    of the layout mpcx_lmpc_disturbance_observer_desc.gain_batch takes.  ValueError before any device call: shapes, nx + ndu > 32, and an
    augmented pair that is not detectable -- rank [[I - A, -Bd], [C, Dd]] = nx + ndu is required, which needs ndu <= ny."""
    import numpy as np
    import torch
    A, Bd, C, Dd, Qw, Qd = (_as_f64(M) for M in (A, Bd, C, Dd, Qw, Qd))
    if A.dim() == 2:
        A, Bd, C, Dd = (M[None] if M.dim() == 2 else M for M in (A, Bd, C, Dd))
    if A.dim() != 3 or A.shape[1] != A.shape[2] or Bd.dim() != 3 or C.dim() != 3 or Dd.dim() != 3:
        raise ValueError(f"A {tuple(A.shape)} is not [Bn, nx, nx] with 3-D Bd, C and Dd beside it")
    bn, nx, ndu, ny = A.shape[0], A.shape[1], Bd.shape[2], C.shape[1]
    for name, M, sh in (("Bd", Bd, (bn, nx, ndu)), ("C", C, (bn, ny, nx)), ("Dd", Dd, (bn, ny, ndu))):
        if tuple(M.shape) != sh:
            raise ValueError(f"{name} {tuple(M.shape)} is not {list(sh)}")
    for name, M, k in (("Qw", Qw, nx), ("Qd", Qd, ndu)):
        if tuple(M.shape) not in ((k, k), (bn, k, k)):
            raise ValueError(f"{name} {tuple(M.shape)} is neither [{k}, {k}] nor [{bn}, {k}, {k}]")
    n = nx + ndu
    if ndu < 1:
        raise ValueError("ndu = 0: there is no disturbance model to estimate")
    if not (1 <= n <= 32 and 1 <= ny <= 32):
        raise ValueError(f"n = {n}, m = {ny}: 1 <= n <= 32 and 1 <= m <= 32 expected")
    Aa = torch.zeros((bn, n, n), dtype=torch.float64)
    Aa[:, :nx, :nx] = A; Aa[:, :nx, nx:] = Bd; Aa[:, nx:, nx:] = torch.eye(ndu, dtype=torch.float64)
    Ca = torch.cat([C, Dd], dim=2)
    # detectability of the integrators: the augmented pair has them observable exactly where this matrix has full column rank
    M = np.concatenate([np.concatenate([np.eye(nx) - A.numpy(), -Bd.numpy()], axis=2), Ca.numpy()], axis=1)
    sv = np.linalg.svd(M, compute_uv=False)                    # [bn, min(nx + ny, n)], descending
    rank = (sv > sv[:, :1] * max(M.shape[1:]) * np.finfo(np.float64).eps).sum(axis=1)
    if (rank < n).any():
        k = int(np.argmax(rank < n))
        raise ValueError(f"instance {k}: rank [[I - A, -Bd], [C, Dd]] = {int(rank[k])} < nx + ndu = {n}: the augmented pair ([[A, Bd], [0, I]], "
                         f"[C, Dd]) is not detectable (ndu <= ny is necessary; so is a disturbance model that reaches the outputs)")
    per = Qw.dim() == 3 or Qd.dim() == 3
    Q = torch.zeros((bn, n, n) if per else (n, n), dtype=torch.float64)
    Q[..., :nx, :nx] = Qw; Q[..., nx:, nx:] = Qd
    return dare(Aa, Ca, Q, Rv, "estimator", device, stream)


def target_maps(A, B, Bd, C, Dd, want_x=False, device=0, stream=None, check_rank=True):
    """Steady-state target maps for a batch of models on the device (mpcx_target_map_batch, no reference counterpart), row-major tensors or
    arrays: A [Bn, nx, nx], B [Bn, nx, nu], Bd [Bn, nx, ndu], C [Bn, ny, nx], Dd [Bn, ny, ndu] (2-D: a batch of one).  The target of a
    reference r, a disturbance estimate dhat and an input reference ubar is
        minimise 1/2 |us - ubar|^2   subject to   (I - A) xs - B us = Bd dhat,   C xs = r - Dd dhat
    and us = map_u [r; dhat; ubar], xs = map_x [r; dhat; ubar].  Returns (map_u [Bn, nu, ny+ndu+nu], flags) or, with want_x, (map_u, map_x
    [Bn, nx, ny+ndu+nu], flags) on the device; flags [Bn] int32: 0 fine, 1 singular -- the maps of such an instance are NaN.  map_u is a view
    of the layout mpcx_lmpc_target_desc.map_batch takes: a loop's target= accepts it as it is.  ValueError before any device call: shapes, and
    (check_rank) an instance that misses one of the two rank conditions -- rank [[I - A, -B], [C, 0]] = nx + ny (every reference can be reached;
    needs ny <= nu) and rank [I - A; C] = nx (no integrator that the outputs do not see)."""
    import numpy as np
    import torch
    A, B, Bd, C, Dd = (_as_f64(M) for M in (A, B, Bd, C, Dd))
    if A.dim() == 2:
        A, B, Bd, C, Dd = (M[None] if M.dim() == 2 else M for M in (A, B, Bd, C, Dd))
    if A.dim() != 3 or A.shape[1] != A.shape[2] or B.dim() != 3 or Bd.dim() != 3 or C.dim() != 3 or Dd.dim() != 3:
        raise ValueError(f"A {tuple(A.shape)} is not [Bn, nx, nx] with 3-D B, Bd, C and Dd beside it")
    bn, nx, nu, ndu, ny = A.shape[0], A.shape[1], B.shape[2], Bd.shape[2], C.shape[1]
    for name, M, sh in (("B", B, (bn, nx, nu)), ("Bd", Bd, (bn, nx, ndu)), ("C", C, (bn, ny, nx)), ("Dd", Dd, (bn, ny, ndu))):
        if tuple(M.shape) != sh:
            raise ValueError(f"{name} {tuple(M.shape)} is not {list(sh)}")
    if nx < 1 or nu < 1 or ny < 1:
        raise ValueError(f"nx = {nx}, nu = {nu}, ny = {ny}: at least one state, one input and one output expected")
    if check_rank and bn:
        An, Bn, Cn = (M.cpu().numpy() for M in (A, B, C))
        IA = np.eye(nx) - An

        def rank(M):
            sv = np.linalg.svd(M, compute_uv=False)            # descending
            return (sv > sv[:, :1] * max(M.shape[1:]) * np.finfo(np.float64).eps).sum(axis=1)
        rs = rank(np.concatenate([np.concatenate([IA, -Bn], axis=2), np.concatenate([Cn, np.zeros((bn, ny, nu))], axis=2)], axis=1))
        if (rs < nx + ny).any():
            k = int(np.argmax(rs < nx + ny))
            raise ValueError(f"instance {k}: rank [[I - A, -B], [C, 0]] = {int(rs[k])} < nx + ny = {nx + ny}: not every reference can be reached "
                             f"in steady state (ny <= nu is necessary)")
        ro = rank(np.concatenate([IA, Cn], axis=1))
        if (ro < nx).any():
            k = int(np.argmax(ro < nx))
            raise ValueError(f"instance {k}: rank [I - A; C] = {int(ro[k])} < nx = {nx}: the model has an integrator that the outputs do not see")
    dev = torch.device("cuda", device)
    # the C ABI takes Eigen's column-major layout: transpose the last two axes
    Ac, Bc, Bdc, Cc, Ddc = (M.to(dev).transpose(-1, -2).contiguous() for M in (A, B, Bd, C, Dd))
    nrhs = ny + ndu + nu
    Tu = torch.empty((bn, nrhs, nu), dtype=torch.float64, device=dev)          # column-major [nu x nrhs]
    Tx = torch.empty((bn, nrhs, nx), dtype=torch.float64, device=dev) if want_x else None
    flags = torch.empty(bn, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    check(_capi.lib().mpcx_target_map_batch(device, nx, nu, ndu, ny, bn, Ac.data_ptr(), Bc.data_ptr(), Bdc.data_ptr(), Cc.data_ptr(), Ddc.data_ptr(),
                                            Tu.data_ptr(), Tx.data_ptr() if want_x else None, flags.data_ptr(), s))
    return (Tu.transpose(1, 2), Tx.transpose(1, 2), flags) if want_x else (Tu.transpose(1, 2), flags)


def steady_state_inputs(map_u, r, dhat, ubar, device=0, stream=None):
    """us [Bn, nu] = map_u [r; dhat; ubar] on the device (mpcx_target_apply_batch), for host-driven loops: the sum the closed loop's kernels
    form, bit for bit -- every row from 0 with fused multiply-adds by ascending column.  map_u [nu, ny+ndu+nu] for the batch or
    [Bn, nu, ny+ndu+nu] per instance (target_maps' as it is), r [Bn, ny], dhat [Bn, ndu], ubar [Bn, nu]."""
    import torch
    T, r, dhat, ubar = (_as_f64(M) for M in (map_u, r, dhat, ubar))
    if r.dim() != 2 or dhat.dim() != 2 or ubar.dim() != 2 or dhat.shape[0] != r.shape[0] or ubar.shape[0] != r.shape[0]:
        raise ValueError(f"r {tuple(r.shape)}, dhat {tuple(dhat.shape)} and ubar {tuple(ubar.shape)} are not [Bn, ny], [Bn, ndu] and [Bn, nu]")
    bn, ny, ndu, nu = r.shape[0], r.shape[1], dhat.shape[1], ubar.shape[1]
    nrhs = ny + ndu + nu
    if tuple(T.shape) not in ((nu, nrhs), (bn, nu, nrhs)):
        raise ValueError(f"map_u {tuple(T.shape)} is neither [{nu}, {nrhs}] nor [{bn}, {nu}, {nrhs}]")
    if nu < 1 or ny < 1:
        raise ValueError(f"nu = {nu}, ny = {ny}: at least one input and one output expected")
    dev = torch.device("cuda", device)
    Tc = T.to(dev).transpose(-1, -2).contiguous()
    rc, dc, uc = (M.to(dev).contiguous() for M in (r, dhat, ubar))
    us = torch.empty((bn, nu), dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    check(_capi.lib().mpcx_target_apply_batch(device, nu, ndu, ny, bn, Tc.data_ptr(), int(T.dim() == 3), rc.data_ptr(), dc.data_ptr(), uc.data_ptr(),
                                              us.data_ptr(), s))
    return us
