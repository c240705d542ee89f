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
