"""Differentiable MPC: the first move of a batch of LMPC solves as a torch.autograd.Function.

    cmd = lmpc_cmd(controller, x0, u0, yref)        # forward: LMPC.optimizeBatch
    loss(cmd).backward()                            # backward: one vector-Jacobian launch (LMPC.sensitivityBatch)

The gradient is that of the solution on the active set the solve ended with: exact wherever the active set does not change
under an infinitesimal perturbation, NaN for an instance that was not solved or whose working set is linearly dependent (the flags of
mpcx_lmpc_sensitivity_batch).  yref is a per-instance constant reference [B, ny]; a per-step reference can be passed but not differentiated.
Torch is imported on first use, as elsewhere in the package."""
from __future__ import annotations

_FUNCTION = None


def _function():
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch

    class LmpcCmd(torch.autograd.Function):
        @staticmethod
        def forward(ctx, controller, x0, u0, yref):
            res = controller.optimizeBatch(x0.detach(), u0.detach(), None if yref is None else yref.detach(), want_active=True)
            ctx.controller = controller
            ctx.has_yref = yref is not None
            ctx.save_for_backward(res.active_lower, res.active_upper, res.status)
            ctx.mark_non_differentiable(res.status)
            return res.cmd, res.status

        @staticmethod
        def backward(ctx, grad_cmd, _grad_status):
            al, au, status = ctx.saved_tensors
            want = tuple(n for n, need in zip(("x0", "u0", "yref"), ctx.needs_input_grad[1:]) if need)
            s = ctx.controller.sensitivityBatch(al, au, status=status, seed_cmd=grad_cmd.contiguous(), want=want)
            return None, s.d_x0, s.d_u0, (s.d_yref if ctx.has_yref else None)

    _FUNCTION = LmpcCmd
    return _FUNCTION


def lmpc_cmd(controller, x0, u0, yref=None, return_status=False):
    """cmd [B, nu] of `controller` (a libmpc_amd.LMPC) at x0 [B, nx], u0 [B, nu] and the per-instance output reference yref [B, ny] (None:
    the controller's own), differentiable with respect to the three.  return_status: (cmd, status) instead."""
    import torch
    _, dev = controller._torch()
    as_t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)).to(device=dev, dtype=torch.float64)
    x0, u0, yref = as_t(x0), as_t(u0), as_t(yref)
    if yref is not None and yref.dim() != 2 and yref.requires_grad:
        raise ValueError("lmpc_cmd differentiates a per-instance output reference [B, ny]; a per-step reference has no gradient here")
    cmd, status = _function().apply(controller, x0, u0, yref)
    return (cmd, status) if return_status else cmd
