"""Differentiable MPC: the first move of a batch of LMPC solves as a torch.autograd.Function.

    cmd = lmpc_cmd(controller, x0, u0, yref)        # forward: LMPC.optimizeBatch
    loss(cmd).backward()                            # backward: one vector-Jacobian launch (LMPC.sensitivityBatch)

The gradient is that of the solution on the active set the solve ended with: exact wherever the active set does not change
under an infinitesimal perturbation, NaN for an instance that was not solved or whose working set is linearly dependent (the flags of
mpcx_lmpc_sensitivity_batch).  yref is a per-instance constant reference [B, ny]; a per-step reference can be passed but not differentiated.
Torch is imported on first use, as elsewhere in the package.

    cmd = lmpc_cmd_params(controller, x0, u0, yref, OWeight, UWeight, DeltaUWeight)

is the same first move, differentiable with respect to the three weight matrices of setObjectiveWeights as well: what a tuning loop needs that
descends on a closed-loop or imitation loss over many instances.  Forward sets the weights, sets the controller up and solves; backward is
one launch of the vector-Jacobian product above and one of LMPC.paramSensitivityBatch with reduce=True -- the weights are
shared by the batch, so their gradient is the sum over the instances, added in a fixed order; an instance that was not solved or whose working
set is dependent contributes nothing to it.  Gradients with respect to the bounds are not part of this function: paramSensitivityBatch returns
them, in the row numbering of the active sets.  The backward pass differentiates the batch the controller solved last, under the set-up of that solve:
call backward before the controller is changed, set up again or given another forward pass of this function (mpcx_lmpc_param_sensitivity_batch
answers MPCX_E_STATE after a change or a new set-up); keep one controller per graph that is kept.

    cmd = lmpc_cmd_model(controller, x0, u0, yref, A, B, C, Bd=None, Dd=None)

differentiates the same first move with respect to the model: what fitting A, B, C of a fleet's controller to logged or expert closed-loop
behaviour needs.  Forward sets the model (and the disturbance matrices, where given), sets the controller up and solves; backward is one launch of
the vector-Jacobian product and one of LMPC.modelSensitivityBatch with reduce=True.  The controller keeps every other setting;
the rules of lmpc_cmd_params hold.

    cmd = lmpc_cmd_fleet(controllers, x0, u0, yref, model, OWeight=..., A=..., ...)

is the fleet's version of the three: K controllers, instance b solved by controller model[b], every parameter tensor with K in front.  Forward
sets the given tensors on every controller, builds a fresh bank (LMPCHetero) from them and solves; backward is one vector-Jacobian launch
 and one of LMPCHetero.gradientBatch with per_controller=True, whose per-controller rows are the gradients
of the K-leading tensors.

    traj_x, traj_u = lmpc_closed_loop(controller, x0, u0, ticks, yref=..., plant=..., noise=..., OWeight=..., A=..., ...)

is the closed loop itself: `ticks` receding-horizon steps on the device (LMPC.make_loop / run_loop), differentiable with respect to every tensor
argument.  Forward applies the given weights and model under the rules of lmpc_cmd_params / lmpc_cmd_model, builds the loop and runs it; backward
is one LMPC.run_loop_gradient -- `ticks` graph replays of "re-solve, vector-Jacobian launches, adjoint kernel", no autograd node
per tick and nothing taped beyond the two trajectories.  What a loss on a closed-loop trajectory needs: tuning weights against a tracking cost,
fitting the controller's model or identifying the plant from logged runs, the sensitivity of a closed-loop cost to the initial state or the
process noise."""
from __future__ import annotations

_FUNCTION = None


def _function():
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch

    class LmpcCmd(torch.autograd.Function):
        @staticmethod
        def forward(ctx, controller, x0, u0, yref, bank_model=None):
            # a bank (LMPCHetero) takes the instance -> controller map in the solve and in the backward launch; a controller has none
            kw = {} if bank_model is None else {"model": bank_model[0]}
            res = controller.optimizeBatch(x0.detach(), u0.detach(), yref=None if yref is None else yref.detach(), want_active=True, **kw)
            ctx.controller, ctx.kw = controller, kw
            ctx.has_yref = yref is not None
            ctx.save_for_backward(res.active_lower, res.active_upper, res.status)
            ctx.mark_non_differentiable(res.status)
            return res.cmd, res.status

        @staticmethod
        def backward(ctx, grad_cmd, _grad_status):
            al, au, status = ctx.saved_tensors
            want = tuple(n for n, need in zip(("x0", "u0", "yref"), ctx.needs_input_grad[1:4]) if need)
            s = ctx.controller.sensitivityBatch(al, au, status=status, seed_cmd=grad_cmd.contiguous(), want=want, **ctx.kw)
            return None, s.d_x0, s.d_u0, (s.d_yref if ctx.has_yref else None), None

    _FUNCTION = LmpcCmd
    return _FUNCTION


_PARAM_FUNCTION = None


def _param_function():
    global _PARAM_FUNCTION
    if _PARAM_FUNCTION is not None:
        return _PARAM_FUNCTION
    import torch

    class LmpcCmdParams(torch.autograd.Function):
        @staticmethod
        def forward(ctx, controller, x0, u0, yref, ow, uw, dw):
            if not controller.setObjectiveWeights(ow.detach().cpu().numpy(), uw.detach().cpu().numpy(), dw.detach().cpu().numpy()):
                raise ValueError("lmpc_cmd_params: the controller refused the weights")
            controller.setup()
            res = controller.optimizeBatch(x0.detach(), u0.detach(), None if yref is None else yref.detach(), want_active=True, want_sequence=True)
            ctx.controller, ctx.res = controller, res
            ctx.has_yref = yref is not None
            ctx.mark_non_differentiable(res.status)
            return res.cmd, res.status

        @staticmethod
        def backward(ctx, grad_cmd, _grad_status):
            c, res = ctx.controller, ctx.res
            seed = grad_cmd.contiguous()
            need = ctx.needs_input_grad
            g = [None] * 7
            want = tuple(n for n, k in zip(("x0", "u0", "yref"), need[1:4]) if k)
            if want:
                s = c.sensitivityBatch(res.active_lower, res.active_upper, status=res.status, seed_cmd=seed, want=want)
                g[1], g[2], g[3] = s.d_x0, s.d_u0, (s.d_yref if ctx.has_yref else None)
            wantp = tuple(n for n, k in zip(("oweight", "uweight", "duweight"), need[4:7]) if k)
            if wantp:
                p = c.paramSensitivityBatch(res, seed_cmd=seed, reduce=True, want=wantp)
                g[4], g[5], g[6] = p.d_oweight, p.d_uweight, p.d_duweight
            return tuple(g)

    _PARAM_FUNCTION = LmpcCmdParams
    return _PARAM_FUNCTION


def lmpc_cmd_params(controller, x0, u0, yref, OWeight, UWeight, DeltaUWeight, return_status=False):
    """cmd [B, nu] of `controller` (a libmpc_amd.LMPC) with the objective weights OWeight [ny, ph], UWeight [nu, ph], DeltaUWeight [nu, ph] (the
    matrices of setObjectiveWeights, torch tensors on any device) at x0 [B, nx], u0 [B, nu] and the per-instance output reference yref [B, ny]
    (None: the controller's own), differentiable with respect to all six.  The controller keeps the weights afterwards.  The gradients of the
    weights are sums over the batch; those of the bounds come from LMPC.paramSensitivityBatch.  return_status: (cmd, status) instead."""
    import torch
    _, dev = controller._torch()
    as_t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)).to(device=dev, dtype=torch.float64)
    x0, u0, yref = as_t(x0), as_t(u0), as_t(yref)
    if yref is not None and yref.dim() != 2 and yref.requires_grad:
        raise ValueError("lmpc_cmd_params differentiates a per-instance output reference [B, ny]; a per-step reference has no gradient here")
    cmd, status = _param_function().apply(controller, x0, u0, yref, as_t(OWeight), as_t(UWeight), as_t(DeltaUWeight))
    return (cmd, status) if return_status else cmd


_MODEL_FUNCTION = None


def _model_function():
    global _MODEL_FUNCTION
    if _MODEL_FUNCTION is not None:
        return _MODEL_FUNCTION
    import torch

    class LmpcCmdModel(torch.autograd.Function):
        @staticmethod
        def forward(ctx, controller, x0, u0, yref, A, B, Cm, Bd, Dd):
            host = lambda t: t.detach().cpu().numpy()
            if not controller.setStateSpaceModel(host(A), host(B), host(Cm)):
                raise ValueError("lmpc_cmd_model: the controller refused the model")
            if Bd is not None and not controller.setDisturbances(host(Bd), host(Dd)):
                raise ValueError("lmpc_cmd_model: the controller refused the disturbance matrices")
            controller.setup()
            res = controller.optimizeBatch(x0.detach(), u0.detach(), None if yref is None else yref.detach(), want_active=True, want_sequence=True)
            ctx.controller, ctx.res = controller, res
            ctx.has_yref = yref is not None
            ctx.mark_non_differentiable(res.status)
            return res.cmd, res.status

        @staticmethod
        def backward(ctx, grad_cmd, _grad_status):
            c, res = ctx.controller, ctx.res
            seed = grad_cmd.contiguous()
            need = ctx.needs_input_grad
            g = [None] * 9
            want = tuple(n for n, k in zip(("x0", "u0", "yref"), need[1:4]) if k)
            if want:
                s = c.sensitivityBatch(res.active_lower, res.active_upper, status=res.status, seed_cmd=seed, want=want)
                g[1], g[2], g[3] = s.d_x0, s.d_u0, (s.d_yref if ctx.has_yref else None)
            wantm = tuple(n for n, k in zip(("A", "B", "C", "Bd", "Dd"), need[4:9]) if k)
            if wantm:
                m = c.modelSensitivityBatch(res, seed_cmd=seed, reduce=True, want=wantm)
                g[4], g[5], g[6], g[7], g[8] = m.d_A, m.d_B, m.d_C, m.d_Bd, m.d_Dd
            return tuple(g)

    _MODEL_FUNCTION = LmpcCmdModel
    return _MODEL_FUNCTION


def lmpc_cmd_model(controller, x0, u0, yref, A, B, C, Bd=None, Dd=None, return_status=False):
    """cmd [B, nu] of `controller` (a libmpc_amd.LMPC) with the model A [nx, nx], B [nx, nu], C [ny, nx] and, where given, the disturbance
    matrices Bd [nx, ndu], Dd [ny, ndu] (the matrices of setStateSpaceModel / setDisturbances, torch tensors on any device) at x0 [B, nx],
    u0 [B, nu] and the per-instance output reference yref [B, ny] (None: the controller's own), differentiable with respect to all of them.  The
    controller keeps the model afterwards, and every other setting.  The gradients of the model are sums over the batch.  return_status:
    (cmd, status) instead."""
    import torch
    _, dev = controller._torch()
    as_t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)).to(device=dev, dtype=torch.float64)
    x0, u0, yref = as_t(x0), as_t(u0), as_t(yref)
    if yref is not None and yref.dim() != 2 and yref.requires_grad:
        raise ValueError("lmpc_cmd_model differentiates a per-instance output reference [B, ny]; a per-step reference has no gradient here")
    if (Bd is None) != (Dd is None):
        raise ValueError("lmpc_cmd_model: Bd and Dd go together")
    cmd, status = _model_function().apply(controller, x0, u0, yref, as_t(A), as_t(B), as_t(C), as_t(Bd), as_t(Dd))
    return (cmd, status) if return_status else cmd


_FLEET_FUNCTION = None
_FLEET_PARAMS = ("oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")


def _fleet_function():
    global _FLEET_FUNCTION
    if _FLEET_FUNCTION is not None:
        return _FLEET_FUNCTION
    import torch

    class LmpcCmdFleet(torch.autograd.Function):
        @staticmethod
        def forward(ctx, controllers, bank_model, device, x0, u0, yref, ow, uw, dw, A, B, Cm, Bd, Dd):
            from .bank import LMPCHetero
            host = lambda t, k: t[k].detach().cpu().numpy()
            for k, c in enumerate(controllers):
                if ow is not None and not c.setObjectiveWeights(host(ow, k), host(uw, k), host(dw, k)):
                    raise ValueError("lmpc_cmd_fleet: controller %d refused the weights" % k)
                if A is not None and not c.setStateSpaceModel(host(A, k), host(B, k), host(Cm, k)):
                    raise ValueError("lmpc_cmd_fleet: controller %d refused the model" % k)
                if Bd is not None and not c.setDisturbances(host(Bd, k), host(Dd, k)):
                    raise ValueError("lmpc_cmd_fleet: controller %d refused the disturbance matrices" % k)
            bank = LMPCHetero(controllers, device=device)
            res = bank.optimizeBatch(x0.detach(), u0.detach(), model=bank_model[0], yref=None if yref is None else yref.detach(), want_active=True,
                                     want_sequence=True)
            ctx.bank, ctx.res = bank, res                      # (the bank lives as long as the graph: backward launches on it)
            ctx.has_yref = yref is not None
            ctx.mark_non_differentiable(res.status)
            return res.cmd, res.status

        @staticmethod
        def backward(ctx, grad_cmd, _grad_status):
            bank, res = ctx.bank, ctx.res
            seed = grad_cmd.contiguous()
            need = ctx.needs_input_grad
            g = [None] * 14
            want = tuple(n for n, k in zip(("x0", "u0", "yref"), need[3:6]) if k)
            if want:
                s = bank.sensitivityBatch(res.active_lower, res.active_upper, model=res._model, status=res.status, seed_cmd=seed, want=want)
                g[3], g[4], g[5] = s.d_x0, s.d_u0, (s.d_yref if ctx.has_yref else None)
            wantp = tuple(n for n, k in zip(_FLEET_PARAMS, need[6:14]) if k)
            if wantp:
                r = bank.gradientBatch(res, seed_cmd=seed, per_controller=True, want=wantp)
                ctx.gradient = r                               # (testing aid: what the launch returned)
                for i, n in enumerate(_FLEET_PARAMS):
                    g[6 + i] = getattr(r, "c_" + n) if n in wantp else None
            return tuple(g)

    _FLEET_FUNCTION = LmpcCmdFleet
    return _FLEET_FUNCTION


def lmpc_cmd_fleet(controllers, x0, u0, yref, model=None, OWeight=None, UWeight=None, DeltaUWeight=None, A=None, B=None, C=None, Bd=None, Dd=None,
                   return_status=False, device=0):
    """cmd [B, nu] of a fleet: K configured controllers (libmpc_amd.LMPC; host-only handles are enough) of equal dimensions, instance b solved
    by controller model[b] (None: instance b = controller b, B = K), at x0 [B, nx], u0 [B, nu] and the per-instance output reference yref
    [B, ny] (None: each controller's own).  Each given parameter tensor has K in front -- OWeight [K, ny, ph], UWeight, DeltaUWeight [K, nu, ph]
    (all three or none), A [K, nx, nx], B [K, nx, nu], C [K, ny, nx] (all three or none), Bd [K, nx, ndu], Dd [K, ny, ndu] (both or none) -- and
    is set on every controller, which keeps it afterwards; cmd is differentiable with respect to all of them and to x0, u0, yref.  The gradient
    of row k of a parameter tensor is the sum over controller k's instances in their order in the batch; an instance that was not solved or
    whose working set is dependent contributes nothing to it.  A loss that needs no model gradient never runs the model part of the kernel.
    The rules of lmpc_cmd_params hold; the bank of the forward pass is kept by the graph.  return_status: (cmd, status) instead."""
    import torch
    controllers = list(controllers)
    if not controllers:
        raise ValueError("lmpc_cmd_fleet: at least one controller")
    for group, what in (((OWeight, UWeight, DeltaUWeight), "OWeight, UWeight and DeltaUWeight"), ((A, B, C), "A, B and C"), ((Bd, Dd), "Bd and Dd")):
        if any(t is None for t in group) and not all(t is None for t in group):
            raise ValueError("lmpc_cmd_fleet: %s go together" % what)
    for t in (OWeight, UWeight, DeltaUWeight, A, B, C, Bd, Dd):
        if t is not None and (len(t.shape) != 3 or t.shape[0] != len(controllers)):
            raise ValueError("lmpc_cmd_fleet: every parameter tensor is [K, rows, columns], K the number of controllers")
    dev = torch.device("cuda", int(device))
    as_t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)).to(device=dev, dtype=torch.float64)
    x0, u0, yref = as_t(x0), as_t(u0), as_t(yref)
    if yref is not None and yref.dim() != 2 and yref.requires_grad:
        raise ValueError("lmpc_cmd_fleet differentiates a per-instance output reference [B, ny]; a per-step reference has no gradient here")
    params = [as_t(t) for t in (OWeight, UWeight, DeltaUWeight, A, B, C, Bd, Dd)]
    cmd, status = _fleet_function().apply(controllers, (model,), int(device), x0, u0, yref, *params)
    return (cmd, status) if return_status else cmd


_LOOP_FUNCTION = None
_LOOP_WANT = ("x0", "u0", "yref", "plant", "plant", "plant", "noise", "oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")


class _LoopHolder:
    """the loop of a forward pass and the gradient object of its backward pass: destroyed with the graph that keeps them"""

    def __init__(self, controller, loop):
        self.controller, self.loop, self.gradient = controller, loop, None

    def close(self):
        if self.gradient is not None:
            self.controller.destroy_loop_gradient(self.gradient)
            self.gradient = None
        if self.loop is not None:
            self.controller.destroy_loop(self.loop)
            self.loop = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _loop_function():
    global _LOOP_FUNCTION
    if _LOOP_FUNCTION is not None:
        return _LOOP_FUNCTION
    import torch

    class LmpcClosedLoop(torch.autograd.Function):
        @staticmethod
        def forward(ctx, controller, ticks, loop_kw, x0, u0, yref, pA, pB, pBd, noise, ow, uw, dw, A, B, Cm, Bd, Dd):
            host = lambda t: t.detach().cpu().numpy()
            if ow is not None and not controller.setObjectiveWeights(host(ow), host(uw), host(dw)):
                raise ValueError("lmpc_closed_loop: the controller refused the weights")
            if A is not None and not controller.setStateSpaceModel(host(A), host(B), host(Cm)):
                raise ValueError("lmpc_closed_loop: the controller refused the model")
            if Bd is not None and not controller.setDisturbances(host(Bd), host(Dd)):
                raise ValueError("lmpc_closed_loop: the controller refused the disturbance matrices")
            controller.setup()
            det = lambda t: None if t is None else t.detach()
            per_instance = pA is not None and pA.dim() == 3
            kw = dict(loop_kw)
            if pA is not None:
                triple = (det(pA), det(pB), det(pBd))
                if per_instance:
                    kw["plants"] = triple
                else:
                    kw["plant"] = tuple(None if t is None else host(t) for t in triple)
            loop = controller.make_loop(det(x0), det(u0), ticks, yref=det(yref), noise=det(noise), **kw)
            ctx.holder = _LoopHolder(controller, loop)
            ctx.per_instance = per_instance
            controller.run_loop(loop)
            torch.cuda.current_stream(controller.device).synchronize()
            ctx.status = loop.result.status
            return loop.result.x.clone(), loop.result.u.clone()

        @staticmethod
        def backward(ctx, grad_x, grad_u):
            hold = ctx.holder
            c = hold.controller
            need = ctx.needs_input_grad[3:]
            want = tuple(sorted({n for n, k in zip(_LOOP_WANT, need) if k}))
            reduce = not ctx.per_instance
            seed_x = None if grad_x is None else grad_x.contiguous()
            seed_u = None if grad_u is None else grad_u.contiguous()
            try:
                r = hold.gradient = c.make_loop_gradient(hold.loop, seed_x=seed_x, seed_u=seed_u, reduce=reduce, want=want)
                c.run_loop_gradient(r)
                torch.cuda.current_stream(c.device).synchronize()
            finally:
                hold.close()
            ctx.gradient = r                                   # (testing aid: what the run returned)
            if reduce:
                shared = lambda t: t
            else:                                              # a set per instance: the shared tensors' gradients are sums over the instances with flag 0
                ok = (r.flags == 0)
                shared = lambda t: None if t is None else torch.where(ok.view(-1, 1, 1), t, torch.zeros_like(t)).sum(dim=0)
            outs = (r.d_x0, r.d_u0, r.d_yref, r.d_plant_A, r.d_plant_B, r.d_plant_Bd, r.d_noise,
                    shared(r.d_oweight), shared(r.d_uweight), shared(r.d_duweight), shared(r.d_A), shared(r.d_B), shared(r.d_C), shared(r.d_Bd), shared(r.d_Dd))
            return (None, None, None) + tuple(g if k else None for g, k in zip(outs, need))

    _LOOP_FUNCTION = LmpcClosedLoop
    return _LOOP_FUNCTION


def lmpc_closed_loop(controller, x0, u0, ticks, yref=None, plant=None, noise=None, OWeight=None, UWeight=None, DeltaUWeight=None,
                     A=None, B=None, C=None, Bd=None, Dd=None, **loop_kw):
    """(traj_x [ticks+1, B, nx], traj_u [ticks, B, nu]) of `ticks` closed-loop steps of `controller` (a libmpc_amd.LMPC) from x0 [B, nx] and the
    last input u0 [B, nu], differentiable with respect to every tensor argument: x0, u0, the per-instance output reference yref [B, ny], the
    process noise [ticks, B, nx], the plant, the weights OWeight [ny, ph], UWeight, DeltaUWeight [nu, ph] (all three or none) and the controller's
    model A, B, C (all three or none), Bd, Dd (both or none).  plant = (A_p, B_p) or (A_p, B_p, Bd_p): [nx, .] one plant for the batch, its
    gradient summed over the instances, or [B, nx, .] a plant per instance; None: the controller's own model -- and where A, B (Bd) are given they
    are then the plant as well, so their gradients are the sum of the model's part and the plant's.  The gradients of plant and controller model are
    separate outputs of the backward pass even when one tensor is passed for both; autograd adds them.  The gradients of shared tensors are sums
    over the instances whose flag is 0; an instance that was not solved at some tick has NaN in its per-instance gradients.  loop_kw: further
    arguments of LMPC.make_loop (uref, duref, dmeas, preview, warm), not differentiated.  The controller keeps the weights and the model
    afterwards; call backward before it is changed again (the rules of lmpc_cmd_params)."""
    import torch
    _, dev = controller._torch()
    as_t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)).to(device=dev, dtype=torch.float64)
    for group, what in (((OWeight, UWeight, DeltaUWeight), "OWeight, UWeight and DeltaUWeight"), ((A, B, C), "A, B and C"), ((Bd, Dd), "Bd and Dd")):
        if any(t is None for t in group) and not all(t is None for t in group):
            raise ValueError("lmpc_closed_loop: %s go together" % what)
    for k in ("plant", "plants", "observer", "disturbance_observer", "target", "noise", "yref"):
        if k in loop_kw:
            raise ValueError("lmpc_closed_loop: %s= is not a loop_kw of this function" % k)
    yref = as_t(yref)
    if yref is not None and yref.dim() != 2 and yref.requires_grad:
        raise ValueError("lmpc_closed_loop differentiates a per-instance output reference [B, ny]; a per-step reference has no gradient here")
    if plant is None and A is not None:
        plant = (A, B, Bd)
    pA, pB, pBd = (tuple(plant) + (None,) * 3)[:3] if plant is not None else (None, None, None)
    if plant is not None and (pA is None or pB is None):
        raise ValueError("lmpc_closed_loop: plant is (A_p, B_p) or (A_p, B_p, Bd_p)")
    return _loop_function().apply(controller, int(ticks), loop_kw, as_t(x0), as_t(u0), yref, as_t(pA), as_t(pB), as_t(pBd), as_t(noise),
                                  as_t(OWeight), as_t(UWeight), as_t(DeltaUWeight), as_t(A), as_t(B), as_t(C), as_t(Bd), as_t(Dd))


def lmpc_cmd(controller, x0, u0, yref=None, return_status=False, model=None):
    """cmd [B, nu] of `controller` (a libmpc_amd.LMPC) at x0 [B, nx], u0 [B, nu] and the per-instance output reference yref [B, ny] (None:
    the controller's own), differentiable with respect to the three.  return_status: (cmd, status) instead.  `controller` may be a bank
    (libmpc_amd.LMPCHetero): model [B] is then the controller of every instance (None: instance b = controller b), passed to the solve and
    to the backward launch (LMPCHetero.sensitivityBatch); None is then each controller's own reference."""
    import torch
    _, dev = controller._torch()
    from .bank import LMPCHetero
    is_bank = isinstance(controller, LMPCHetero)
    if model is not None and not is_bank:
        raise ValueError("lmpc_cmd: model= is the instance -> controller map of a bank (LMPCHetero)")
    as_t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)).to(device=dev, dtype=torch.float64)
    x0, u0, yref = as_t(x0), as_t(u0), as_t(yref)
    if yref is not None and yref.dim() != 2 and yref.requires_grad:
        raise ValueError("lmpc_cmd differentiates a per-instance output reference [B, ny]; a per-step reference has no gradient here")
    cmd, status = _function().apply(controller, x0, u0, yref, (model,) if is_bank else None)      # (a tuple: the map passes through apply as it is)
    return (cmd, status) if return_status else cmd
