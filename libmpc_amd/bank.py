"""A mixed batch over a few different controllers.

The engine's batch is B instances of ONE controller (one model, one set of weights and bounds: what a `mpc::LMPC<>` object
is in the reference).  A fleet usually has a handful of vehicle variants, not B: `LMPCBank` holds K controllers, takes a
batch whose instances carry a controller index, solves each group on its own HIP stream (the handles are independent: own
workspace, own dispatch queues, so the groups overlap on the GPU) and returns the results in the caller's order.

This is heterogeneity by grouping -- no new kernel, every instance is solved by exactly the code path and with exactly the
results of its own controller.  `LMPCHetero` is the other end: K controllers (K up to the batch size: every instance its own
A, B, C, weights, bounds) behind ONE set of kernels, each instance reading its own model's factors from HBM
(mpcx_lmpc_hetero_*, include/mpcx.h).  torch is used for what it is here for: device memory, index_select / index_copy and
streams."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

import ctypes as C

from . import _capi
from ._capi import check
from .lmpc import LMPC, BatchResult, ClosedLoopResult, Loop, SensitivityResult, _LoopFrontEnd


def group_by_model(model, n_models: int):
    """Stable grouping of instance indices by controller index.  Returns (order, offsets): `order[offsets[k]:offsets[k+1]]`
    are the instances of controller k in their original relative order."""
    model = np.asarray(model, dtype=np.int64).reshape(-1)
    if model.size and (model.min() < 0 or model.max() >= n_models):
        raise ValueError("controller index out of range")
    order = np.argsort(model, kind="stable")
    counts = np.bincount(model, minlength=n_models)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return order, offsets


PARAM_OUTPUTS = ("oweight", "uweight", "duweight", "lower", "upper")
MODEL_OUTPUTS = ("A", "B", "C", "Bd", "Dd")


@dataclass
class BankGradientResult:
    """Gradients of sum(seed * output) of a bank's solved batch with respect to the weights, the bounds and the model of the controller each
    instance was solved with (mpcx_lmpc_hetero_gradient_batch), device tensors.  Per instance: d_oweight [B, ny, ph],
    d_uweight, d_duweight [B, nu, ph], d_lower, d_upper [B, m_ref], d_A [B, nx, nx], d_B [B, nx, nu], d_C [B, ny, nx], d_Bd [B, nx, ndu],
    d_Dd [B, ny, ndu], indexed as the setters' matrices (None: not asked for; d_Bd, d_Dd None without exogenous inputs); the rows of a flagged
    instance are NaN.  Per controller (per_controller=True): c_* the same with K in front, row k the sum over controller k's instances whose
    flag is 0 in their order in the batch, and n_used [K] how many those were.  flags [B] as SensitivityResult's."""
    d_oweight: "object" = None
    d_uweight: "object" = None
    d_duweight: "object" = None
    d_lower: "object" = None
    d_upper: "object" = None
    d_A: "object" = None
    d_B: "object" = None
    d_C: "object" = None
    d_Bd: "object" = None
    d_Dd: "object" = None
    flags: "object" = None
    c_oweight: "object" = None
    c_uweight: "object" = None
    c_duweight: "object" = None
    c_lower: "object" = None
    c_upper: "object" = None
    c_A: "object" = None
    c_B: "object" = None
    c_C: "object" = None
    c_Bd: "object" = None
    c_Dd: "object" = None
    n_used: "object" = None


class LMPCBank:
    """K `libmpc_amd.LMPC` controllers of equal dimensions behind one `optimizeBatch(x0, lastU, model, ...)`."""

    def __init__(self, controllers):
        if not controllers:
            raise ValueError("at least one controller")
        c0 = controllers[0]
        for c in controllers:
            if (c.nx, c.nu, c.ny, c.ph, c.device) != (c0.nx, c0.nu, c0.ny, c0.ph, c0.device):
                raise ValueError("the controllers of a bank share their dimensions and their device")
            if c._has_terminal != c0._has_terminal:
                raise ValueError("a bank has a terminal cost in every controller or in none (setTerminalCost); P, xT and Tx may differ")
        self.controllers = list(controllers)
        self.nx, self.nu, self.ny, self.ph, self.device = c0.nx, c0.nu, c0.ny, c0.ph, c0.device
        self._streams = [torch.cuda.Stream(device=self.device) for _ in controllers]

    def optimizeBatch(self, x0, lastU, model, yref=None, want_sequence=False) -> BatchResult:
        """x0 [B, nx], lastU [B, nu], model [B] (controller index per instance), yref None | [B, ny] | [B, ph, ny]."""
        dev = torch.device("cuda", self.device)
        x0 = torch.as_tensor(x0, dtype=torch.float64, device=dev)
        lastU = torch.as_tensor(lastU, dtype=torch.float64, device=dev)
        if yref is not None:
            yref = torch.as_tensor(yref, dtype=torch.float64, device=dev)
        B = x0.shape[0]
        order, offsets = group_by_model(model.cpu().numpy() if torch.is_tensor(model) else model, len(self.controllers))
        if order.size != B:
            raise ValueError("one controller index per instance")
        order_t = torch.from_numpy(order).to(dev)
        out = BatchResult(cmd=torch.empty((B, self.nu), dtype=torch.float64, device=dev),
                          cost=torch.empty(B, dtype=torch.float64, device=dev),
                          status=torch.empty(B, dtype=torch.int32, device=dev),
                          solver_status=torch.empty(B, dtype=torch.int32, device=dev),
                          is_feasible=torch.empty(B, dtype=torch.int32, device=dev),
                          iterations=torch.empty(B, dtype=torch.int32, device=dev))
        if want_sequence:
            out.seq_state = torch.empty((B, self.ph + 1, self.nx), dtype=torch.float64, device=dev)
            out.seq_output = torch.empty((B, self.ph + 1, self.ny), dtype=torch.float64, device=dev)
            out.seq_input = torch.empty((B, self.ph + 1, self.nu), dtype=torch.float64, device=dev)
        cur = torch.cuda.current_stream(dev)
        keep = []
        for k, c in enumerate(self.controllers):
            lo, hi = int(offsets[k]), int(offsets[k + 1])
            if hi == lo:
                continue
            s = self._streams[k]
            s.wait_stream(cur)                                   # the inputs were produced on the caller's stream
            with torch.cuda.stream(s):
                idx = order_t[lo:hi]
                xk, uk = x0.index_select(0, idx), lastU.index_select(0, idx)
                yk = None if yref is None else yref.index_select(0, idx)
                r = c.optimizeBatch(xk, uk, yref=yk, want_sequence=want_sequence, stream=s)
                for name in ("cmd", "cost", "status", "solver_status", "is_feasible", "iterations") + \
                        (("seq_state", "seq_output", "seq_input") if want_sequence else ()):
                    getattr(out, name).index_copy_(0, idx, getattr(r, name))
                keep.append((r, xk, uk, yk, idx))
            cur.wait_stream(s)                                   # the caller's stream sees the scattered results
        out._inputs = keep
        return out


class LMPCHetero(_LoopFrontEnd):
    """K configured `libmpc_amd.LMPC` controllers (host-only handles, `device=-1`, are enough) of equal dimensions and equal
    pattern of finite bounds, solved together by one set of kernels: instance b uses controller `model[b]` (default: b).
    In the reference each of them is its own `mpc::LMPC<>` object (LMPC.hpp:751)."""

    def __init__(self, controllers, device=0, condense_on_host=False):
        """condense_on_host: every controller's prediction matrices, Hessian and factors on the host cores instead of by the
        device kernel (lmpc_hetero.hip; the default wherever the dimensions fit it)"""
        if not controllers:
            raise ValueError("at least one controller")
        c0 = controllers[0]
        self.nx, self.nu, self.ny, self.ndu, self.ph = c0.nx, c0.nu, c0.ny, c0.ndu, c0.ph
        self.device = int(device)
        self._lib = _capi.lib()
        arr = (C.c_void_p * len(controllers))(*[c._h for c in controllers])
        self._h = C.c_void_p()
        check(self._lib.mpcx_lmpc_hetero_create_ex(arr, len(controllers), self.device, int(bool(condense_on_host)), C.byref(self._h)))
        n, aw, mref, bpm = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(self._lib.mpcx_lmpc_hetero_get_info(self._h, C.byref(n), C.byref(aw), C.byref(mref), C.byref(bpm)))
        self.count, self.active_words, self.m_ref, self.bytes_per_model = n.value, aw.value, mref.value, bpm.value
        self._template = c0
        self._models = [(c._A, c._B, c._Bd) for c in controllers]        # as given to the setters: what plants=(A, None, None) completes
        self._outputs = [c._C for c in controllers]
        self._feedthrough = [c._Dd for c in controllers]
        self._controllers = list(controllers)                            # (their handles hold the weights: lqr_terminal_costs)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.mpcx_lmpc_hetero_destroy(self._h)
            self._h = None

    def info(self):
        return {"active_words": self.active_words, "m_ref": self.m_ref}

    def debug_get(self, k, name):
        """testing aid: an O(n^3) array of controller k as the bank holds it on the device"""
        f = self._lib.mpcx_lmpc_hetero_debug_get
        n = check(f(self._h, int(k), name.encode(), None, 0))
        out = np.zeros(n)
        check(f(self._h, int(k), name.encode(), out.ctypes.data_as(C.c_void_p), n))
        return out

    def make_batch(self, x0, u0, model=None, **kw):
        b, res, keep = LMPC.make_batch(self, x0, u0, **kw)      # the descriptor is the single-controller one: it only needs the dimensions and info()
        mi = None
        if model is not None:
            mi = torch.as_tensor(model).to(device=torch.device("cuda", self.device), dtype=torch.int32).contiguous()
            if mi.numel() != b.batch or (mi.numel() and (int(mi.min()) < 0 or int(mi.max()) >= self.count)):
                raise ValueError("model: one controller index in [0, %d) per instance" % self.count)
        return b, res, keep + (mi,), mi

    def launch(self, b, mi=None, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        check(self._lib.mpcx_lmpc_hetero_solve_batch(self._h, C.byref(b), None if mi is None else C.c_void_p(mi.data_ptr()), C.c_void_p(s.cuda_stream)))

    def time_launches(self, b, mi, repeats, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        ms = C.c_float()
        check(self._lib.mpcx_lmpc_hetero_time_solve_batch(self._h, C.byref(b), None if mi is None else C.c_void_p(mi.data_ptr()),
                                                          C.c_void_p(s.cuda_stream), int(repeats), C.byref(ms)))
        return ms.value

    def optimizeBatch(self, x0, lastU, model=None, yref=None, uref=None, duref=None, dmeas=None, want_active=False, want_sequence=False,
                      stream=None, warm=None, warm_shift=False, sensitivities=False) -> BatchResult:
        """x0 [B, nx], lastU [B, nu]; model [B] controller index per instance (None: instance b = controller b); references None
        (each controller's own) | [B, n] | [B, ph, n]; warm / warm_shift: a previous result's active sets as the first working sets, as
        LMPC.optimizeBatch takes them.  sensitivities=True: the Jacobians of cmd on the active sets this solve wrote, as
        `result.sensitivities` (one more launch on the same stream)"""
        b, res, keep, mi = self.make_batch(x0, lastU, model, yref=yref, uref=uref, duref=duref, dmeas=dmeas, want_active=want_active or sensitivities,
                                           want_sequence=want_sequence, warm=warm, warm_shift=warm_shift)
        self.launch(b, mi, stream)
        res._inputs = keep
        res._batch, res._model = b, mi         # the descriptor and the map: gradientBatch differentiates the batch they describe
        if sensitivities:
            res.sensitivities = self.sensitivityBatch(res.active_lower, res.active_upper, model=mi, status=res.status, stream=stream)
        return res

    # -- sensitivities of a solved batch (mpcx_lmpc_hetero_sensitivity_batch) ----------------------------------
    def _model_index(self, model, B):
        """model as make_batch validates it: None, or one controller index in [0, count) per instance, int32 on the device"""
        if model is None:
            if B != self.count:
                raise ValueError("model: without it the batch must be the bank (instance b = controller b)")
            return None
        mi = torch.as_tensor(model).to(device=torch.device("cuda", self.device), dtype=torch.int32).contiguous()
        if mi.numel() != B or (mi.numel() and (int(mi.min()) < 0 or int(mi.max()) >= self.count)):
            raise ValueError("model: one controller index in [0, %d) per instance" % self.count)
        return mi

    def make_sensitivity(self, active_lower, active_upper, model=None, status=None, seed_cmd=None, seed_input=None, want=("x0", "u0", "yref")):
        """Allocate outputs and fill the mpcx_lmpc_sens descriptor, which is the single-controller one.  Returns (Sens, SensitivityResult,
        keepalive, model index on the device | None)."""
        d, out, keep = LMPC.make_sensitivity(self, active_lower, active_upper, status, seed_cmd, seed_input, want)
        mi = self._model_index(model, d.batch)
        return d, out, keep + (mi,), mi

    def launch_sensitivity(self, desc, mi=None, stream=None, keep=None):
        """One asynchronous launch for a descriptor built by make_sensitivity(); streams as in LMPC.launch()."""
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
            for t in (keep or ()):
                if t is not None:
                    t.record_stream(s)
        check(self._lib.mpcx_lmpc_hetero_sensitivity_batch(self._h, C.byref(desc), None if mi is None else C.c_void_p(mi.data_ptr()),
                                                           C.c_void_p(s.cuda_stream)))

    def sensitivityBatch(self, active_lower, active_upper, model=None, status=None, seed_cmd=None, seed_input=None, stream=None,
                         want=("x0", "u0", "yref")) -> SensitivityResult:
        """LMPC.sensitivityBatch for a bank: the slope of solved instances on their active sets, instance b differentiated on controller
        model[b] (None: controller b) -- one launch.  active_lower / active_upper [B, active_words] as optimizeBatch(want_active=True)
        wrote them; status [B] (optional) marks the instances that were not solved.  Without seeds: the Jacobians of cmd.  seed_cmd
        [B, nu] and / or seed_input [B, ph + 1, nu]: the vector-Jacobian products.  want: which outputs to compute."""
        d, out, keep, mi = self.make_sensitivity(active_lower, active_upper, model, status, seed_cmd, seed_input, want)
        self.launch_sensitivity(d, mi, stream, keep)
        out._inputs = keep[:5] + (mi,)
        return out

    # -- gradients on weights, bounds and models of a solved batch (mpcx_lmpc_hetero_gradient_batch) --------------
    def make_gradient(self, result, model=None, seed_cmd=None, seed_input=None, per_controller=False, want=PARAM_OUTPUTS + MODEL_OUTPUTS):
        """Allocate outputs and fill the mpcx_lmpc_bank_grad descriptor for `result`: what optimizeBatch(..., want_active=True,
        want_sequence=True) of this bank returned (or the Batch descriptor of make_batch, whose tensors the caller keeps alive), with the
        `model` it was solved with.  per_controller: the sums over each controller's instances besides, the grouping (group_by_model) built
        and uploaded here, so that the launch allocates nothing.  Returns (BankGrad, BankGradientResult, keepalive, model index on the
        device | None)."""
        b = getattr(result, "_batch", result)
        if not isinstance(b, _capi.Batch):
            raise ValueError("gradientBatch needs the result of optimizeBatch(want_active=True, want_sequence=True) or a Batch descriptor")
        unknown = [n for n in want if n not in PARAM_OUTPUTS + MODEL_OUTPUTS]
        if unknown or not want:
            raise ValueError("want: names out of %s" % (PARAM_OUTPUTS + MODEL_OUTPUTS,))
        with_model = any(n in want for n in ("A", "B", "C")) or (self.ndu > 0 and any(n in want for n in ("Bd", "Dd")))
        if not (b.active_lower and b.active_upper and b.seq_output and b.seq_input and (b.seq_state or not with_model)):
            raise ValueError("the batch must have been solved with want_active=True and want_sequence=True")
        if seed_cmd is None and seed_input is None:
            raise ValueError("a gradient needs seed_cmd or seed_input")
        B = int(b.batch)
        if model is None and B != self.count:
            raise ValueError("model: without it the batch must be the bank (instance b = controller b)")
        _, dev = self._torch()
        mi = self._model_index(model, B)
        sc = self._dev(torch, dev, seed_cmd, (B, self.nu))
        si = self._dev(torch, dev, seed_input, (B, self.ph + 1, self.nu))
        f64, K = torch.float64, self.count
        # (the kernel writes each matrix column-major, as its setter reads it: allocated [columns, rows], handed out transposed)
        shapes = {"oweight": (self.ph, self.ny), "uweight": (self.ph, self.nu), "duweight": (self.ph, self.nu), "lower": (self.m_ref,),
                  "upper": (self.m_ref,), "A": (self.nx, self.nx), "B": (self.nu, self.nx), "C": (self.nx, self.ny), "Bd": (self.ndu, self.nx),
                  "Dd": (self.ndu, self.ny)}
        names = [n for n in PARAM_OUTPUTS + MODEL_OUTPUTS if n in want and int(np.prod(shapes[n])) > 0]
        dt = {n: torch.empty((B,) + shapes[n], dtype=f64, device=dev) for n in names}
        ct = {n: torch.empty((K,) + shapes[n], dtype=f64, device=dev) for n in names} if per_controller else {}
        flags = torch.empty((B,), dtype=torch.int32, device=dev)
        order = offsets = n_used = None
        if per_controller:
            idx = np.arange(B) if mi is None else mi.cpu().numpy()
            o, off = group_by_model(idx, K)
            order = torch.from_numpy(o.astype(np.int32)).to(dev)
            offsets = torch.from_numpy(off.astype(np.int32)).to(dev)
            n_used = torch.zeros((K,), dtype=torch.int32, device=dev)
        tr = lambda t: t.transpose(-1, -2) if t.dim() == 3 else t
        out = BankGradientResult(flags=flags, n_used=n_used, **{"d_" + n: tr(t) for n, t in dt.items()}, **{"c_" + n: tr(t) for n, t in ct.items()})

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())
        d = _capi.BankGrad()
        d.solved = C.cast(C.pointer(b), C.c_void_p)
        d.seed_cmd, d.seed_input, d.flags = ptr(sc), ptr(si), ptr(flags)
        for n in PARAM_OUTPUTS + MODEL_OUTPUTS:
            setattr(d, "d_" + n, ptr(dt.get(n)))
            setattr(d, "c_" + n, ptr(ct.get(n)))
        d.group_order, d.group_offsets, d.n_used = ptr(order), ptr(offsets), ptr(n_used)
        keep = (b, result, sc, si, flags, order, offsets, n_used, mi) + tuple(dt.values()) + tuple(ct.values())
        return d, out, keep, mi

    def launch_gradient(self, desc, mi=None, stream=None, keep=None):
        """One asynchronous launch (two kernels with per-controller sums) for a descriptor built by make_gradient(); streams as in
        LMPC.launch()."""
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
            for t in (keep or ()):
                if isinstance(t, torch.Tensor):
                    t.record_stream(s)
        check(self._lib.mpcx_lmpc_hetero_gradient_batch(self._h, C.byref(desc), None if mi is None else C.c_void_p(mi.data_ptr()),
                                                        C.c_void_p(s.cuda_stream)))

    def gradientBatch(self, result, model=None, seed_cmd=None, seed_input=None, per_controller=False, stream=None,
                      want=PARAM_OUTPUTS + MODEL_OUTPUTS) -> BankGradientResult:
        """The gradient of sum(seed_cmd * cmd) + sum(seed_input * input sequence) of a solved batch with respect to OWeight, UWeight,
        DeltaUWeight, to every bound of the QP and to every entry of A, B, C, Bd, Dd of the controller each instance was solved with: one
        launch after the solve, on each instance's active set.  result: what optimizeBatch(..., want_active=True, want_sequence=True) of this
        bank returned, unchanged since; model as it was given there (None: the one the result remembers).  per_controller: the sums over each
        controller's instances as well (in a fixed order: the same bits every time).  want: which outputs to compute; without a model output
        the model part of the kernel does not run."""
        if model is None:
            model = getattr(result, "_model", None)
        d, out, keep, mi = self.make_gradient(result, model, seed_cmd, seed_input, per_controller, want)
        self.launch_gradient(d, mi, stream, keep)
        out._inputs = keep
        return out

    # -- the closed loop on the device (mpcx_lmpc_hetero_loop_create*; the loop itself is _LoopFrontEnd's) ---------------------
    _loop_entry = "mpcx_lmpc_hetero_loop_create"

    def _own_plant(self, B, model=None):
        """A, B, Bd of each instance's own controller, [B, nx, .] numpy"""
        idx = np.arange(B) if model is None else np.asarray(model.cpu() if torch.is_tensor(model) else model, dtype=np.int64).reshape(-1)
        if any(m[0] is None for m in self._models):
            raise _capi.MpcxError(_capi.E_STATE, "state-space model not set")
        return tuple(np.stack([m[j] for m in self._models])[idx] for j in range(3))

    def kalman_gains(self, Qw, Rv):
        """The steady-state Kalman predictor gain of every controller's own (A, C), [count, nx, ny] on the device, for the process-noise
        covariance Qw ([nx, nx], or [count, nx, nx] one per controller) and the sensor-noise covariance Rv ([ny, ny] or [count, ny, ny]):
        one batched device call (libmpc_amd.utils.kalman_gains) where LMPC.kalman_gain iterates one controller on the host.  Index it by
        the instances' controllers (gains[model]) for observer=.  Raises MpcxError naming the first controller whose equation was not
        solved."""
        from .utils import kalman_gains
        if any(m[0] is None for m in self._models):
            raise _capi.MpcxError(_capi.E_STATE, "state-space model not set")
        A = np.stack([m[0] for m in self._models]); Cm = np.stack(self._outputs)
        L, _, flags = kalman_gains(A, Cm, Qw, Rv, device=self.device)
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            k = int(bad[0])
            why = {1: "Rv is not positive definite", 2: "the doubling iteration has not converged",
                   3: "the doubling iteration broke down: is (A, C) detectable?"}[int(flags[k])]
            raise _capi.MpcxError(_capi.E_NUMERIC, f"controller {k}: {why}")
        return L

    def disturbance_gains(self, Qw, Qd, Rv):
        """LMPC.disturbance_gain for every controller of the bank, [count, nx+ndu, ny] on the device, in one batched call
        (libmpc_amd.utils.disturbance_gains): the gains [Lx; Ld] of each controller's model augmented with its integrating disturbance model.
        Index it by the instances' controllers (gains[model]) for disturbance_observer=.  ValueError, before any device call, naming the first
        controller whose augmented pair is not detectable; MpcxError naming the first whose equation was not solved."""
        from .utils import disturbance_gains
        if any(m[0] is None for m in self._models):
            raise _capi.MpcxError(_capi.E_STATE, "state-space model not set")
        A = np.stack([m[0] for m in self._models]); Bd = np.stack([m[2] for m in self._models])
        L, _, flags = disturbance_gains(A, Bd, np.stack(self._outputs), np.stack(self._feedthrough), Qw, Qd, Rv, device=self.device)
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            k = int(bad[0])
            why = {1: "Rv is not positive definite", 2: "the doubling iteration has not converged",
                   3: "the doubling iteration broke down"}[int(flags[k])]
            raise _capi.MpcxError(_capi.E_NUMERIC, f"controller {k}: {why}")
        return L

    def lqr_terminal_costs(self, step=1):
        """LMPC.lqr_terminal_cost for every controller of the bank, (P [count, nx, nx], K [count, nu, nx]) on the device, in one batched
        mpcx_dare_batch call (libmpc_amd.utils.lqr_gains).  A terminal cost is part of a controller: give each its P with setTerminalCost
        before the bank is created from them.  ValueError where an input weight is not positive; MpcxError naming the first controller whose
        equation was not solved."""
        from .utils import lqr_gains
        A, B, Q, R = (np.stack(m) for m in zip(*[c._lqr_problem(step) for c in self._controllers]))
        K, X, flags = lqr_gains(A, B, Q, R, device=self.device)
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            raise _capi.MpcxError(_capi.E_NUMERIC, f"controller {int(bad[0])}: the Riccati equation was not solved (flag {int(flags[int(bad[0])])})")
        return X, K

    def target_maps(self):
        """LMPC.target_map for every controller of the bank, [count, nu, ny+ndu+nu] on the device, in one batched call
        (libmpc_amd.utils.target_maps).  Index it by the instances' controllers (maps[model]) for target=.  ValueError, before any device call,
        naming the first controller that misses a rank condition; MpcxError naming the first whose KKT system is singular all the same."""
        from .utils import target_maps
        if any(m[0] is None for m in self._models):
            raise _capi.MpcxError(_capi.E_STATE, "state-space model not set")
        A, B, Bd = (np.stack([m[j] for m in self._models]) for j in range(3))
        T, flags = target_maps(A, B, Bd, np.stack(self._outputs), np.stack(self._feedthrough), device=self.device)
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            raise _capi.MpcxError(_capi.E_NUMERIC, f"controller {int(bad[0])}: the KKT system of the target is singular")
        return T

    def make_loop(self, x0, lastU, ticks, model=None, plant=None, plants=None, yref=None, uref=None, duref=None, dmeas=None, preview=False,
                  noise=None, warm=True, stream=None, observer=None, xhat0=None, meas_noise=None, disturbance_observer=None, dhat0=None,
                  target=None) -> Loop:
        """LMPC.make_loop for a bank: every tick is the bank's batched solve (instance b by controller model[b]; None: controller b)
        followed by the plant step.  plant: one plant for all, (A_p, B_p, Bd_p); plants: a plant per instance, (A [B,nx,nx],
        B [B,nx,nu] | None, Bd | None); a None entry of either, and no plant at all, mean each instance's own controller.  References:
        None is each controller's own, also for the exogenous input that drives the plant.  observer, xhat0, meas_noise: output feedback as
        in LMPC.make_loop, instance b estimated with its own controller's model; the gain is per instance, [B, nx, ny] (the controllers
        differ: one gain for all raises ValueError).  disturbance_observer, dhat0: offset-free tracking as in LMPC.make_loop, the gain
        [B, nx+ndu, ny] (LMPCHetero.disturbance_gains indexed by the instances' controllers); dmeas= is then the true disturbance, None each
        controller's own exogenous input.  target: steady-state targets as in LMPC.make_loop, the map [B, nu, ny+ndu+nu]
        (LMPCHetero.target_maps indexed by the instances' controllers); yref / uref None: each controller's own as r and ubar.  Destroy the
        loop before the bank."""
        x0t = x0 if hasattr(x0, "shape") else np.asarray(x0)
        B = int(x0t.shape[0])
        plants = self._check_plants(B, plant, plants)
        checked = self._check_observers(B, int(ticks), observer, disturbance_observer, xhat0, dhat0, meas_noise, bank=True)
        self._check_target(B, target, disturbance_observer, bank=True)
        mi = None
        if model is not None:
            mi = torch.as_tensor(model).to(device=torch.device("cuda", self.device), dtype=torch.int32).contiguous()
            if mi.numel() != B or (mi.numel() and (int(mi.min()) < 0 or int(mi.max()) >= self.count)):
                raise ValueError("model: one controller index in [0, %d) per instance" % self.count)
        if plant is not None:
            plant = tuple(plant) + (None,) * (3 - len(plant))
            if any(m is None and cols > 0 for m, cols in zip(plant, (self.nx, self.nu, self.ndu))):
                # a bank has no one model to complete a partial plant with: the given matrices for every instance, the rest each instance's own
                plants = tuple(None if m is None else np.broadcast_to(np.asarray(m, dtype=np.float64), (B,) + np.shape(m)) for m in plant)
                plant = None

        loop = self._make_loop(x0, lastU, ticks, plant, plants, yref, uref, duref, dmeas, preview, noise, warm, stream, model=mi,
                               observer=observer, xhat0=xhat0, meas_noise=meas_noise, bank=True, disturbance_observer=disturbance_observer, dhat0=dhat0, checked=checked,
                               target=target)
        loop.keep += (mi,)
        return loop

    def simulate(self, x0, lastU, ticks, model=None, plant=None, plants=None, yref=None, uref=None, duref=None, dmeas=None, preview=False,
                 noise=None, warm=True, stream=None, observer=None, xhat0=None, meas_noise=None, disturbance_observer=None, dhat0=None,
                 target=None) -> ClosedLoopResult:
        """make_loop + run_loop + destroy_loop: one closed-loop run, synchronised."""
        loop = self.make_loop(x0, lastU, ticks, model, plant, plants, yref, uref, duref, dmeas, preview, noise, warm,
                              observer=observer, xhat0=xhat0, meas_noise=meas_noise, disturbance_observer=disturbance_observer, dhat0=dhat0,
                              target=target)
        try:
            self.run_loop(loop, stream)
            (stream if stream is not None else torch.cuda.current_stream(self.device)).synchronize()
        finally:
            self.destroy_loop(loop)
        return loop.result
