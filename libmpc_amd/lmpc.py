"""Host-side mirror of libmpc++'s linear MPC front-end for the batched MI355X engine.

`LMPC` keeps the method names, argument meaning and return/raise behaviour of
`mpc::LMPC<>` (reference include/mpc/LMPC.hpp, and its pybind export
python/pybind_export.cpp:59-123) for the one path this package replaces -- what sits
behind `optimize()` -- and adds `optimizeBatch()`: B independent instances of the same
controller solved by one HIP kernel launch through the C ABI in include/mpcx.h.

PyTorch is plumbing here (device buffers and streams), not the product: all numerics
run in libmpcx.so.  There is no CPU fallback; a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from ._capi import LParams, MpcxError, check

inf = float("inf")


class HorizonSlice:
    """Half-open step range [start, end); {-1,-1} = whole horizon (Types.hpp:57-82)."""

    def __init__(self, start, end):
        self.start, self.end = int(start), int(end)

    @staticmethod
    def all():
        return HorizonSlice(-1, -1)


def _slice(s):
    if s is None:
        return HorizonSlice.all()
    if isinstance(s, HorizonSlice):
        return s
    a, b = s
    return HorizonSlice(a, b)


class SolutionStats:
    """mpc::SolutionStats (Profiler.hpp:19-60) as the pybind module exposes it; times in seconds"""

    def __init__(self):
        self.totalSolutionTime = 0.0
        self.numberOfSolutions = 0
        self.minSolutionTime = float("inf")
        self.maxSolutionTime = 0.0
        self.averageSolutionTime = 0.0
        self.standardDeviation = 0.0
        self.solutionsStates = {}
        self._sq = 0.0

    def add(self, dt, status):
        self.totalSolutionTime += dt
        self.numberOfSolutions += 1
        self.minSolutionTime = min(self.minSolutionTime, dt)
        self.maxSolutionTime = max(self.maxSolutionTime, dt)
        self._sq += dt * dt
        n = self.numberOfSolutions
        self.averageSolutionTime = self.totalSolutionTime / n
        self.standardDeviation = max(self._sq / n - self.averageSolutionTime ** 2, 0.0) ** 0.5
        self.solutionsStates[status] = self.solutionsStates.get(status, 0) + 1


class ResultStatus:
    SUCCESS, MAX_ITERATION, INFEASIBLE, ERROR, UNKNOWN = range(5)


def LParameters(**kw) -> LParams:
    """mpc::LParameters with the reference defaults (Types.hpp:146-161)."""
    p = LParams()
    _capi.lib().mpcx_lparams_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


@dataclass
class Result:
    """mpc::Result<nu> (Types.hpp:168-182)."""
    solver_status: int = 0
    is_feasible: bool = False
    solver_status_msg: str = ""
    cost: float = 0.0
    status: int = ResultStatus.UNKNOWN
    cmd: np.ndarray = field(default_factory=lambda: np.zeros(0))


@dataclass
class OptSequence:
    """mpc::OptSequence (Types.hpp:184-198): row i = horizon step i."""
    state: np.ndarray
    output: np.ndarray
    input: np.ndarray


@dataclass
class BatchResult:
    """Result<nu> for B instances as structure-of-arrays of device tensors."""
    cmd: "object"
    cost: "object"
    status: "object"
    solver_status: "object"
    is_feasible: "object"
    iterations: "object"
    active_lower: "object" = None
    active_upper: "object" = None
    seq_state: "object" = None
    seq_output: "object" = None
    seq_input: "object" = None
    polish_rounds: "object" = None
    active_count: "object" = None
    sensitivities: "object" = None      # a SensitivityResult (optimizeBatch(..., sensitivities=True))


@dataclass
class ParamSensitivityResult:
    """Gradients of sum(seed * output) of a solved batch with respect to the controller's weights and bounds (mpcx_lmpc_param_sensitivity_batch,
    DESIGN.md 4.9), device tensors.  Per instance: d_oweight [B, ny, ph], d_uweight, d_duweight [B, nu, ph] -- indexed as the matrices
    setObjectiveWeights takes --, d_lower, d_upper [B, m_ref] in the row numbering of the active sets; reduced: the same without the leading
    B, summed over the instances whose flag is 0, and n_used [1] how many those were.  flags [B] as SensitivityResult's; per instance, the
    rows of a flagged instance are NaN."""
    d_oweight: "object"
    d_uweight: "object"
    d_duweight: "object"
    d_lower: "object"
    d_upper: "object"
    flags: "object"
    n_used: "object" = None


@dataclass
class ModelSensitivityResult:
    """Gradients of sum(seed * output) of a solved batch with respect to the model (mpcx_lmpc_model_sensitivity_batch), device
    tensors.  Per instance: d_A [B, nx, nx], d_B [B, nx, nu], d_C [B, ny, nx], d_Bd [B, nx, ndu], d_Dd [B, ny, ndu] -- indexed as the matrices
    setStateSpaceModel / setDisturbances take (d_Bd, d_Dd None without exogenous inputs) --; reduced: the same without the leading B, summed
    over the instances whose flag is 0, and n_used [1] how many those were.  flags [B] as SensitivityResult's; per instance, the entries of a
    flagged instance are NaN."""
    d_A: "object"
    d_B: "object"
    d_C: "object"
    d_Bd: "object"
    d_Dd: "object"
    flags: "object"
    n_used: "object" = None


@dataclass
class SensitivityResult:
    """The slope of a solved batch on each instance's active set (mpcx_lmpc_sensitivity_batch), device tensors.
    Jacobian mode: d_x0 [B, nu, nx], d_u0 [B, nu, nu], d_yref [B, nu, ny] -- the local feedback law
    cmd ~ cmd* + d_x0 (x - x0) + d_u0 (lastU - u0) + d_yref (yref - yref0).  With seeds: the gradients [B, nx], [B, nu], [B, ny] of
    sum(seed * output).  d_yref is with respect to a shift of the output reference common to all steps.  flags [B]: 0 fine, 1 not solved,
    2 dependent working set, 3 working set larger than the kernel's plan; the rows of an instance with a non-zero flag are NaN."""
    d_x0: "object"
    d_u0: "object"
    d_yref: "object"
    flags: "object"


@dataclass
class ClosedLoopResult:
    """A closed-loop run on the device (LMPC.simulate), tick-major device tensors: x [ticks+1, B, nx] (row 0 = the initial
    state), u [ticks, B, nu], the others [ticks, B].  An observed loop (observer=) also fills xhat [ticks+1, B, nx], the estimates
    the solves read (row 0 = xhat0), and y [ticks, B, ny], the measurements; x is then the plant's true state.  An offset-free loop
    (disturbance_observer=) fills those and dhat [ticks+1, B, ndu], the disturbance estimates the solves read (row 0 = dhat0); with
    steady-state targets (target=) also us [ticks+1, B, nu], the input references the solves read (row k: tick k's; the last row is computed
    and not used)."""
    x: "object"
    u: "object"
    cost: "object"
    status: "object"
    solver_status: "object"
    iterations: "object"
    polish_rounds: "object"
    active_count: "object"
    xhat: "object" = None
    y: "object" = None
    dhat: "object" = None
    us: "object" = None
    gradient: "object" = None           # a LoopGradientResult (LMPC.simulate(..., gradient=dict(...)))


@dataclass
class LoopGradientResult:
    """Gradients of sum(seed_x * x) + sum(seed_u * u) of a closed-loop run (mpcx_lmpc_loop_grad_*), device tensors.  Per instance
    always: d_x0 [B, nx], d_u0 [B, nu], d_yref [B, ny] (a shift of the output reference common to all steps and ticks), d_noise [ticks, B, nx].
    Per instance [B, ..] or, reduced, without the leading B and summed over the instances whose flag is 0 (n_used [1]: how many): the plant
    d_plant_A [nx, nx], d_plant_B [nx, nu], d_plant_Bd [nx, ndu] (views of one tensor; None without exogenous inputs), the weights d_oweight
    [ny, ph], d_uweight, d_duweight [nu, ph] and the controller's model d_A, d_B, d_C, d_Bd, d_Dd, indexed as their setters take them.  flags [B]:
    0, or the OR over the ticks of SensitivityResult's codes; every per-instance entry of a flagged instance is NaN.  What was not asked for is
    None.  handle, seed_x, seed_u: the native object and the seeds as every run reads them (refill in place)."""
    d_x0: "object" = None
    d_u0: "object" = None
    d_yref: "object" = None
    d_noise: "object" = None
    d_plant_A: "object" = None
    d_plant_B: "object" = None
    d_plant_Bd: "object" = None
    d_oweight: "object" = None
    d_uweight: "object" = None
    d_duweight: "object" = None
    d_A: "object" = None
    d_B: "object" = None
    d_C: "object" = None
    d_Bd: "object" = None
    d_Dd: "object" = None
    flags: "object" = None
    n_used: "object" = None
    handle: "object" = None
    seed_x: "object" = None
    seed_u: "object" = None
    keep: tuple = ()


LOOP_GRADIENT_WANT = ("x0", "u0", "yref", "noise", "plant", "oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")


@dataclass
class Loop:
    """a loop made by LMPC.make_loop / LMPCHetero.make_loop: the native handle, the result whose tensors every run fills, the tensors the graph
    points at, and (plants=) the per-instance plants as every run reads them, [B, nx (nx+nu+ndu)] in LMPC.pack_plants' layout.  An observed
    loop: gains (per-instance observer=) [B, nx ny] in LMPC.pack_gains' layout, xhat0 and meas_noise as every run reads them (refill in place);
    an offset-free loop: gains [B, (nx+ndu) ny] in the same layout, and dhat0; with targets: maps (per-instance target=) [B, nu (ny+ndu+nu)] in
    LMPC.pack_gains' layout (refill in place)"""
    handle: "object"
    result: ClosedLoopResult
    ticks: int
    keep: tuple = ()
    plants: "object" = None
    gains: "object" = None
    xhat0: "object" = None
    meas_noise: "object" = None
    dhat0: "object" = None
    maps: "object" = None


def _cm(a, rows, cols):
    """column-major float64 host copy with a shape check"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1 and cols == 1:
        a = a.reshape(rows, 1)
    if a.shape != (rows, cols):
        raise ValueError(f"expected shape {(rows, cols)}, got {a.shape}")
    return np.asfortranarray(a)


def _vec(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.shape[0] != n:
        raise ValueError(f"expected length {n}, got {a.shape[0]}")
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _shape(a):
    return tuple((a if hasattr(a, "shape") else np.asarray(a)).shape)


class _LoopFrontEnd:
    """What LMPC and LMPCHetero share: device tensors for a descriptor, and the closed loop on the device (mpcx_lmpc_loop_*,
    mpcx_lmpc_hetero_loop_*).  The class that inherits it has nx, nu, ndu, ny, ph, device, _lib, _h and _own_plant."""

    def _torch(self):
        import torch
        if self.device < 0 or not torch.cuda.is_available():
            raise MpcxError(_capi.E_DEVICE, "optimize needs an MI355X: libmpc_amd has no CPU solve path")
        return torch, torch.device("cuda", self.device)

    def _dev(self, torch, dev, a, shape):
        if a is None:
            return None
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        t = t.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _ref(self, torch, dev, a, B, n):
        """classify a per-solve reference: None -> shared, [B,n] -> per instance, [B,ph,n] -> per step"""
        if a is None:
            return None, _capi.REF_SHARED
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        t = t.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(t.shape) == (B, n):
            return t, _capi.REF_PER_INSTANCE
        if tuple(t.shape) == (B, self.ph, n):
            return t, _capi.REF_PER_STEP
        raise ValueError(f"reference must be [B,{n}] or [B,{self.ph},{n}], got {tuple(t.shape)}")

    def _loop_ref(self, torch, dev, a, B, n, ticks, preview):
        """a loop's reference: None -> shared; [B,n] -> per instance; [B,ph,n] -> per step, the same at every tick; with
        preview=True a 3-D array is [B, ticks+ph, n] and tick k sees rows k .. k+ph-1"""
        if a is None:
            return None, _capi.REF_SHARED
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        t = t.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(t.shape) == (B, n):
            return t, _capi.REF_PER_INSTANCE
        if preview and tuple(t.shape) == (B, ticks + self.ph, n):
            return t, _capi.REF_PREVIEW
        if not preview and tuple(t.shape) == (B, self.ph, n):
            return t, _capi.REF_PER_STEP
        want = f"[B,{ticks + self.ph},{n}] (preview)" if preview else f"[B,{self.ph},{n}]"
        raise ValueError(f"reference must be [B,{n}] or {want}, got {tuple(t.shape)}")

    def _check_plants(self, B, plant, plants):
        """plants= as a triple (A [B,nx,nx], B [B,nx,nu] | None, Bd [B,nx,ndu] | None), its shapes checked -- on the host, ahead of any device call"""
        if plant is not None and plants is not None:
            raise ValueError("plant= (one plant for the batch) and plants= (a plant per instance) exclude each other")
        if plants is None:
            return None
        plants = tuple(plants)
        if not 1 <= len(plants) <= 3:
            raise ValueError("plants is (A, B, Bd), the trailing entries optional")
        plants += (None,) * (3 - len(plants))
        for name, m, cols in zip(("A", "B", "Bd"), plants, (self.nx, self.nu, self.ndu)):
            if m is not None and _shape(m) != (B, self.nx, cols):
                raise ValueError(f"plants: {name} must be [{B},{self.nx},{cols}], got {_shape(m)}")
        return plants

    def _check_gain(self, name, gain, rows, B, ticks, xhat0, dhat0, meas_noise, bank):
        """observer= or disturbance_observer= (`name`: [rows, ny] one gain, [B, rows, ny] a gain per instance), xhat0=, dhat0= and meas_noise=, their
        shapes checked -- on the host, ahead of any device call; True for a gain per instance"""
        sh = _shape(gain)
        if sh not in ((rows, self.ny), (B, rows, self.ny)):
            raise ValueError(f"{name} must be [{rows},{self.ny}] or [{B},{rows},{self.ny}], got {sh}")
        if bank and len(sh) == 2:
            raise ValueError(f"a bank's controllers differ: {name} must be a gain per instance, [{B},{rows},{self.ny}]")
        for what, a, want in (("xhat0", xhat0, (B, self.nx)), ("dhat0", dhat0, (B, self.ndu)), ("meas_noise", meas_noise, (ticks, B, self.ny))):
            if a is not None and _shape(a) != want:
                raise ValueError(f"{what} must be [{','.join(map(str, want))}], got {_shape(a)}")
        return len(sh) == 3

    def _check_observers(self, B, ticks, observer, disturbance_observer, xhat0, dhat0, meas_noise, bank=False):
        """the checks of observer= ([nx, ny] or [B, nx, ny]) or of disturbance_observer= ([nx+ndu, ny] or [B, nx+ndu, ny]; the two exclude each
        other), whichever is given: (offset-free?, a gain per instance?)"""
        if disturbance_observer is None and dhat0 is not None:
            raise ValueError("dhat0= belongs to an offset-free loop: give disturbance_observer=")
        if disturbance_observer is not None:
            if observer is not None:
                raise ValueError("observer= (a state observer) and disturbance_observer= (its offset-free form) exclude each other")
            if self.ndu == 0:
                raise ValueError("disturbance_observer= needs a controller with exogenous inputs (ndu > 0) and a disturbance model (setDisturbances)")
            return True, self._check_gain("disturbance_observer", disturbance_observer, self.nx + self.ndu, B, ticks, xhat0, dhat0, meas_noise, bank)
        if observer is None:
            if xhat0 is not None or meas_noise is not None:
                raise ValueError("xhat0= and meas_noise= belong to an observed loop: give observer=")
            return False, False
        return False, self._check_gain("observer", observer, self.nx, B, ticks, xhat0, None, meas_noise, bank)

    def _check_target(self, B, target, disturbance_observer, bank=False):
        """target= ([nu, ny+ndu+nu] one map, [B, nu, ny+ndu+nu] a map per instance): True for a map per instance"""
        if target is None:
            return False
        if disturbance_observer is None:
            raise ValueError("target= (steady-state targets) needs disturbance_observer=: the targets are computed from its disturbance estimate")
        sh = _shape(target)
        n = self.ny + self.ndu + self.nu
        if sh not in ((self.nu, n), (B, self.nu, n)):
            raise ValueError(f"target must be [{self.nu},{n}] or [{B},{self.nu},{n}], got {sh}")
        if bank and len(sh) == 2:
            raise ValueError(f"a bank's controllers differ: target must be a map per instance, [{B},{self.nu},{n}]")
        return len(sh) == 3

    @staticmethod
    def pack_gains(L):
        """[B, nx ny]: per instance L_b column-major -- mpcx_lmpc_observer_desc.gain_batch; a torch tensor [B, nx, ny] in, a tensor out
        (what to copy_ into Loop.gains for the next run)"""
        return L.transpose(1, 2).reshape(L.shape[0], L.shape[1] * L.shape[2]).contiguous()

    _loop_entry = "mpcx_lmpc_loop_create"        # (LMPCHetero: mpcx_lmpc_hetero_loop_create)

    def _create_loop(self, d, od, offset_free, td, bank, model, stream, out):
        """the one of the library's entries that makes this loop: by owner (a controller, or a bank, whose entries also take the model index)
        and by what the loop has -- no observer, an observer (od an ObserverDesc), a disturbance observer (od a DisturbanceObserverDesc),
        targets on top (td)"""
        kind = "" if od is None else "_offset_free_target" if td is not None else "_offset_free" if offset_free else "_observed"
        descs = tuple(C.byref(a) for a in (d, od, td) if a is not None)
        index = (None if model is None else C.c_void_p(model.data_ptr()),) if bank else ()
        return getattr(self._lib, self._loop_entry + kind)(self._h, *descs, *index, stream, out)

    @staticmethod
    def pack_plants(A, B, Bd):
        """[B, nx (nx+nu+ndu)]: per instance A_b | B_b | Bd_b, each column-major -- mpcx_lmpc_loop_desc.plant_batch; torch tensors in, a tensor out
        (what to copy_ into Loop.plants for the next run)"""
        import torch
        n = A.shape[0]
        return torch.cat([m.transpose(1, 2).reshape(n, m.shape[1] * m.shape[2]) for m in (A, B, Bd)], dim=1).contiguous()

    def _make_loop(self, x0, lastU, ticks, plant, plants, yref, uref, duref, dmeas, preview, noise, warm, stream, model=None,
                   observer=None, xhat0=None, meas_noise=None, bank=False, disturbance_observer=None, dhat0=None, checked=None, target=None):
        """the descriptor of a loop, its result tensors and the create call; model: a bank's model index (a device tensor) or None; checked:
        what _check_observers returned where the caller has run it already"""
        ticks = int(ticks)
        B = int(_shape(x0)[0])
        plants = self._check_plants(B, plant, plants)
        offset_free, per_instance_gain = checked or self._check_observers(B, ticks, observer, disturbance_observer, xhat0, dhat0, meas_noise, bank)
        per_instance_map = self._check_target(B, target, disturbance_observer, bank)
        torch, dev = self._torch()
        x0 = self._dev(torch, dev, x0, (B, self.nx))
        u0 = self._dev(torch, dev, lastU, (B, self.nu))
        refs = [self._loop_ref(torch, dev, a, B, n, ticks, preview)
                for a, n in ((yref, self.ny), (uref, self.nu), (duref, self.nu), (dmeas, self.ndu))]
        w = self._dev(torch, dev, noise, (ticks, B, self.nx))
        f64, i32 = torch.float64, torch.int32
        T = max(ticks, 0)
        res = ClosedLoopResult(
            x=torch.zeros((T + 1, B, self.nx), dtype=f64, device=dev), u=torch.zeros((T, B, self.nu), dtype=f64, device=dev),
            cost=torch.zeros((T, B), dtype=f64, device=dev), status=torch.zeros((T, B), dtype=i32, device=dev),
            solver_status=torch.zeros((T, B), dtype=i32, device=dev), iterations=torch.zeros((T, B), dtype=i32, device=dev),
            polish_rounds=torch.zeros((T, B), dtype=i32, device=dev), active_count=torch.zeros((T, B), dtype=i32, device=dev))

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        d = _capi.LoopDesc()
        d.batch, d.ticks = B, ticks
        mats, pb = [], None
        if plant is not None:
            plant = tuple(plant) + (None,) * (3 - len(plant))
            for name, m, cols in zip(("plant_A", "plant_B", "plant_Bd"), plant, (self.nx, self.nu, self.ndu)):
                if m is not None and cols > 0:
                    mats.append(_cm(m, self.nx, cols))
                    setattr(d, name, mats[-1].ctypes.data)
        if plants is not None:
            own = self._own_plant(B, model) if any(m is None for m in plants) else (None,) * 3
            full = [self._dev(torch, dev, m if isinstance(m, torch.Tensor) else np.array(o if m is None else m, dtype=np.float64), (B, self.nx, cols))
                    for m, o, cols in zip(plants, own, (self.nx, self.nu, self.ndu))]
            pb = self.pack_plants(*full)
            d.plant_batch = ptr(pb)
        d.x0, d.u0 = ptr(x0), ptr(u0)
        (yr, d.yref_mode), (ur, d.uref_mode), (dr, d.duref_mode), (de, d.dmeas_mode) = refs
        d.yref, d.uref, d.duref, d.dmeas = ptr(yr), ptr(ur), ptr(dr), ptr(de)
        d.noise = ptr(w)
        d.carry_working_set = int(bool(warm))
        d.traj_x, d.traj_u, d.traj_cost = ptr(res.x), ptr(res.u), ptr(res.cost)
        d.traj_status, d.traj_solver_status, d.traj_iterations = ptr(res.status), ptr(res.solver_status), ptr(res.iterations)
        d.traj_polish_rounds, d.traj_active_count = ptr(res.polish_rounds), ptr(res.active_count)
        od, gains, gain_h, xh, v, dh = None, None, None, None, None, None
        if offset_free:
            observer = disturbance_observer
        if observer is not None:
            od = _capi.DisturbanceObserverDesc() if offset_free else _capi.ObserverDesc()
            rows = self.nx + (self.ndu if offset_free else 0)
            if per_instance_gain:
                # not through _dev: its .contiguous() would copy what utils.kalman_gains / disturbance_gains return -- a view of this very
                # layout, which pack_gains then takes as it is (Loop.gains is in that case the caller's own tensor); the shape has been checked
                g = observer if isinstance(observer, torch.Tensor) else torch.as_tensor(np.asarray(observer, dtype=np.float64))
                gains = self.pack_gains(g.to(device=dev, dtype=torch.float64))
                od.gain_batch = ptr(gains)
            else:
                gain_h = _cm(observer.cpu().numpy() if isinstance(observer, torch.Tensor) else observer, rows, self.ny)
                od.gain = gain_h.ctypes.data
            xh = self._dev(torch, dev, xhat0, (B, self.nx))
            v = self._dev(torch, dev, meas_noise, (ticks, B, self.ny))
            res.xhat = torch.zeros((T + 1, B, self.nx), dtype=f64, device=dev)
            res.y = torch.zeros((T, B, self.ny), dtype=f64, device=dev)
            od.xhat0, od.meas_noise, od.traj_xhat, od.traj_y = ptr(xh), ptr(v), ptr(res.xhat), ptr(res.y)
            if offset_free:
                dh = self._dev(torch, dev, dhat0, (B, self.ndu))
                res.dhat = torch.zeros((T + 1, B, self.ndu), dtype=f64, device=dev)
                od.dhat0, od.traj_dhat = ptr(dh), ptr(res.dhat)
        td, maps, map_h = None, None, None
        if target is not None:
            td = _capi.TargetDesc()
            if per_instance_map:                # (not through _dev, as the gains: utils.target_maps' view is this very layout)
                t = target if isinstance(target, torch.Tensor) else torch.as_tensor(np.asarray(target, dtype=np.float64))
                maps = self.pack_gains(t.to(device=dev, dtype=torch.float64))
                td.map_batch = ptr(maps)
            else:
                map_h = _cm(target.cpu().numpy() if isinstance(target, torch.Tensor) else target, self.nu, self.ny + self.ndu + self.nu)
                td.map = map_h.ctypes.data
            res.us = torch.zeros((T + 1, B, self.nu), dtype=f64, device=dev)
            td.traj_us = ptr(res.us)
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else torch.cuda.Stream(device=dev)
        if s.cuda_stream == 0:
            raise ValueError("a loop is captured on a non-default stream")
        s.wait_stream(cur)                      # the tensors above were filled on the current stream
        h = C.c_void_p()
        check(self._create_loop(d, od, offset_free, td, bank, model, C.c_void_p(s.cuda_stream), C.byref(h)))
        cur.wait_stream(s)
        # keep: what the graph points at; [0], [1]: x0 and lastU as every run reads them
        return Loop(handle=h, result=res, ticks=ticks, keep=(x0, u0, yr, ur, dr, de, w, s, pb, gains, xh, v, dh, maps), plants=pb, gains=gains,
                    xhat0=xh, meas_noise=v, dhat0=dh, maps=maps)

    def run_loop(self, loop: Loop, stream=None) -> ClosedLoopResult:
        """One asynchronous run of a loop from its x0 / lastU tensors: `loop.result` is filled once the stream has been synchronised.  A loop
        uses the controller's one workspace, like `launch`: one launch or run of a controller in flight at a time."""
        torch, _ = self._torch()
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
        check(self._lib.mpcx_lmpc_loop_run(loop.handle, C.c_void_p(s.cuda_stream)))
        return loop.result

    def destroy_loop(self, loop: Loop):
        if loop.handle:
            check(self._lib.mpcx_lmpc_loop_destroy(loop.handle))
            loop.handle = None


class LMPC(_LoopFrontEnd):
    """Linear MPC controller whose optimize() runs on an MI355X.

    Mirrors mpc::LMPC<Tnx,Tnu,Tndu,Tny,Tph,Tch> with run-time sizes
    (the reference's MPC_DYNAMIC form, LMPC.hpp:57-62).  `device=-1` builds a
    host-only handle: setters and the condensing work, any solve raises.
    """

    def __init__(self, nx, nu, ndu, ny, ph, ch, device=0):
        self._lib = _capi.lib()
        self.nx, self.nu, self.ndu, self.ny, self.ph, self.ch = map(int, (nx, nu, ndu, ny, ph, ch))
        self.device = int(device)
        d = _capi.Dims(self.nx, self.nu, self.ndu, self.ny, self.ph, self.ch)
        self._h = C.c_void_p()
        check(self._lib.mpcx_lmpc_create(C.byref(d), self.device, C.byref(self._h)))
        self._A = self._B = None                                 # the model as given, for loops whose plants default to it
        self._Bd = np.zeros((self.nx, self.ndu))
        self._C, self._Dd = None, np.zeros((self.ny, self.ndu))               # the outputs as given: what an observed loop measures with
        self._has_terminal = False                               # a terminal cost is set (a bank takes it in every controller or in none)
        self._nlin = 0                                           # linear rows stored (setLinearConstraints)
        self._last = Result(cmd=np.zeros(self.nu))
        self._stats = SolutionStats()
        self._last_u0 = np.zeros(self.nu)
        self._seq = OptSequence(np.zeros((self.ph + 1, self.nx)), np.zeros((self.ph + 1, self.ny)),
                                np.zeros((self.ph + 1, self.nu)))

    def __del__(self):
        try:
            if self._h:
                self._lib.mpcx_lmpc_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- not available on the linear front-end (LMPC.hpp:68-100) -------------------
    def setDiscretizationSamplingTime(self, ts):
        raise RuntimeError("Linear MPC supports only discrete time systems")

    def setInputScale(self, scaling):
        raise RuntimeError("Linear MPC does not support input scaling")

    def setStateScale(self, scaling):
        raise RuntimeError("Linear MPC does not support state scaling")

    def setLoggerLevel(self, level):
        return True

    def setLoggerPrefix(self, prefix):
        return True

    # -- set-up ---------------------------------------------------------------------
    def _ok(self, rc):
        if rc == _capi.E_INVALID:
            return False          # the reference's setters return false on a bad slice
        check(rc)
        return True

    def setOptimizerParameters(self, params: LParams):
        check(self._lib.mpcx_lmpc_set_optimizer_parameters(self._h, C.byref(params)))
        self._warm_enabled = bool(params.enable_warm_start)
        self._warm_prev = None

    def setStrictInfeasibility(self, on=True):
        """extension: report infeasible QPs as INFEASIBLE / NaN instead of the reference's
        MAX_ITERATION + last iterate (see include/mpcx.h)"""
        check(self._lib.mpcx_lmpc_set_strict_infeasibility(self._h, int(bool(on))))

    def setStateSpaceModel(self, A, B, Cm):
        A, B, Cm = _cm(A, self.nx, self.nx), _cm(B, self.nx, self.nu), _cm(Cm, self.ny, self.nx)
        ok = self._ok(self._lib.mpcx_lmpc_set_state_space_model(self._h, _p(A), _p(B), _p(Cm)))
        if ok:
            self._A, self._B, self._C = A.copy(), B.copy(), Cm.copy()
        return ok

    def setDisturbances(self, Bd, Dd):
        Bd, Dd = _cm(Bd, self.nx, self.ndu), _cm(Dd, self.ny, self.ndu)
        ok = self._ok(self._lib.mpcx_lmpc_set_disturbances(self._h, _p(Bd), _p(Dd)))
        if ok:
            self._Bd, self._Dd = Bd.copy(), Dd.copy()
        return ok

    def setObjectiveWeights(self, OWeight, UWeight, DeltaUWeight, slice=None):
        ow = np.asarray(OWeight, dtype=np.float64)
        if ow.ndim == 2 and slice is None:
            O, U, D = _cm(OWeight, self.ny, self.ph), _cm(UWeight, self.nu, self.ph), _cm(DeltaUWeight, self.nu, self.ph)
            return self._ok(self._lib.mpcx_lmpc_set_objective_weights(self._h, _p(O), _p(U), _p(D)))
        s = _slice(slice)
        o, u, d = _vec(OWeight, self.ny), _vec(UWeight, self.nu), _vec(DeltaUWeight, self.nu)
        return self._ok(self._lib.mpcx_lmpc_set_objective_weights_slice(self._h, _p(o), _p(u), _p(d), s.start, s.end))

    def _bounds(self, lo, hi, rows, cols, fmat, fslice, slice):
        a = np.asarray(lo, dtype=np.float64)
        if a.ndim == 2 and slice is None:
            L, H = _cm(lo, rows, cols), _cm(hi, rows, cols)
            return self._ok(fmat(self._h, _p(L), _p(H)))
        s = _slice(slice)
        l, h = _vec(lo, rows), _vec(hi, rows)
        return self._ok(fslice(self._h, _p(l), _p(h), s.start, s.end))

    def setStateBounds(self, XMin, XMax, slice=None):
        return self._bounds(XMin, XMax, self.nx, self.ph, self._lib.mpcx_lmpc_set_state_bounds,
                            self._lib.mpcx_lmpc_set_state_bounds_slice, slice)

    def setInputBounds(self, UMin, UMax, slice=None):
        return self._bounds(UMin, UMax, self.nu, self.ch, self._lib.mpcx_lmpc_set_input_bounds,
                            self._lib.mpcx_lmpc_set_input_bounds_slice, slice)

    def setOutputBounds(self, YMin, YMax, slice=None):
        return self._bounds(YMin, YMax, self.ny, self.ph, self._lib.mpcx_lmpc_set_output_bounds,
                            self._lib.mpcx_lmpc_set_output_bounds_slice, slice)

    def setInputRateBounds(self, DUMin, DUMax, slice=None):
        """extension: dumin <= u_k - u_{k-1} <= dumax, the bounds of the reference QP's delta-u rows (ProblemBuilder.hpp:768-793; the
        reference has no setter).  [nu x ph] matrices, column i bounding delta_i = v_{i+1} - v_i with v_0 = lastU, or vectors with a
        prediction-horizon slice; columns past the control horizon are kept and not read."""
        return self._bounds(DUMin, DUMax, self.nu, self.ph, self._lib.mpcx_lmpc_set_input_rate_bounds,
                            self._lib.mpcx_lmpc_set_input_rate_bounds_slice, slice)

    def setSoftConstraintWeights(self, xw, yw, sw, slice=None):
        """extension: soft state / output / scalar rows.  A weight rho in (0, inf] per state component (xw[nx]), per output component
        (yw[ny]) and for the scalar row (sw); inf keeps the row hard, a finite weight replaces it by 0.5 rho dist^2(row value, [lo, hi]) in
        the cost.  None leaves that kind of row as it is.  Without a slice the whole horizon (steps 0 .. ph) is set; a slice works as
        setStateBounds' does, so that the weight lands on the rows the same slice bounds.  Input and input-rate bounds stay hard.
        False for NaN, zero or a negative weight and for a bad slice.  The reference's LMPC has no counterpart."""
        x = None if xw is None else _vec(np.broadcast_to(np.asarray(xw, dtype=np.float64), (self.nx,)) if np.ndim(xw) == 0 else xw, self.nx)
        y = None if yw is None else _vec(np.broadcast_to(np.asarray(yw, dtype=np.float64), (self.ny,)) if np.ndim(yw) == 0 else yw, self.ny)
        s = None if sw is None else _vec([float(sw)], 1)
        px, py, ps = (None if a is None else _p(a) for a in (x, y, s))
        if slice is None:
            return self._ok(self._lib.mpcx_lmpc_set_soft_constraint_weights(self._h, px, py, ps))
        sl = _slice(slice)
        return self._ok(self._lib.mpcx_lmpc_set_soft_constraint_weights_slice(self._h, px, py, ps, sl.start, sl.end))

    def setTerminalCost(self, P, xT=None, Tx=None):
        """extension: the terminal cost 0.5 (x_ph - x_T)' P (x_ph - x_T) with x_T = xT + Tx [yref(., ph - 1); dmeas(., ph - 1)].  P [nx x nx]
        symmetric positive semidefinite (lqr_terminal_cost gives the cost-to-go of the unconstrained problem), xT [nx] and Tx [nx x (ny + ndu)]
        default to zero; the columns of Tx are the first ny + ndu columns of target_map(want_x=True)'s map_x.  P = None removes the term.  The
        constant 0.5 x_T' P x_T is not part of `cost`.  False for NaN / inf, an asymmetric P or one with a negative eigenvalue (nothing is
        stored then).  The reference's LMPC has no counterpart."""
        if P is None:
            self._has_terminal = False
            return self._ok(self._lib.mpcx_lmpc_set_terminal_cost(self._h, None, None, None))
        Pm = _cm(P, self.nx, self.nx)
        x = None if xT is None else _vec(xT, self.nx)
        T = None if Tx is None else _cm(Tx, self.nx, self.ny + self.ndu)
        ok = self._ok(self._lib.mpcx_lmpc_set_terminal_cost(self._h, _p(Pm), None if x is None else _p(x), None if T is None else _p(T)))
        self._has_terminal = self._has_terminal or ok             # (a refused call stores nothing: what was there stays)
        return ok

    def setLinearConstraints(self, Fx, Fu, lo, hi, slice=None):
        """extension: nc linear rows lo[c, i] <= Fx[c, :] x_i + Fu[c, :] v_i <= hi[c, i] for the steps i = 0 .. ph, with v_i = u_{i-1} and
        v_0 = lastU -- the scalar row's convention for nc rows whose coefficients Fx [nc x nx], Fu [nc x nu] all steps share.  Without a
        slice lo and hi are [nc x (ph + 1)], column i bounding step i (a vector [nc] is taken for every step); with a slice they are vectors
        [nc] and the slice works as setScalarConstraint's does -- (ph - 1, ph) is a terminal set F x_ph <= g.  An infinite side is absent;
        Fx = None (or no rows) removes the rows.  False, with nothing stored, for NaN, an infinite coefficient, lo > hi, more than
        MPCX_MAX_LINEAR_ROWS rows, or a slice whose nc differs from the stored rows' while other steps hold bounds.  The reference's LMPC
        has no counterpart; the rows' active bits sit behind the reference's, at m_ref(reference) + i nc + c."""
        if Fx is None or np.asarray(Fx).size + np.asarray(Fu).size == 0:
            ok = self._ok(self._lib.mpcx_lmpc_set_linear_constraints(self._h, 0, None, None, None, None))
            self._nlin = 0 if ok else self._nlin
            return ok
        Fx = np.atleast_2d(np.asarray(Fx, dtype=np.float64))
        nc = Fx.shape[0]
        Fxm, Fum = _cm(Fx, nc, self.nx), _cm(np.atleast_2d(np.asarray(Fu, dtype=np.float64)), nc, self.nu)
        if slice is None:
            L, H = (np.asarray(a, dtype=np.float64) for a in (lo, hi))
            L, H = (np.repeat(a.reshape(nc, 1), self.ph + 1, axis=1) if a.ndim < 2 else a for a in (L, H))
            L, H = _cm(L, nc, self.ph + 1), _cm(H, nc, self.ph + 1)
            ok = self._ok(self._lib.mpcx_lmpc_set_linear_constraints(self._h, nc, _p(Fxm), _p(Fum), _p(L), _p(H)))
        else:
            sl = _slice(slice)
            L, H = _vec(lo, nc), _vec(hi, nc)
            ok = self._ok(self._lib.mpcx_lmpc_set_linear_constraints_slice(self._h, nc, _p(Fxm), _p(Fum), _p(L), _p(H), sl.start, sl.end))
        self._nlin = nc if ok else self._nlin                     # (a refused call stores nothing: what was there stays)
        return ok

    def setLinearConstraintWeights(self, w, slice=None):
        """extension: soft linear rows.  A weight rho in (0, inf] per row (w[nc], or one number for all), inf keeping the row hard, under
        the rules of setSoftConstraintWeights; without a slice the steps 0 .. ph, a slice as setLinearConstraints' does."""
        nc = self._nlin
        wv = _vec(np.broadcast_to(np.asarray(w, dtype=np.float64), (nc,)) if np.ndim(w) == 0 else w, nc)
        if slice is None:
            return self._ok(self._lib.mpcx_lmpc_set_linear_constraint_weights(self._h, _p(wv)))
        sl = _slice(slice)
        return self._ok(self._lib.mpcx_lmpc_set_linear_constraint_weights_slice(self._h, _p(wv), sl.start, sl.end))

    def _lqr_problem(self, step):
        """(A, B, Q, R) of the unconstrained problem whose cost-to-go is the terminal weight: the weights of user column `step`"""
        if self._A is None:
            raise MpcxError(_capi.E_STATE, "state-space model not set")
        if not 0 <= int(step) < self.ph:
            raise ValueError(f"step {step} is not a column of the weights, 0 .. {self.ph - 1}")
        # the weights as the handle stores them (user column k is internal column k + 1): one source of truth
        ow = self.debug_get("wOutput").reshape(self.ph + 1, self.ny)[int(step) + 1]
        r = self.debug_get("wU").reshape(self.ph + 1, self.nu)[int(step) + 1]
        if not (r > 0).all():
            raise ValueError("lqr_terminal_cost needs a positive input weight (UWeight) in every component: R = diag(UW[:, step]) must be positive definite")
        return self._A, self._B, self._C.T @ np.diag(ow) @ self._C, np.diag(r)

    def lqr_terminal_cost(self, step=1):
        """(P [nx, nx], K [nu, nx]): the cost-to-go and the gain u = -K x of the infinite-horizon problem with Q = C' diag(OW[:, step]) C and
        R = diag(UW[:, step]) -- the weights of user column `step` as the handle stores them -- through libmpc_amd.utils.lqr_gains (one
        mpcx_dare_batch call on the device).  setTerminalCost(P) then makes the horizon's cost the infinite one wherever no constraint is
        active behind it.  The weight on the input increments (DeltaUWeight) is ignored: with one, P is not the exact cost-to-go.  ValueError
        where an input weight is not positive; MpcxError where the equation was not solved."""
        from .utils import lqr_gains
        A, B, Q, R = self._lqr_problem(step)
        K, X, flags = lqr_gains(A, B, Q, R, device=max(self.device, 0))
        if int(flags[0]):
            why = {1: "R is not positive definite", 2: "the doubling iteration has not converged",
                   3: "the doubling iteration broke down: is (A, B) stabilisable?"}[int(flags[0])]
            raise MpcxError(_capi.E_NUMERIC, why)
        return X[0].cpu().numpy().copy(), K[0].cpu().numpy().copy()

    def setScalarConstraint(self, *args):
        """(min, max, X, U, slice) as LMPC.hpp:355 or (index, min, max, X, U) as LMPC.hpp:409."""
        if len(args) != 5:
            raise TypeError("setScalarConstraint takes (min, max, X, U, slice) or (index, min, max, X, U)")
        if isinstance(args[4], (HorizonSlice, tuple, list)) or args[4] is None:
            smin, smax, X, U, sl = args
            s = _slice(sl)
            X, U = _vec(X, self.nx), _vec(U, self.nu)
            return self._ok(self._lib.mpcx_lmpc_set_scalar_constraint_slice(
                self._h, float(smin), float(smax), _p(X), _p(U), s.start, s.end))
        index, smin, smax, X, U = args
        X, U = _vec(X, self.nx), _vec(U, self.nu)
        return self._ok(self._lib.mpcx_lmpc_set_scalar_constraint_index(
            self._h, int(index), float(smin), float(smax), _p(X), _p(U)))

    def setReferences(self, outRef, cmdRef, deltaCmdRef, slice=None):
        a = np.asarray(outRef, dtype=np.float64)
        if a.ndim == 2 and slice is None:
            Y, U, D = _cm(outRef, self.ny, self.ph), _cm(cmdRef, self.nu, self.ph), _cm(deltaCmdRef, self.nu, self.ph)
            return self._ok(self._lib.mpcx_lmpc_set_references(self._h, _p(Y), _p(U), _p(D)))
        s = _slice(slice)
        y, u, d = _vec(outRef, self.ny), _vec(cmdRef, self.nu), _vec(deltaCmdRef, self.nu)
        return self._ok(self._lib.mpcx_lmpc_set_references_slice(self._h, _p(y), _p(u), _p(d), s.start, s.end))

    def setExogenousInputs(self, uMeas, slice=None):
        a = np.asarray(uMeas, dtype=np.float64)
        if a.ndim == 2 and slice is None:
            Dm = _cm(uMeas, self.ndu, self.ph)
            return self._ok(self._lib.mpcx_lmpc_set_exogenous_inputs(self._h, _p(Dm)))
        s = _slice(slice)
        d = _vec(uMeas, self.ndu)
        return self._ok(self._lib.mpcx_lmpc_set_exogenous_inputs_slice(self._h, _p(d), s.start, s.end))

    # -- introspection -----------------------------------------------------------------
    def setup(self):
        check(self._lib.mpcx_lmpc_setup(self._h))

    def info(self):
        i = _capi.Info()
        check(self._lib.mpcx_lmpc_get_info(self._h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in _capi.Info._fields_}

    def debug_get(self, name):
        """testing aid: condensed arrays as computed by the host set-up"""
        f = self._lib.mpcx_lmpc_debug_get
        n = check(f(self._h, name.encode(), None, 0))
        out = np.zeros(n)
        check(f(self._h, name.encode(), _p(out), n))
        return out

    def setTotalBatch(self, total):
        """sharding: this controller is given contiguous shards of a batch of `total` instances (one rank of N); the kernel form is then chosen
        for the whole batch's size and a shard's results are bit for bit the rows of the unsharded solve (0: every call is a whole batch)"""
        check(self._lib.mpcx_lmpc_set_total_batch(self._h, int(total)))
        return True

    def debug_force_generic(self, on=True):
        """testing aid: route every batch through the generic (roll-out) assemble kernel"""
        check(self._lib.mpcx_lmpc_debug_force_generic(self._h, int(bool(on))))

    def debug_use_fused(self, on=True):
        """experiment / testing knob: False / 0 = assemble and solve as two kernels, True / 1 = the record computed inside the solve
        kernel by one mat-vec (persistent form from 1024 instances on), 2 = assemble + solve in one workgroup of sixteen
        wavefronts (lmpc_solve_group), -1 = automatic (the default: the workgroup form up to 4096 instances, two kernels beyond; the fused
        forms only on request)"""
        check(self._lib.mpcx_lmpc_debug_use_fused(self._h, -1 if on is None else int(on)))

    def make_batch(self, x0, u0, yref=None, uref=None, duref=None, dmeas=None,
                   want_active=False, want_sequence=False, warm=None, warm_shift=False):
        """Allocate outputs and fill the mpcx_lmpc_batch descriptor.  Returns (Batch, BatchResult, keepalive)."""
        torch, dev = self._torch()
        x0t = x0 if hasattr(x0, "shape") else np.asarray(x0)
        B = int(x0t.shape[0])
        x0 = self._dev(torch, dev, x0, (B, self.nx))
        u0 = self._dev(torch, dev, u0, (B, self.nu))
        yr, ym = self._ref(torch, dev, yref, B, self.ny)
        ur, um = self._ref(torch, dev, uref, B, self.nu)
        dr, dmo = self._ref(torch, dev, duref, B, self.nu)
        de, dem = self._ref(torch, dev, dmeas, B, self.ndu)
        i = self.info()
        f64, i32 = torch.float64, torch.int32
        res = BatchResult(
            cmd=torch.empty((B, self.nu), dtype=f64, device=dev),
            cost=torch.empty((B,), dtype=f64, device=dev),
            status=torch.empty((B,), dtype=i32, device=dev),
            solver_status=torch.empty((B,), dtype=i32, device=dev),
            is_feasible=torch.empty((B,), dtype=i32, device=dev),
            iterations=torch.empty((B,), dtype=i32, device=dev),
            polish_rounds=torch.zeros((B,), dtype=i32, device=dev),
            active_count=torch.zeros((B,), dtype=i32, device=dev))
        if want_active:
            res.active_lower = torch.zeros((B, i["active_words"]), dtype=i32, device=dev)
            res.active_upper = torch.zeros((B, i["active_words"]), dtype=i32, device=dev)
        if want_sequence:
            res.seq_state = torch.empty((B, self.ph + 1, self.nx), dtype=f64, device=dev)
            res.seq_output = torch.empty((B, self.ph + 1, self.ny), dtype=f64, device=dev)
            res.seq_input = torch.empty((B, self.ph + 1, self.nu), dtype=f64, device=dev)

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        b = _capi.Batch()
        b.batch = B
        b.x0, b.u0 = ptr(x0), ptr(u0)
        b.yref, b.yref_mode = ptr(yr), ym
        b.uref, b.uref_mode = ptr(ur), um
        b.duref, b.duref_mode = ptr(dr), dmo
        b.dmeas, b.dmeas_mode = ptr(de), dem
        b.cmd, b.cost = ptr(res.cmd), ptr(res.cost)
        b.status, b.solver_status = ptr(res.status), ptr(res.solver_status)
        b.is_feasible, b.iterations = ptr(res.is_feasible), ptr(res.iterations)
        b.active_lower, b.active_upper = ptr(res.active_lower), ptr(res.active_upper)
        b.seq_state, b.seq_output, b.seq_input = ptr(res.seq_state), ptr(res.seq_output), ptr(res.seq_input)
        b.polish_rounds, b.active_count = ptr(res.polish_rounds), ptr(res.active_count)
        wl = wu = None
        if warm is not None:                       # a previous BatchResult (with its active sets) or a (lower, upper) pair
            wl, wu = (warm.active_lower, warm.active_upper) if hasattr(warm, "active_lower") else warm
            if wl is None or wu is None:
                raise ValueError("warm start needs the previous solve's active sets (want_active=True)")
            wl = wl.to(dev).contiguous(); wu = wu.to(dev).contiguous()
            if tuple(wl.shape) != (B, i["active_words"]) or tuple(wu.shape) != (B, i["active_words"]):
                raise ValueError("warm-start active sets have the wrong shape")
            b.warm_active_lower, b.warm_active_upper = ptr(wl), ptr(wu)
            b.warm_shift = int(bool(warm_shift))
        keep = (x0, u0, yr, ur, dr, de, wl, wu)
        return b, res, keep

    def launch(self, batch, stream=None, keep=None):
        """One asynchronous kernel launch for a descriptor built by make_batch().

        A handle owns one workspace and one set of dispatch queues: keep ONE launch of a controller in flight at a time
        (launches on the same stream are ordered; for overlapping batches use one controller per stream, as bench.py
        does).  make_batch() fills its tensors on torch's current stream: a different launch stream first waits for it,
        and `keep` (the tensors the descriptor points at) is tied to the launch stream so that the caching allocator
        does not recycle them while the kernels still read them."""
        torch, _ = self._torch()
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
            for t in (keep or ()):
                if t is not None:
                    t.record_stream(s)
        check(self._lib.mpcx_lmpc_solve_batch(self._h, C.byref(batch), C.c_void_p(s.cuda_stream)))

    def make_graph(self, batch, stream):
        """One step as a HIP graph (mpcx_lmpc_graph_create): the launches of `launch(batch)` captured once on `stream` (a
        non-default torch stream) and replayed by `launch_graph`.  The descriptor's tensors stay where they are; write new
        inputs into them in place."""
        g = C.c_void_p()
        check(self._lib.mpcx_lmpc_graph_create(self._h, C.byref(batch), C.c_void_p(stream.cuda_stream), C.byref(g)))
        return g

    def launch_graph(self, graph, stream):
        check(self._lib.mpcx_lmpc_graph_launch(graph, C.c_void_p(stream.cuda_stream)))

    def destroy_graph(self, graph):
        check(self._lib.mpcx_lmpc_graph_destroy(graph))

    def target_map(self, want_x=False):
        """The steady-state target map [nu, ny+ndu+nu] = [Tr | Td | Tu] of the controller's own model and disturbance model: us = Tr r + Td dhat +
        Tu ubar is the input that holds the outputs on r against the disturbance dhat, as close to ubar as that allows -- what target= takes
        (libmpc_amd.utils.target_maps, one device call).  ValueError, before any device call, where a reference cannot be reached or an
        integrator is not seen by the outputs; MpcxError where the elimination met a vanishing pivot all the same.  want_x: (map_u, map_x
        [nx, ny+ndu+nu]) instead."""
        from .utils import target_maps
        if self._A is None:
            raise MpcxError(_capi.E_STATE, "state-space model not set")
        out = target_maps(self._A, self._B, self._Bd, self._C, self._Dd, want_x=want_x, device=max(self.device, 0))
        if int(out[-1][0]):
            raise MpcxError(_capi.E_NUMERIC, "the KKT system of the target is singular")
        maps = tuple(m[0].cpu().numpy().copy() for m in out[:-1])
        return maps if want_x else maps[0]

    def kalman_gain(self, Qw, Rv, want_P=False):
        """The steady-state Kalman predictor gain L [nx, ny] of the controller's own (A, C) for process-noise covariance Qw [nx, nx] and
        sensor-noise covariance Rv [ny, ny] (mpcx_lmpc_kalman_gain: Riccati iteration on the host; works on a host-only handle).
        want_P: (L, P, iterations) instead."""
        Q, R = _cm(Qw, self.nx, self.nx), _cm(Rv, self.ny, self.ny)
        L, P = np.zeros((self.nx, self.ny), order="F"), np.zeros((self.nx, self.nx), order="F")
        it = C.c_int(0)
        check(self._lib.mpcx_lmpc_kalman_gain(self._h, _p(Q), _p(R), _p(L), _p(P), C.byref(it)))
        return (L, P, it.value) if want_P else L

    def disturbance_gain(self, Qw, Qd, Rv, want_P=False):
        """The steady-state Kalman predictor gain [nx+ndu, ny] = [Lx; Ld] of the controller's model augmented with its integrating
        disturbance model, ([[A, Bd], [0, I]], [C, Dd]), for the covariances Qw [nx, nx] of the process noise, Qd [ndu, ndu] of the
        disturbance's random walk and Rv [ny, ny] of the sensor noise: what disturbance_observer= takes (libmpc_amd.utils.disturbance_gains,
        one device call).  ValueError, before any device call, where the augmented pair is not detectable; MpcxError where the equation was
        not solved.  want_P: (L, P) instead."""
        from .utils import disturbance_gains
        if self._A is None:
            raise MpcxError(_capi.E_STATE, "state-space model not set")
        L, P, flags = disturbance_gains(self._A, self._Bd, self._C, self._Dd, Qw, Qd, Rv, device=max(self.device, 0))
        if int(flags[0]):
            why = {1: "Rv is not positive definite", 2: "the doubling iteration has not converged",
                   3: "the doubling iteration broke down"}[int(flags[0])]
            raise MpcxError(_capi.E_NUMERIC, why)
        L, P = L[0].cpu().numpy().copy(), P[0].cpu().numpy().copy()
        return (L, P) if want_P else L

    def _own_plant(self, B, model=None):
        """the controller's own A, B, Bd for B instances (numpy, broadcast)"""
        if self._A is None:
            raise MpcxError(_capi.E_STATE, "state-space model not set")
        return tuple(np.broadcast_to(m, (B,) + m.shape) for m in (self._A, self._B, self._Bd))

    def make_loop(self, x0, lastU, ticks, plant=None, yref=None, uref=None, duref=None, dmeas=None, preview=False,
                  noise=None, warm=True, stream=None, plants=None, observer=None, xhat0=None, meas_noise=None,
                  disturbance_observer=None, dhat0=None, target=None) -> Loop:
        """A closed-loop run of `ticks` receding-horizon steps captured for `run_loop`: every tick is the batched solve followed by
        the plant step x <- A_p x + B_p cmd + Bd_p d_k + w_k on the device, with no host work in between.

        plant: None (the controller's own A, B, Bd) or (A_p, B_p) / (A_p, B_p, Bd_p), None entries meaning the controller's;
        plants: a plant per instance instead, (A [B,nx,nx], B [B,nx,nu] | None, Bd [B,nx,ndu] | None), None entries again the
        controller's -- packed into Loop.plants, which every run reads again (refill it in place: LMPC.pack_plants);
        noise: [ticks, B, nx] additive process disturbance the controller does not know about; warm: carry each tick's
        working set into the next tick's solve (tick 0 is cold); preview: 3-D references are [B, ticks+ph, n] windows.
        x0 / lastU are read again by every run_loop: tensors given here can be refilled in place (Loop.keep[0], [1]).

        observer: output feedback.  The solves then read an estimate xhat instead of the state: each tick measures y = C x + Dd d_k + v_k and
        updates xhat <- A xhat + B cmd + Bd d_k + L (y - C xhat - Dd d_k) with the controller's own model.  observer is the gain L, [nx, ny]
        for the batch (LMPC.kalman_gain) or [B, nx, ny] per instance (Loop.gains, refill with LMPC.pack_gains); xhat0: [B, nx], the first
        estimate (None: x0); meas_noise: [ticks, B, ny] sensor noise v_k.  The result's xhat and y are then filled, and x is the true state.

        disturbance_observer: offset-free tracking, exclusive with observer=.  The estimator carries [xhat; dhat] with the controller's own
        disturbance model (setDisturbances), dhat <- dhat + Ld e beside xhat <- A xhat + B cmd + Bd dhat + Lx e, and the solves read dhat as
        their exogenous input, constant along the horizon.  dmeas= is then the TRUE disturbance, in every layout it has: it drives the plant
        and the measurement and the controller never sees it (None: the controller's own exogenous input, zeros unless set).  The gain is
        [Lx; Ld], [nx+ndu, ny] for the batch (LMPC.disturbance_gain) or [B, nx+ndu, ny] per instance (utils.disturbance_gains' as it is);
        dhat0: [B, ndu], the first estimate (None: 0).  The result's dhat is filled as well.  Without target= the output settles on its reference only
        where the input weight is zero (or uref is the steady-state input).

        target: steady-state targets, with disturbance_observer= only.  The map [nu, ny+ndu+nu] for the batch (LMPC.target_map) or
        [B, nu, ny+ndu+nu] per instance (utils.target_maps' as it is; Loop.maps, refill with LMPC.pack_gains).  At every tick the loop
        computes us_k = T [r_k; dhat_k; ubar_k] -- r_k and ubar_k step 0 of the tick's yref and uref, in every layout they have -- and the
        solve reads us_k as its input reference, constant along the horizon: uref= is then ubar, what the input is held close to where the
        outputs leave it free.  yref reaches the solve unchanged.  us is not clipped to the input bounds (the result's us shows it)."""
        return self._make_loop(x0, lastU, ticks, plant, plants, yref, uref, duref, dmeas, preview, noise, warm, stream,
                               observer=observer, xhat0=xhat0, meas_noise=meas_noise, disturbance_observer=disturbance_observer, dhat0=dhat0,
                               target=target)

    def make_loop_gradient(self, loop: Loop, seed_x=None, seed_u=None, reduce=True, want=LOOP_GRADIENT_WANT, stream=None) -> LoopGradientResult:
        """The backward pass of a plain loop of this controller (make_loop without observer), captured for run_loop_gradient
        (mpcx_lmpc_loop_grad_create): the gradient of sum(seed_x * x) + sum(seed_u * u) of the loop's last run.  seed_x
        [ticks+1, B, nx], seed_u [ticks, B, nu] (one may be None) are read again by every run: refill result.seed_x / result.seed_u in place.
        want: which of LOOP_GRADIENT_WANT to compute -- without weights and model the backward ticks keep no sequences, without a model
        matrix they launch no model kernel.  reduce: plant, weights and model summed over the instances whose flag is 0 (in a fixed order)
        instead of a set per instance.  Destroy the gradient (destroy_loop_gradient) before its loop."""
        torch, dev = self._torch()
        unknown = set(want) - set(LOOP_GRADIENT_WANT)
        if unknown:
            raise ValueError(f"want: unknown outputs {sorted(unknown)}")
        T, B = loop.ticks, int(loop.result.x.shape[1])
        sx = self._dev(torch, dev, seed_x, (T + 1, B, self.nx))
        su = self._dev(torch, dev, seed_u, (T, B, self.nu))
        if sx is None and su is None:
            raise ValueError("a loop gradient needs seed_x or seed_u")
        f64 = torch.float64
        lead = () if reduce else (B,)
        new = lambda name, shape: torch.zeros(shape, dtype=f64, device=dev) if (name in want and all(n > 0 for n in shape)) else None
        # (matrices are written column-major, as their setters read them: allocated [columns, rows], handed out transposed)
        mat = lambda name, rows, cols: new(name, lead + (cols, rows))
        tr = lambda t: None if t is None else t.transpose(-1, -2)
        npl = self.nx + self.nu + self.ndu
        plant = new("plant", lead + (npl, self.nx))
        ow, uw, dw = mat("oweight", self.ny, self.ph), mat("uweight", self.nu, self.ph), mat("duweight", self.nu, self.ph)
        gA, gB, gC = mat("A", self.nx, self.nx), mat("B", self.nx, self.nu), mat("C", self.ny, self.nx)
        gBd, gDd = mat("Bd", self.nx, self.ndu), mat("Dd", self.ny, self.ndu)
        out = LoopGradientResult(
            d_x0=new("x0", (B, self.nx)), d_u0=new("u0", (B, self.nu)), d_yref=new("yref", (B, self.ny)), d_noise=new("noise", (T, B, self.nx)),
            d_oweight=tr(ow), d_uweight=tr(uw), d_duweight=tr(dw), d_A=tr(gA), d_B=tr(gB), d_C=tr(gC), d_Bd=tr(gBd), d_Dd=tr(gDd),
            flags=torch.zeros((B,), dtype=torch.int32, device=dev), n_used=torch.zeros((1,), dtype=torch.int32, device=dev) if reduce else None,
            seed_x=sx, seed_u=su)
        if plant is not None:
            pt = tr(plant)
            out.d_plant_A, out.d_plant_B = pt[..., :self.nx], pt[..., self.nx:self.nx + self.nu]
            out.d_plant_Bd = pt[..., self.nx + self.nu:] if self.ndu > 0 else None

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())
        d = _capi.LoopGradDesc()
        d.seed_x, d.seed_u, d.reduce = ptr(sx), ptr(su), int(bool(reduce))
        d.d_x0, d.d_u0, d.d_yref, d.d_noise, d.d_plant = ptr(out.d_x0), ptr(out.d_u0), ptr(out.d_yref), ptr(out.d_noise), ptr(plant)
        d.d_oweight, d.d_uweight, d.d_duweight = ptr(ow), ptr(uw), ptr(dw)
        d.d_A, d.d_B, d.d_C, d.d_Bd, d.d_Dd = ptr(gA), ptr(gB), ptr(gC), ptr(gBd), ptr(gDd)
        d.flags, d.n_used = ptr(out.flags), ptr(out.n_used)
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else torch.cuda.Stream(device=dev)
        if s.cuda_stream == 0:
            raise ValueError("a loop gradient is captured on a non-default stream")
        s.wait_stream(cur)
        h = C.c_void_p()
        check(self._lib.mpcx_lmpc_loop_grad_create(loop.handle, C.byref(d), C.c_void_p(s.cuda_stream), C.byref(h)))
        s.synchronize()
        out.handle = h
        out.keep = (loop, sx, su, plant, ow, uw, dw, gA, gB, gC, gBd, gDd, s)
        return out

    def run_loop_gradient(self, gradient: LoopGradientResult, stream=None) -> LoopGradientResult:
        """One asynchronous backward pass over the last completed run of the gradient's loop: `ticks` graph replays between a begin and a
        finish kernel; the result's tensors are filled once the stream has been synchronised.  Streams and the one-launch-in-flight rule as
        for run_loop."""
        torch, _ = self._torch()
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
        check(self._lib.mpcx_lmpc_loop_grad_run(gradient.handle, C.c_void_p(s.cuda_stream)))
        return gradient

    def destroy_loop_gradient(self, gradient: LoopGradientResult):
        if gradient.handle:
            check(self._lib.mpcx_lmpc_loop_grad_destroy(gradient.handle))
            gradient.handle = None

    def simulate(self, x0, lastU, ticks, plant=None, yref=None, uref=None, duref=None, dmeas=None, preview=False,
                 noise=None, warm=True, stream=None, plants=None, observer=None, xhat0=None, meas_noise=None,
                 disturbance_observer=None, dhat0=None, target=None, gradient=None) -> ClosedLoopResult:
        """make_loop + run_loop + destroy_loop: one closed-loop run, synchronised.  gradient: dict(seed_x=, seed_u=, want=, reduce=) -- the
        backward pass of that run as well (make_loop_gradient's arguments), returned as result.gradient."""
        loop = self.make_loop(x0, lastU, ticks, plant, yref, uref, duref, dmeas, preview, noise, warm, plants=plants,
                              observer=observer, xhat0=xhat0, meas_noise=meas_noise, disturbance_observer=disturbance_observer, dhat0=dhat0,
                              target=target)
        torch, _ = self._torch()
        grad = None
        try:
            if gradient is not None:
                grad = self.make_loop_gradient(loop, **gradient)
            self.run_loop(loop, stream)
            if grad is not None:
                self.run_loop_gradient(grad, stream)
                loop.result.gradient = grad
            (stream if stream is not None else torch.cuda.current_stream(self.device)).synchronize()
        finally:
            if grad is not None:
                self.destroy_loop_gradient(grad)
            self.destroy_loop(loop)
        return loop.result

    def time_launches(self, batch, repeats, stream=None):
        """Mean kernel time (ms) over `repeats` launches, HIP events on the launch stream."""
        torch, _ = self._torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        ms = C.c_float()
        check(self._lib.mpcx_lmpc_time_solve_batch(self._h, C.byref(batch), C.c_void_p(s.cuda_stream), int(repeats), C.byref(ms)))
        return ms.value

    def optimizeBatch(self, x0, lastU, yref=None, uref=None, duref=None, dmeas=None,
                      want_active=False, want_sequence=False, stream=None, warm=None, warm_shift=False, sensitivities=False) -> BatchResult:
        """B independent LOptimizer::run calls (LOptimizer.hpp:189) in one launch.  `warm`: the BatchResult of the
        previous control tick (solved with want_active=True) -- its active sets seed the working sets; warm_shift=True
        looks each row up one horizon step later (receding horizon).  sensitivities=True: the Jacobians of cmd on the active
        sets this solve wrote, as `result.sensitivities` (one more launch on the same stream)."""
        b, res, keep = self.make_batch(x0, lastU, yref, uref, duref, dmeas, want_active or sensitivities or warm is not None, want_sequence, warm, warm_shift)
        self.launch(b, stream, keep)
        res._inputs = keep                     # the inputs live as long as the result that was computed from them
        res._batch = b                         # ... and the descriptor: paramSensitivityBatch differentiates the batch it describes
        if sensitivities:
            res.sensitivities = self.sensitivityBatch(res.active_lower, res.active_upper, status=res.status, stream=stream)
        return res

    def make_sensitivity(self, active_lower, active_upper, status=None, seed_cmd=None, seed_input=None, want=("x0", "u0", "yref")):
        """Allocate outputs and fill the mpcx_lmpc_sens descriptor.  Returns (Sens, SensitivityResult, keepalive)."""
        torch, dev = self._torch()
        words = self.info()["active_words"]
        al = active_lower.to(dev).contiguous(); au = active_upper.to(dev).contiguous()
        B = int(al.shape[0])
        if tuple(al.shape) != (B, words) or tuple(au.shape) != (B, words) or al.dtype != torch.int32 or au.dtype != torch.int32:
            raise ValueError(f"active sets must be int32 [B, {words}]")
        st = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
        if st is not None and tuple(st.shape) != (B,):
            raise ValueError("status must be [B]")
        sc = self._dev(torch, dev, seed_cmd, (B, self.nu))
        si = self._dev(torch, dev, seed_input, (B, self.ph + 1, self.nu))
        jac = sc is None and si is None
        lead = (B, self.nu) if jac else (B,)
        f64 = torch.float64
        out = SensitivityResult(
            d_x0=torch.empty(lead + (self.nx,), dtype=f64, device=dev) if "x0" in want else None,
            d_u0=torch.empty(lead + (self.nu,), dtype=f64, device=dev) if "u0" in want else None,
            d_yref=torch.empty(lead + (self.ny,), dtype=f64, device=dev) if "yref" in want else None,
            flags=torch.empty((B,), dtype=torch.int32, device=dev))

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())
        d = _capi.Sens()
        d.batch = B
        d.active_lower, d.active_upper, d.status = ptr(al), ptr(au), ptr(st)
        d.mode = _capi.SENS_JACOBIAN if jac else _capi.SENS_VJP
        d.seed_cmd, d.seed_input = ptr(sc), ptr(si)
        d.d_x0, d.d_u0, d.d_yref, d.flags = ptr(out.d_x0), ptr(out.d_u0), ptr(out.d_yref), ptr(out.flags)
        return d, out, (al, au, st, sc, si, out.d_x0, out.d_u0, out.d_yref, out.flags)

    def launch_sensitivity(self, desc, stream=None, keep=None):
        """One asynchronous launch for a descriptor built by make_sensitivity(); streams as in launch()."""
        torch, _ = self._torch()
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
            for t in (keep or ()):
                if t is not None:
                    t.record_stream(s)
        check(self._lib.mpcx_lmpc_sensitivity_batch(self._h, C.byref(desc), C.c_void_p(s.cuda_stream)))

    def sensitivityBatch(self, active_lower, active_upper, status=None, seed_cmd=None, seed_input=None, stream=None,
                         want=("x0", "u0", "yref")) -> SensitivityResult:
        """The slope of solved instances on their active sets (mpcx_lmpc_sensitivity_batch): one launch.  active_lower / active_upper
        [B, active_words] as optimizeBatch(want_active=True) wrote them; status [B] (optional) marks the instances that were not
        solved.  Without seeds: the Jacobians of cmd.  seed_cmd [B, nu] and / or seed_input [B, ph + 1, nu] (a cotangent on the input
        sequence as the solve writes it: row 0 is cmd): the vector-Jacobian products.  want: which outputs to compute."""
        d, out, keep = self.make_sensitivity(active_lower, active_upper, status, seed_cmd, seed_input, want)
        self.launch_sensitivity(d, stream, keep)
        out._inputs = keep[:5]
        return out

    def make_param_sensitivity(self, solved, seed_cmd=None, seed_input=None, reduce=False,
                               want=("oweight", "uweight", "duweight", "lower", "upper")):
        """Allocate outputs and fill the mpcx_lmpc_param_sens descriptor for `solved`: a BatchResult of optimizeBatch(..., want_active=True,
        want_sequence=True), or the Batch descriptor of make_batch (whose tensors the caller keeps alive).  With reduce the handle's partial
        sums are sized here, so that the launch allocates nothing.  Returns (ParamSens, ParamSensitivityResult, keepalive)."""
        torch, dev = self._torch()
        b = getattr(solved, "_batch", solved)
        if not isinstance(b, _capi.Batch):
            raise ValueError("paramSensitivityBatch needs the result of optimizeBatch(want_active=True, want_sequence=True) or a Batch descriptor")
        if not (b.active_lower and b.active_upper and b.seq_output and b.seq_input):
            raise ValueError("the batch must have been solved with want_active=True and want_sequence=True")
        B = int(b.batch)
        sc = self._dev(torch, dev, seed_cmd, (B, self.nu))
        si = self._dev(torch, dev, seed_input, (B, self.ph + 1, self.nu))
        if sc is None and si is None:
            raise ValueError("a parameter sensitivity needs seed_cmd or seed_input")
        m = self.info()["m_ref"]
        lead = () if reduce else (B,)
        f64 = torch.float64
        # (the kernel writes each weight matrix column-major, as the setter reads it: allocated [ph, rows], handed out transposed)
        mat = lambda rows, name: torch.empty(lead + (self.ph, rows), dtype=f64, device=dev) if name in want else None
        ow, uw, dw = mat(self.ny, "oweight"), mat(self.nu, "uweight"), mat(self.nu, "duweight")
        lo = torch.empty(lead + (m,), dtype=f64, device=dev) if "lower" in want else None
        up = torch.empty(lead + (m,), dtype=f64, device=dev) if "upper" in want else None
        flags = torch.empty((B,), dtype=torch.int32, device=dev)
        n_used = torch.zeros((1,), dtype=torch.int32, device=dev) if reduce else None
        tr = lambda t: None if t is None else t.transpose(-1, -2)
        out = ParamSensitivityResult(tr(ow), tr(uw), tr(dw), lo, up, flags, n_used)
        if reduce:
            check(self._lib.mpcx_lmpc_param_sens_reserve(self._h, B))

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())
        d = _capi.ParamSens()
        d.solved = C.cast(C.pointer(b), C.c_void_p)
        d.seed_cmd, d.seed_input, d.reduce = ptr(sc), ptr(si), int(bool(reduce))
        d.d_oweight, d.d_uweight, d.d_duweight, d.d_lower, d.d_upper = ptr(ow), ptr(uw), ptr(dw), ptr(lo), ptr(up)
        d.flags, d.n_used = ptr(flags), ptr(n_used)
        return d, out, (b, solved, sc, si, ow, uw, dw, lo, up, flags, n_used)

    def launch_param_sensitivity(self, desc, stream=None, keep=None):
        """One asynchronous launch (two kernels with reduce) for a descriptor built by make_param_sensitivity(); streams as in launch()."""
        torch, _ = self._torch()
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
            for t in (keep or ()):
                if isinstance(t, torch.Tensor):
                    t.record_stream(s)
        check(self._lib.mpcx_lmpc_param_sensitivity_batch(self._h, C.byref(desc), C.c_void_p(s.cuda_stream)))

    def paramSensitivityBatch(self, solved, seed_cmd=None, seed_input=None, reduce=False, stream=None,
                              want=("oweight", "uweight", "duweight", "lower", "upper")) -> ParamSensitivityResult:
        """The gradient of sum(seed_cmd * cmd) + sum(seed_input * input sequence) of a solved batch with respect to OWeight, UWeight,
        DeltaUWeight and to every bound of the QP (mpcx_lmpc_param_sensitivity_batch): one launch after the solve, on each instance's
        active set.  solved: the result of optimizeBatch(..., want_active=True, want_sequence=True) of this controller, unchanged since.
        reduce: the sum over the batch (in a fixed order: the same bits every time) instead of one set per instance.  Bounds come in the
        row numbering of the active sets (info()["m_ref"] rows)."""
        d, out, keep = self.make_param_sensitivity(solved, seed_cmd, seed_input, reduce, want)
        self.launch_param_sensitivity(d, stream, keep)
        out._inputs = keep[:4]
        return out

    def make_model_sensitivity(self, solved, seed_cmd=None, seed_input=None, reduce=False, want=("A", "B", "C", "Bd", "Dd")):
        """Allocate outputs and fill the mpcx_lmpc_model_sens descriptor for `solved`: a BatchResult of optimizeBatch(..., want_active=True,
        want_sequence=True), or the Batch descriptor of make_batch (whose tensors the caller keeps alive).  The kernel's operand and, with
        reduce, the handle's partial sums are sized here, so that the launch allocates nothing.  Returns (ModelSens, ModelSensitivityResult,
        keepalive)."""
        torch, dev = self._torch()
        b = getattr(solved, "_batch", solved)
        if not isinstance(b, _capi.Batch):
            raise ValueError("modelSensitivityBatch needs the result of optimizeBatch(want_active=True, want_sequence=True) or a Batch descriptor")
        if not (b.active_lower and b.active_upper and b.seq_state and b.seq_output and b.seq_input):
            raise ValueError("the batch must have been solved with want_active=True and want_sequence=True")
        B = int(b.batch)
        sc = self._dev(torch, dev, seed_cmd, (B, self.nu))
        si = self._dev(torch, dev, seed_input, (B, self.ph + 1, self.nu))
        if sc is None and si is None:
            raise ValueError("a model sensitivity needs seed_cmd or seed_input")
        lead = () if reduce else (B,)
        f64 = torch.float64
        # (the kernel writes each matrix column-major, as the setter reads it: allocated [columns, rows], handed out transposed)
        mat = lambda rows, cols, name: torch.empty(lead + (cols, rows), dtype=f64, device=dev) if (name in want and rows * cols > 0) else None
        gA, gB, gC = mat(self.nx, self.nx, "A"), mat(self.nx, self.nu, "B"), mat(self.ny, self.nx, "C")
        gBd, gDd = mat(self.nx, self.ndu, "Bd"), mat(self.ny, self.ndu, "Dd")
        flags = torch.empty((B,), dtype=torch.int32, device=dev)
        n_used = torch.zeros((1,), dtype=torch.int32, device=dev) if reduce else None
        tr = lambda t: None if t is None else t.transpose(-1, -2)
        out = ModelSensitivityResult(tr(gA), tr(gB), tr(gC), tr(gBd), tr(gDd), flags, n_used)
        check(self._lib.mpcx_lmpc_model_sens_reserve(self._h, B if reduce else 0))

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())
        d = _capi.ModelSens()
        d.solved = C.cast(C.pointer(b), C.c_void_p)
        d.seed_cmd, d.seed_input, d.reduce = ptr(sc), ptr(si), int(bool(reduce))
        d.d_A, d.d_B, d.d_C, d.d_Bd, d.d_Dd = ptr(gA), ptr(gB), ptr(gC), ptr(gBd), ptr(gDd)
        d.flags, d.n_used = ptr(flags), ptr(n_used)
        return d, out, (b, solved, sc, si, gA, gB, gC, gBd, gDd, flags, n_used)

    def launch_model_sensitivity(self, desc, stream=None, keep=None):
        """One asynchronous launch (two kernels with reduce) for a descriptor built by make_model_sensitivity(); streams as in launch()."""
        torch, _ = self._torch()
        cur = torch.cuda.current_stream(self.device)
        s = stream if stream is not None else cur
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)
            for t in (keep or ()):
                if isinstance(t, torch.Tensor):
                    t.record_stream(s)
        check(self._lib.mpcx_lmpc_model_sensitivity_batch(self._h, C.byref(desc), C.c_void_p(s.cuda_stream)))

    def modelSensitivityBatch(self, solved, seed_cmd=None, seed_input=None, reduce=False, stream=None,
                              want=("A", "B", "C", "Bd", "Dd")) -> ModelSensitivityResult:
        """The gradient of sum(seed_cmd * cmd) + sum(seed_input * input sequence) of a solved batch with respect to every entry of A, B, C, Bd
        and Dd (mpcx_lmpc_model_sensitivity_batch): one launch after the solve, on each instance's active set.  solved: the result of
        optimizeBatch(..., want_active=True, want_sequence=True) of this controller, unchanged since.  reduce: the sum over the batch (in a
        fixed order: the same bits every time) instead of one set per instance."""
        d, out, keep = self.make_model_sensitivity(solved, seed_cmd, seed_input, reduce, want)
        self.launch_model_sensitivity(d, stream, keep)
        out._inputs = keep[:4]
        return out

    def optimize(self, x0, lastU) -> Result:
        """IMPC::optimize (IMPC.hpp:149-166) for one instance, through the batched path."""
        import time
        t_start = time.perf_counter()
        self._last_u0 = np.asarray(lastU, dtype=np.float64).reshape(self.nu).copy()
        warm = getattr(self, "_warm_prev", None) if getattr(self, "_warm_enabled", False) else None
        r = self.optimizeBatch(np.asarray(x0, dtype=np.float64).reshape(1, self.nx),
                               np.asarray(lastU, dtype=np.float64).reshape(1, self.nu), want_sequence=True,
                               want_active=getattr(self, "_warm_enabled", False), warm=warm)
        if getattr(self, "_warm_enabled", False):
            self._warm_prev = r                   # LOptimizer keeps optimal_prev_x / _y (LOptimizer.hpp:295-296, 372)
        sst = int(r.solver_status[0].item())
        self._last = Result(solver_status=sst, is_feasible=bool(r.is_feasible[0].item()), solver_status_msg="",
                            cost=float(r.cost[0].item()), status=int(r.status[0].item()),
                            cmd=r.cmd[0].cpu().numpy().copy())
        self._seq = OptSequence(r.seq_state[0].cpu().numpy().copy(), r.seq_output[0].cpu().numpy().copy(),
                                r.seq_input[0].cpu().numpy().copy())
        self._stats.add(time.perf_counter() - t_start, self._last.status)
        return self._last

    def getLastResult(self) -> Result:
        return self._last

    def getOptimalSequence(self) -> OptSequence:
        return self._seq

    # ---- the rest of the pybind module's LMPC surface (python/pybind_export.cpp:93-123) --------------------------
    def getExecutionStats(self) -> "SolutionStats":
        """IMPC::getExecutionStats (IMPC.hpp:201-204, Profiler.hpp): wall time of the optimize() calls made so far."""
        return self._stats

    def resetStats(self):
        self._stats = SolutionStats()

    def getSolverWarmStartDual(self):
        """LMPC::getSolverWarmStartDual (LMPC.hpp:697-700) returns OSQP's dual vector; what this engine carries between
        ticks is the active set, so the vector holds -1 / 0 / +1 per reference row (lower / inactive / upper): the
        sign pattern of OSQP's y."""
        r = getattr(self, "_warm_prev", None)
        i = self.info()
        y = np.zeros(i["m_ref"])
        if r is not None:
            al, au = (r.active_lower, r.active_upper) if hasattr(r, "active_lower") else r
            lo = al[0].cpu().numpy().view(np.uint32); hi = au[0].cpu().numpy().view(np.uint32)
            for k in range(i["m_ref"]):
                if (lo[k >> 5] >> (k & 31)) & 1:
                    y[k] = -1.0
                elif (hi[k >> 5] >> (k & 31)) & 1:
                    y[k] = 1.0
        return y

    def getSolverWarmStartPrimal(self):
        """LMPC::getSolverWarmStartPrimal (LMPC.hpp:677-680): the reference QP's primal vector [xi_0..xi_ph | du_0..du_ph-1]
        (ProblemBuilder.hpp:70-76), rebuilt from the last optimal sequence."""
        seq = self._seq
        ph, nx, nu = self.ph, self.nx, self.nu
        v = np.vstack([self._last_u0[None, :], seq.input[:ph]])              # v_i = u_{i-1}
        xi = np.hstack([seq.state, v])
        du = np.diff(v, axis=0)
        return np.concatenate([xi.reshape(-1), du.reshape(-1)])

    def setSolverWarmStart(self, warm_primal, warm_dual):
        """LMPC::setSolverWarmStart (LMPC.hpp:716-722): only the sign pattern of the dual is used (see above)."""
        import torch
        i = self.info()
        y = np.asarray(warm_dual, dtype=np.float64).reshape(-1)
        if y.size != i["m_ref"]:
            raise ValueError("dual vector must have one entry per reference constraint row")
        lo = np.zeros(i["active_words"], dtype=np.uint32); hi = np.zeros(i["active_words"], dtype=np.uint32)
        for k in np.nonzero(y)[0]:
            (lo if y[k] < 0 else hi)[k >> 5] |= np.uint32(1 << (k & 31))
        dev = torch.device("cuda", self.device)
        self._warm_prev = (torch.from_numpy(lo.view(np.int32)[None, :]).to(dev), torch.from_numpy(hi.view(np.int32)[None, :]).to(dev))
