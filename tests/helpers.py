"""Shared test helpers: drive the CPU oracle and the product with the same reference-style calls."""
import math

import numpy as np

from oracle.lmpc_oracle import OracleLMPC, default_params

INF = float("inf")


class OracleFrontEnd:
    """The reference's LMPC front-end logic (include/mpc/LMPC.hpp) on top of the C oracle:
    {-1,-1} slices go through the matrix setters, other slices through the per-index setters,
    exactly as LMPC.hpp:153-292,436-481,596-660 do.  Lets a test issue the same calls to the
    oracle and to libmpc_amd.LMPC."""

    def __init__(self, nx, nu, ndu, ny, ph, ch):
        self.nx, self.nu, self.ndu, self.ny, self.ph, self.ch = nx, nu, ndu, ny, ph, ch
        self.o = OracleLMPC(nx, nu, ndu, ny, ph, ch)
        self.yRef = np.zeros((ny, ph)); self.uRef = np.zeros((nu, ph)); self.duRef = np.zeros((nu, ph))
        self.dMeas = np.zeros((ndu, ph))

    @staticmethod
    def _unset(s):
        return s is None or tuple(s) == (-1, -1)

    def _pred_ok(self, s):
        a, b = s
        return not (a >= b or a > self.ph or b > self.ph or a < 0)

    def _ctrl_ok(self, s):
        a, b = s
        return not (a >= b or a > self.ch or b > self.ch or a < 0)

    def setStateSpaceModel(self, A, B, C):
        return bool(self.o.set_model(A, B, C))

    def setDisturbances(self, Bd, Dd):
        return bool(self.o.set_exogenous(np.asarray(Bd, float).reshape(self.nx, self.ndu),
                                         np.asarray(Dd, float).reshape(self.ny, self.ndu)))

    def setOptimizerParameters(self, **kw):
        self.o.params = default_params(**kw)

    def setObjectiveWeights(self, ow, uw, duw, slice=None):
        ow = np.asarray(ow, float)
        if ow.ndim == 2 and slice is None:
            return bool(self.o.set_objective(ow, uw, duw))
        if self._unset(slice):
            rep = lambda v: np.tile(np.asarray(v, float).reshape(-1, 1), (1, self.ph))
            return bool(self.o.set_objective(rep(ow), rep(uw), rep(duw)))
        if not self._pred_ok(slice):
            return False
        for i in range(slice[0], slice[1]):
            self.o.set_objective_idx(i, ow, uw, duw)
        return True

    def _bounds(self, lo, hi, cols, fmat, fidx, ok, slice):
        lo = np.asarray(lo, float)
        if lo.ndim == 2 and slice is None:
            return bool(fmat(lo, hi))
        if self._unset(slice):
            rep = lambda v: np.tile(np.asarray(v, float).reshape(-1, 1), (1, cols))
            return bool(fmat(rep(lo), rep(hi)))
        if not ok(slice):
            return False
        for i in range(slice[0], slice[1]):
            fidx(i, lo, hi)
        return True

    def setStateBounds(self, lo, hi, slice=None):
        return self._bounds(lo, hi, self.ph, self.o.set_state_bounds, self.o.set_state_bounds_idx, self._pred_ok, slice)

    def setInputBounds(self, lo, hi, slice=None):
        return self._bounds(lo, hi, self.ch, self.o.set_input_bounds, self.o.set_input_bounds_idx, self._ctrl_ok, slice)

    def setOutputBounds(self, lo, hi, slice=None):
        return self._bounds(lo, hi, self.ph, self.o.set_output_bounds, self.o.set_output_bounds_idx, self._pred_ok, slice)

    def setScalarConstraint(self, *args):
        if isinstance(args[4], (tuple, list)) or args[4] is None:
            smin, smax, X, U, sl = args
            if self._unset(sl):
                return bool(self.o.set_scalar(np.full(self.ph, smin), np.full(self.ph, smax), X, U))
            if not self._pred_ok(sl):
                return False
            for i in range(sl[0], sl[1]):
                self.o.set_scalar_idx(i, smin, smax, X, U)
            return True
        index, smin, smax, X, U = args
        if index >= self.ph:
            return False
        self.o.set_scalar_idx(index, smin, smax, X, U)
        return True

    def setReferences(self, y, u, du, slice=None):
        y = np.asarray(y, float)
        if y.ndim == 2 and slice is None:
            self.yRef[:] = y; self.uRef[:] = u; self.duRef[:] = du
            return True
        s = (0, self.ph) if self._unset(slice) else slice
        if not self._pred_ok(s):
            return False
        for i in range(s[0], s[1]):
            self.yRef[:, i] = y; self.uRef[:, i] = u; self.duRef[:, i] = du
        return True

    def setExogenousInputs(self, d, slice=None):
        d = np.asarray(d, float)
        if d.ndim == 2 and slice is None:
            self.dMeas[:] = d
            return True
        s = (0, self.ph) if self._unset(slice) else slice
        if not self._unset(slice) and not self._ctrl_ok(s):       # LMPC.hpp:571: control-horizon validity
            return False
        for i in range(s[0], s[1]):
            self.dMeas[:, i] = d
        return True

    def optimize(self, x0, u0, yRef=None, uRef=None, duRef=None, dMeas=None):
        """one cold-start LOptimizer::run; optional per-solve overrides of the references"""
        yR = self.yRef if yRef is None else yRef
        uR = self.uRef if uRef is None else uRef
        dR = self.duRef if duRef is None else duRef
        dM = self.dMeas if dMeas is None else dMeas
        return self.o.solve(x0, u0, yR, uR, dR, dM)


def configure_quadrotor(c, ph, ch=None):
    """examples/quadrotor_ex.cpp:52-93 through reference-style calls (works on both front-ends)."""
    from oracle.lmpc_numpy import quadrotor_model
    ch = ph if ch is None else ch
    Ad, Bd, Cd = quadrotor_model()
    assert c.setStateSpaceModel(Ad, Bd, Cd)
    assert c.setObjectiveWeights([0, 0, 10, 10, 10, 10, 0, 0, 0, 5, 5, 5], [0.1] * 4, [0] * 4, (0, ph))
    xmin = [-math.pi / 6, -math.pi / 6, -INF, -INF, -INF, -1] + [-INF] * 6
    xmax = [math.pi / 6, math.pi / 6] + [INF] * 10
    assert c.setStateBounds(xmin, xmax, (0, ph))
    assert c.setOutputBounds([-INF] * 12, [INF] * 12, (0, ph))
    assert c.setInputBounds([9.6 - 10.5916] * 4, [13 - 10.5916] * 4, (0, ch))
    yref = np.zeros(12); yref[2] = 1.0
    assert c.setReferences(yref, np.zeros(4), np.zeros(4), (0, ph))
    return c


def quadrotor_oracle(ph, ch=None, maximum_iteration=250):
    """the quadrotor controller on the raw C oracle (for batch drivers)"""
    f = OracleFrontEnd(12, 4, 4, 12, ph, ph if ch is None else ch)
    configure_quadrotor(f, ph, ch)
    f.o.params = default_params(maximum_iteration=maximum_iteration)
    return f.o


def random_lmpc_spec(seed, nx=3, nu=2, ndu=1, ny=2, ph=6, ch=3):
    """A small controller exercising every LMPC feature: disturbances, per-step weights, state /
    input / output bounds on slices, a scalar constraint, move blocking (ch < ph), references."""
    r = np.random.default_rng(seed)
    A = r.normal(size=(nx, nx)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
    spec = dict(dims=(nx, nu, ndu, ny, ph, ch), A=A, B=r.normal(size=(nx, nu)), C=r.normal(size=(ny, nx)),
                Bd=0.3 * r.normal(size=(nx, ndu)), Dd=0.2 * r.normal(size=(ny, ndu)),
                OW=r.uniform(0.5, 2.0, size=(ny, ph)), UW=r.uniform(0.05, 0.2, size=(nu, ph)),
                DUW=r.uniform(0.0, 0.1, size=(nu, ph)),
                umin=-0.6 * np.ones(nu), umax=0.7 * np.ones(nu),
                xmin=np.array([-2.0] + [-INF] * (nx - 1)), xmax=np.array([2.0] + [INF] * (nx - 1)),
                ymin=np.full(ny, -3.0), ymax=np.full(ny, 3.0),
                sX=r.normal(size=nx), sU=r.normal(size=nu), smin=-4.0, smax=4.0,
                yref=r.normal(size=(ny, ph)), uref=0.05 * r.normal(size=(nu, ph)), duref=0.01 * r.normal(size=(nu, ph)),
                dmeas=0.2 * r.normal(size=(ndu, ph)))
    return spec


def configure_random(c, spec):
    nx, nu, ndu, ny, ph, ch = spec["dims"]
    assert c.setStateSpaceModel(spec["A"], spec["B"], spec["C"])
    assert c.setDisturbances(spec["Bd"], spec["Dd"])
    assert c.setObjectiveWeights(spec["OW"], spec["UW"], spec["DUW"])
    assert c.setInputBounds(spec["umin"], spec["umax"], None)
    assert c.setStateBounds(spec["xmin"], spec["xmax"], (1, ph))
    assert c.setOutputBounds(spec["ymin"], spec["ymax"], (0, ph - 1))
    assert c.setScalarConstraint(spec["smin"], spec["smax"], spec["sX"], spec["sU"], (1, ph))
    assert c.setReferences(spec["yref"], spec["uref"], spec["duref"])
    assert c.setExogenousInputs(spec["dmeas"])
    return c


def bits_to_rows(words, m):
    """[B, W] int32 bitmap words -> list of sorted row-index arrays"""
    w = np.ascontiguousarray(np.asarray(words)).astype(np.uint32)
    out = []
    for b in range(w.shape[0]):
        bits = np.unpackbits(w[b].view(np.uint8), bitorder="little")[:m]
        out.append(np.nonzero(bits)[0])
    return out


def rel_err(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def oracle_batch_parallel(ph, x0, u0, yref, want_active=False, workers=None, **kw):
    """solve_batch_constref of the C oracle over a thread pool (ctypes releases the GIL during the call; one oracle handle per
    thread): the whole benchmark batch in seconds instead of a sample of it"""
    import os
    from concurrent.futures import ThreadPoolExecutor
    B = len(x0)
    workers = workers or max(1, min(16, (os.cpu_count() or 1)))
    bounds = np.linspace(0, B, workers + 1).astype(int)
    def job(k):
        lo, hi = bounds[k], bounds[k + 1]
        if hi <= lo:
            return None
        return quadrotor_oracle(ph, **kw).solve_batch_constref(x0[lo:hi], u0[lo:hi], yref[lo:hi], want_active=want_active)
    with ThreadPoolExecutor(workers) as ex:
        parts = [r for r in ex.map(job, range(workers)) if r is not None]
    out = {}
    for k in parts[0]:
        if parts[0][k] is None or np.isscalar(parts[0][k]):
            out[k] = parts[0][k]
        else:
            out[k] = np.concatenate([p_[k] for p_ in parts])
    return out


def assert_matches_oracle(r, ref, o_neq, o_ncon, rtol_cmd=1e-5, rtol_cost=1e-7, check_active=True):
    """GPU batch result against oracle results: cmd, cost on the instances the oracle polished, active sets bit for bit there,
    loose on the others (the reference returns an eps = 1e-4 ADMM iterate there, the GPU the exact optimum); returns the number
    of unpolished instances"""
    cmd = r.cmd.cpu().numpy(); cost = r.cost.cpu().numpy(); st = r.status.cpu().numpy()
    pol = ref["polished"] == 1
    assert np.array_equal(st[ref["status"] == 0], np.zeros((ref["status"] == 0).sum(), dtype=st.dtype))
    scale = np.maximum(np.abs(ref["cmd"]).max(axis=1), 1e-12)
    err = np.abs(cmd - ref["cmd"]).max(axis=1) / scale
    assert err[pol].max() <= rtol_cmd, (err[pol].max(), int(np.argmax(err * pol)))
    if (~pol).any():
        assert err[~pol].max() <= 5e-2
    cerr = np.abs(cost - ref["cost"]) / np.maximum(1.0, np.abs(ref["cost"]))
    assert cerr[pol].max() <= rtol_cost, cerr[pol].max()
    if check_active:
        wl = np.ascontiguousarray(r.active_lower.cpu().numpy()).astype(np.uint32); wu = np.ascontiguousarray(r.active_upper.cpu().numpy()).astype(np.uint32)
        bl = np.unpackbits(wl.view(np.uint8).reshape(len(wl), -1), axis=1, bitorder="little")[:, :o_ncon]
        bu = np.unpackbits(wu.view(np.uint8).reshape(len(wu), -1), axis=1, bitorder="little")[:, :o_ncon]
        rl = (ref["active_lower"] != 0).astype(np.uint8); ru = (ref["active_upper"] != 0).astype(np.uint8)
        same = (bl[:, o_neq:] == rl[:, o_neq:]).all(axis=1) & (bu[:, o_neq:] == ru[:, o_neq:]).all(axis=1)
        assert same[pol].all(), int(np.argmin(same | ~pol))
    return int((~pol).sum())


# ---------------------------------------------------------------------------------------------
# a family of controllers whose optima have large active sets (working sets past the lean kernels' 16 rows)
# ---------------------------------------------------------------------------------------------
def axes_spec(nax, ph, ch=None, vmax=0.8, umax=1.0, seed=0, perturb=0.0, ny_mode="eye", extra_states=0, zero_weight=False):
    """`nax` double-integrator axes (position, velocity; dt = 0.1), one input each: inputs in +-umax over the control horizon,
    velocities in +-vmax at every step, output weights 10 on positions and 1 on velocities, input weight 0.01, delta-u weight 0.1.
    perturb: relative spread of the limits and weights drawn from `seed` (one controller of a heterogeneous bank).
    ny_mode: "eye" (C = I), "select" (C picks the positions and the first velocity: ny < nx), "mix" (C = I plus nax rows
    position + velocity of each axis: ny > nx; those outputs carry bounds too).  extra_states: states with no bounds, a stable
    mode driven by the first position.  zero_weight: no input and delta-u weight and none on the last step's outputs -- the last
    input then does not enter the cost and the condensed Hessian is singular (the set-up regularises it)."""
    ch = ph if ch is None else ch
    r = np.random.default_rng(seed)
    jit = lambda n: 1.0 + perturb * r.uniform(-1.0, 1.0, size=n)
    dt = 0.1
    n2 = 2 * nax
    nx, nu = n2 + extra_states, nax
    A = np.eye(nx); B = np.zeros((nx, nu))
    for a in range(nax):
        A[2 * a, 2 * a + 1] = dt
        B[2 * a, a] = 0.5 * dt * dt; B[2 * a + 1, a] = dt
    for e in range(extra_states):
        A[n2 + e, n2 + e] = 0.9 - 0.1 * e
        A[n2 + e, 0] = 0.05
    wpos = 10.0 * jit(nax); wvel = 1.0 * jit(nax)
    ow_state = np.zeros(nx); ow_state[0:n2:2] = wpos; ow_state[1:n2:2] = wvel
    if ny_mode == "eye":
        Cm = np.eye(nx); OW = ow_state.copy()
    elif ny_mode == "select":
        rows = list(range(0, n2, 2)) + [1]
        Cm = np.eye(nx)[rows]; OW = ow_state[rows]
    elif ny_mode == "mix":
        mix = np.zeros((nax, nx))
        for a in range(nax):
            mix[a, 2 * a] = 1.0; mix[a, 2 * a + 1] = 0.5
        Cm = np.vstack([np.eye(nx), mix]); OW = np.concatenate([ow_state, np.full(nax, 0.5)])
    else:
        raise ValueError(ny_mode)
    ny = Cm.shape[0]
    OW = np.tile(OW[:, None], (1, ph))
    UW = np.full((nu, ph), 0.01) * jit(nu)[:, None]
    DUW = np.full((nu, ph), 0.1) * jit(nu)[:, None]
    if zero_weight:
        UW[:] = 0.0; DUW[:] = 0.0; OW[:, -1] = 0.0
    um = umax * jit(nu); vm = vmax * jit(nax)
    xmin = np.full(nx, -INF); xmax = np.full(nx, INF)
    xmin[1:n2:2] = -vm; xmax[1:n2:2] = vm
    ymin = np.full(ny, -INF); ymax = np.full(ny, INF)
    if ny_mode == "mix":
        ymin[nx:] = -4.0; ymax[nx:] = 4.0
    return dict(dims=(nx, nu, 0, ny, ph, ch), A=A, B=B, C=Cm, OW=OW, UW=UW, DUW=DUW,
                umin=-um, umax=um, xmin=xmin, xmax=xmax, ymin=ymin, ymax=ymax, nax=nax)


def configure_axes(c, spec, maximum_iteration=4000):
    """the controller of `spec` through reference-style calls (LMPC or OracleFrontEnd); references zero"""
    from oracle.lmpc_oracle import default_params
    nx, nu, ndu, ny, ph, ch = spec["dims"]
    assert c.setStateSpaceModel(spec["A"], spec["B"], spec["C"])
    assert c.setObjectiveWeights(spec["OW"], spec["UW"], spec["DUW"])
    assert c.setInputBounds(spec["umin"], spec["umax"], (0, ch))
    assert c.setStateBounds(spec["xmin"], spec["xmax"], (0, ph))
    assert c.setOutputBounds(spec["ymin"], spec["ymax"], (0, ph))
    assert c.setReferences(np.zeros(ny), np.zeros(nu), np.zeros(nu), (0, ph))
    if isinstance(c, OracleFrontEnd):
        c.o.params = default_params(maximum_iteration=maximum_iteration)
    else:
        from libmpc_amd import LParameters
        c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration))
    return c


def axes_oracle(spec, maximum_iteration=4000):
    return configure_axes(OracleFrontEnd(*spec["dims"]), spec, maximum_iteration).o


def axes_batch(spec, B, seed=2024):
    """x0: positions U(-s, s) with s ~ U(0, 3) per instance, velocities U(-0.5, 0.5), extra states U(-0.5, 0.5);
    lastU U(-0.5, 0.5) inside the input box; yref [B, ny] zero (the references of the set-up)"""
    nx, nu, ndu, ny, ph, ch = spec["dims"]
    nax = spec["nax"]
    r = np.random.default_rng(seed)
    s = r.uniform(0.0, 3.0, size=(B, 1))
    x0 = r.uniform(-0.5, 0.5, size=(B, nx))
    x0[:, 0:2 * nax:2] = s * r.uniform(-1.0, 1.0, size=(B, nax))
    u0 = r.uniform(-0.5, 0.5, size=(B, nu)) * np.minimum(1.0, np.abs(spec["umax"]))[None, :]
    return np.ascontiguousarray(x0), np.ascontiguousarray(u0), np.zeros((B, ny))


def oracle_batch_parallel_spec(spec, x0, u0, yref=None, maximum_iteration=4000, workers=None):
    """oracle_batch_parallel for any axes_spec controller: one cold oracle solve per instance over a thread pool, active bitmaps
    included, plus 'n_active' (active inequality rows per instance) and 'violation': how far the oracle's sequence lies outside
    the bounds.  Active rows are those with a nonzero multiplier; a row the oracle flags at its bound with a multiplier of exactly
    zero (a degenerate optimum: it may or may not be in an optimal working set) is kept in 'active_*_flagged' and counted in
    'n_flagged' only.  OSQP accepts a polished point whose residuals are no worse than the ADMM iterate's, so now and then a 'polished'
    point misses an active row and crosses that bound by up to ADMM accuracy; such a point is not the exact optimum the kernels
    are held to, and 'polished' is cleared there ('polished_raw' keeps the oracle's flag)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    nx, nu, ndu, ny, ph, ch = spec["dims"]
    B = len(x0)
    yref = np.zeros((B, ny)) if yref is None else yref
    workers = workers or max(1, min(16, (os.cpu_count() or 1)))
    bounds = np.linspace(0, B, workers + 1).astype(int)
    umax = np.abs(spec["umax"]); xlo, xhi, ylo, yhi = spec["xmin"], spec["xmax"], spec["ymin"], spec["ymax"]
    zu, zd = np.zeros((nu, ph)), np.zeros((max(ndu, 0), ph))

    def job(k):
        o = axes_oracle(spec, maximum_iteration)
        out = []
        for b in range(bounds[k], bounds[k + 1]):
            r = o.solve(x0[b], u0[b], np.tile(yref[b][:, None], (1, ph)), zu, zu, zd)
            st, inp, outp = r["state"], r["input"], r["output"]
            # (input rows checked without move blocking only: with ch < ph the bound columns map onto blocks of steps)
            v = max(np.max(np.abs(inp[:ch]) - umax[None, :], initial=0.0) if ch == ph else 0.0,
                    np.max(np.maximum(xlo[None, :] - st[1:], st[1:] - xhi[None, :]), initial=0.0),
                    np.max(np.maximum(ylo[None, :] - outp[1:], outp[1:] - yhi[None, :]), initial=0.0))
            out.append((b, r, max(v, 0.0)))
        return out
    with ThreadPoolExecutor(workers) as ex:
        parts = [x for p_ in ex.map(job, range(workers)) for x in p_]
    o = axes_oracle(spec, maximum_iteration)
    res = {"neq": o.neq, "ncon": o.ncon, "nvar": o.nvar}
    res["cmd"] = np.zeros((B, nu)); res["cost"] = np.zeros(B); res["violation"] = np.zeros(B)
    for k in ("status", "solver_status", "iters", "polished"):
        res[k] = np.zeros(B, dtype=np.int32)
    for k in ("active_lower", "active_upper", "active_lower_flagged", "active_upper_flagged"):
        res[k] = np.zeros((B, o.ncon), dtype=np.uint8)
    for b, r, v in parts:
        res["cmd"][b] = r["cmd"]; res["cost"][b] = r["cost"]; res["violation"][b] = v
        for k in ("status", "solver_status", "iters", "polished"):
            res[k][b] = r[k]
        res["active_lower"][b] = r["active_lower"] & (r["y"] != 0); res["active_upper"][b] = r["active_upper"] & (r["y"] != 0)
        res["active_lower_flagged"][b] = r["active_lower"]; res["active_upper_flagged"][b] = r["active_upper"]
    # the box rows of step 0 bound the initial state and lastU, which are given, not decided: the condensed problem has no such rows and
    # the kernels never report them, while OSQP, once x0 sits on a bound (closed loop), splits a multiplier between such a row and the
    # initial-condition equality
    na = nx + nu
    for k in ("active_lower", "active_upper", "active_lower_flagged", "active_upper_flagged"):
        res[k][:, o.neq:o.neq + na] = 0
    res["polished_raw"] = res["polished"].copy()
    res["polished"][res["violation"] > 1e-7] = 0
    res["n_active"] = ((res["active_lower"][:, o.neq:] != 0) | (res["active_upper"][:, o.neq:] != 0)).sum(axis=1)
    res["n_flagged"] = ((res["active_lower_flagged"][:, o.neq:] != 0) | (res["active_upper_flagged"][:, o.neq:] != 0)).sum(axis=1)
    return res


# the workloads of tests/test_lmpc_shapes*.py
SHAPES_MAXIT = 4000
SHAPES_MAIN = (3, 20, 1024)               # nax, ph, batch: working sets of 0 to ~60 rows, spread evenly
# name -> (axes_spec arguments, kernel template variant, cost_direct)
SHAPES_VARIANTS = {
    "v1": (dict(nax=3, ph=20), 1, 0),                          # nz = 60
    "v1_zero_weight": (dict(nax=3, ph=20, zero_weight=True), 1, 1),
    "v2": (dict(nax=3, ph=50), 2, 0),                          # nz = 150
    "v4": (dict(nax=6, ph=50), 4, 0),                          # nz = 300
    "ldg": (dict(nax=2, ph=40, ny_mode="mix"), 2, 0),          # nz = 80, 160 bounded rows
}
SHAPES_EDGES = {
    "nu1": dict(nax=1, ph=20),
    "nu3": dict(nax=3, ph=10),
    "nu5": dict(nax=5, ph=8),
    "nx3": dict(nax=1, ph=20, extra_states=1),
    "ny_lt_nx": dict(nax=3, ph=12, ny_mode="select"),
    "ny_gt_nx": dict(nax=2, ph=15, ny_mode="mix"),
    "ch_lt_ph": dict(nax=3, ph=20, ch=8),
    "nz47": dict(nax=1, ph=47),
    "nz48": dict(nax=1, ph=48),
    "nz49": dict(nax=1, ph=49),
    "kin72": dict(nax=2, ph=6, extra_states=28),               # nx = ny = 32, nu = 2
}
