"""Reference for the input-rate bounds: the reference QP itself (oracle.lmpc_numpy.ProblemBuilderRef) with its delta-u rows made
finite, solved by the numpy restatement of OSQP.  ProblemBuilder.hpp:768-793 builds ph*nu inequality rows on the delta-u variables
with bounds +-inf for steps i <= ch and 0 behind the control horizon; the reference has no setter for the free ones, so this module
overwrites lineq / uineq at off_du after build().  Also: an independent numpy condensing of those rows for the host tests.

A controller is described by a `spec` dict (rate_spec / integrator_spec) and applied with the same calls to libmpc_amd.LMPC
(configure) and to the numpy builder (builder)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import lmpc_numpy as LN
from oracle import osqp_numpy as OSQP

INF = float("inf")
MAXIT = 4000            # helpers.SHAPES_MAXIT


def rate_spec(seed, nx, nu, ndu, ny, ph, ch, rate=0.1, box=None, state=False, output=False, scalar=False, vary=False):
    """A random stable controller with input-rate bounds.  rate: the bound's size; vary: bounds that differ per step and per
    component, every third (step + component) one-sided.  box: input box +-box over the control horizon; state / output / scalar:
    a state bound, output bounds and the scalar row as in helpers.random_lmpc_spec."""
    r = np.random.default_rng(seed)
    A = r.normal(size=(nx, nx)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
    sp = dict(dims=(nx, nu, ndu, ny, ph, ch), A=A, B=r.normal(size=(nx, nu)), C=r.normal(size=(ny, nx)),
              OW=r.uniform(0.5, 2.0, size=(ny, ph)), UW=r.uniform(0.05, 0.2, size=(nu, ph)), DUW=r.uniform(0.0, 0.1, size=(nu, ph)),
              yref=r.normal(size=(ny, ph)), uref=np.zeros((nu, ph)), duref=np.zeros((nu, ph)))
    if ndu:
        sp.update(Bd=0.3 * r.normal(size=(nx, ndu)), Dd=0.2 * r.normal(size=(ny, ndu)), dmeas=0.2 * r.normal(size=(ndu, ph)))
    lo = np.full((nu, ph), -rate); hi = np.full((nu, ph), rate)
    if vary:
        lo *= r.uniform(0.5, 1.5, size=(nu, ph)); hi *= r.uniform(0.5, 1.5, size=(nu, ph))
        for i in range(ph):
            for j in range(nu):
                if (i + j) % 3 == 1:
                    lo[j, i] = -INF
                elif (i + j) % 3 == 2 and (i + j) % 2 == 0:
                    hi[j, i] = INF
    sp.update(dumin=lo, dumax=hi)
    if box is not None:
        sp.update(umin=-box * np.ones(nu), umax=box * np.ones(nu))
    if state:
        sp.update(xmin=np.array([-2.0] + [-INF] * (nx - 1)), xmax=np.array([2.0] + [INF] * (nx - 1)))
    if output:
        sp.update(ymin=np.full(ny, -3.0), ymax=np.full(ny, 3.0))
    if scalar:
        sp.update(sX=r.normal(size=nx), sU=r.normal(size=nu), smin=-4.0, smax=4.0)
    return sp


def integrator_spec(ph=10, rate=0.1, box=1.0, yref=1.0):
    """a double integrator (position, velocity; dt = 0.1), the position as output, a step reference"""
    dt = 0.1
    sp = dict(dims=(2, 1, 0, 1, ph, ph), A=np.array([[1.0, dt], [0.0, 1.0]]), B=np.array([[0.5 * dt * dt], [dt]]), C=np.array([[1.0, 0.0]]),
              OW=np.full((1, ph), 10.0), UW=np.full((1, ph), 0.01), DUW=np.full((1, ph), 0.1),
              yref=np.full((1, ph), yref), uref=np.zeros((1, ph)), duref=np.zeros((1, ph)))
    if box is not None:
        sp.update(umin=-box * np.ones(1), umax=box * np.ones(1))
    if rate is not None:
        sp.update(dumin=np.full((1, ph), -rate), dumax=np.full((1, ph), rate))
    return sp


def full_feature_spec():
    """(4, 2, 1, 2, 10, 10) with Bd, Dd: input box, a state bound, output bounds, the scalar row and rate bounds that differ per step and
    component, tight enough that all four kinds of row are active together; the state, output and scalar rows start at step 1, so that
    no instance is infeasible by its data alone"""
    sp = rate_spec(300, 4, 2, 1, 2, 10, 10, rate=0.15, vary=True, box=0.5, state=True, output=True, scalar=True)
    sp["xmin"][0] = -1.0; sp["xmax"][0] = 1.0; sp["ymin"][:] = -1.2; sp["ymax"][:] = 1.2; sp["smin"] = -1.0; sp["smax"] = 1.0
    sp["first"] = 1
    return sp


def full_feature_batch(B=24):
    """x0, u0, per-step yref [B, ny, ph], per-instance dmeas [B, ndu, ph]"""
    r = np.random.default_rng(11)
    return 0.3 * r.normal(size=(B, 4)), r.uniform(-0.2, 0.2, size=(B, 2)), 1.5 * r.normal(size=(B, 2, 10)), 0.2 * r.normal(size=(B, 1, 10))


LARGE_DIMS = (2, 4, 0, 1, 40, 40)       # 160 rate rows: the two-chunk kernel variant


def large_case(B=8):
    """the case whose oracle solves take a second each: its results are recorded (tests/golden/make_rate_bounds_golden.py)"""
    sp = rate_spec(401, *LARGE_DIMS, rate=0.1)
    r = np.random.default_rng(13)
    return sp, r.normal(size=(B, 2)), r.uniform(-0.3, 0.3, size=(B, 4)), 1.2 * r.normal(size=(B, 1))


def random_batch(sp, B, seed, yscale=None):
    """x0 ~ N(0, 1), lastU ~ U(-0.3, 0.3), yref None (the controller's) or [B, ny] ~ yscale N(0, 1)"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    r = np.random.default_rng(seed)
    x0 = r.normal(size=(B, nx)); u0 = r.uniform(-0.3, 0.3, size=(B, nu))
    return x0, u0, (None if yscale is None else yscale * r.normal(size=(B, ny)))


def without_rate(sp):
    return {k: v for k, v in sp.items() if k not in ("dumin", "dumax")}


def configure(c, sp, maximum_iteration=MAXIT, rate=True):
    """the controller of `sp` on a libmpc_amd.LMPC; rate=False: everything but the rate bounds"""
    from libmpc_amd import LParameters
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    assert c.setStateSpaceModel(sp["A"], sp["B"], sp["C"])
    if "Bd" in sp:
        assert c.setDisturbances(sp["Bd"], sp["Dd"])
        assert c.setExogenousInputs(sp["dmeas"])
    assert c.setObjectiveWeights(sp["OW"], sp["UW"], sp["DUW"])
    if "umin" in sp:
        assert c.setInputBounds(sp["umin"], sp["umax"], (sp.get("box_first", 0), ch))     # (column 0 of the box bounds lastU itself)
    first = sp.get("first", 0)                 # the first bounded step of the state / output / scalar rows
    if "xmin" in sp:
        assert c.setStateBounds(sp["xmin"], sp["xmax"], (first, ph))
    if "ymin" in sp:
        assert c.setOutputBounds(sp["ymin"], sp["ymax"], (first, ph))
    if "sX" in sp:
        assert c.setScalarConstraint(sp["smin"], sp["smax"], sp["sX"], sp["sU"], (first, ph))
    assert c.setReferences(sp["yref"], sp["uref"], sp["duref"])
    if rate and "dumin" in sp:
        assert c.setInputRateBounds(sp["dumin"], sp["dumax"])
    c.setOptimizerParameters(LParameters(maximum_iteration=maximum_iteration))
    return c


def builder(sp):
    """the reference's builder after the same calls, built, with the delta-u rows of the steps i <= ch overwritten"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    pb = LN.ProblemBuilderRef(nx, nu, ndu, ny, ph, ch)
    pb.set_state_model(sp["A"], sp["B"], sp["C"])
    if "Bd" in sp:
        pb.set_exogenous(sp["Bd"], sp["Dd"])
    pb.set_objective_mat(sp["OW"], sp["UW"], sp["DUW"])
    for i in range(sp.get("box_first", 0), ch if "umin" in sp else 0):
        pb.set_input_bounds_idx(i, sp["umin"], sp["umax"])
    for i in range(sp.get("first", 0), ph):
        if "xmin" in sp:
            pb.set_state_bounds_idx(i, sp["xmin"], sp["xmax"])
        if "ymin" in sp:
            pb.set_output_bounds_idx(i, sp["ymin"], sp["ymax"])
        if "sX" in sp:
            pb.set_scalar_idx(i, sp["smin"], sp["smax"], sp["sX"], sp["sU"])
    pb.build()
    d = pb.d
    if "dumin" in sp:
        for i in range(min(ph, ch + 1)):
            for j in range(nu):
                pb.lineq[d.off_du + i * nu + j] = sp["dumin"][j, i]
                pb.uineq[d.off_du + i * nu + j] = sp["dumax"][j, i]
    return pb


def _result_status(s):
    """LOptimizer.hpp:386-415"""
    return {OSQP.OSQP_SOLVED: 0, OSQP.OSQP_MAX_ITER_REACHED: 1, OSQP.OSQP_PRIMAL_INFEASIBLE: 2, OSQP.OSQP_DUAL_INFEASIBLE: 2,
            OSQP.OSQP_SOLVED_INACCURATE: 0, OSQP.OSQP_PRIMAL_INFEASIBLE_INACCURATE: 0, OSQP.OSQP_DUAL_INFEASIBLE_INACCURATE: 0,
            OSQP.OSQP_NON_CVX: 3}.get(s, 4)


def solve_one(pb, sp, x0, u0, yref=None, dmeas=None, maximum_iteration=MAXIT):
    """one cold LOptimizer::run of the reference QP; yref [ny] (constant along the horizon) or [ny, ph], dmeas [ndu, ph]"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = pb.d
    yR = sp["yref"] if yref is None else (np.tile(np.asarray(yref, float)[:, None], (1, ph)) if np.ndim(yref) == 1 else np.asarray(yref, float))
    dM = (sp.get("dmeas", np.zeros((ndu, ph))) if dmeas is None else np.asarray(dmeas, float))
    q, l, u = pb.get(np.asarray(x0, float), np.asarray(u0, float), yR, sp["uref"], sp["duref"], dM)
    r = OSQP.solve(pb.P, q, pb.A, l, u, OSQP.Settings(max_iter=maximum_iteration))
    C = pb.ssC[:ny, :nx]; Dd = pb.ssDv[:ny, :]
    state, out, inp = LN.unpack_solution(d, r["x"], C, Dd, dM)
    st = r["status"]
    # OSQP accepts a polished point whose residuals are no worse than the ADMM iterate's; now and then its guess of the active set holds a
    # row too many, and the "polished" point is feasible with a multiplier of the wrong sign on that row: not a KKT point, not the optimum
    # (a tighter ADMM run finds a lower cost).  As helpers.oracle_batch_parallel_spec does for points outside the bounds, 'polished' is
    # cleared there ('polished_raw' keeps the oracle's flag).
    yi = r["y"][d.neq:]
    wrong = max(np.max(yi[np.asarray(r["active_lower"], bool)[d.neq:]], initial=0.0), np.max(-yi[np.asarray(r["active_upper"], bool)[d.neq:]], initial=0.0))
    polished = int(r["polished"]) if wrong <= 1e-9 * max(1.0, np.abs(yi).max(initial=0.0)) else 0
    al = np.asarray(r["active_lower"], bool) & (r["y"] != 0); au = np.asarray(r["active_upper"], bool) & (r["y"] != 0)
    return dict(cmd=inp[0].copy(), cost=float(r["obj"]), status=_result_status(st), solver_status=int(st),
                is_feasible=st in (OSQP.OSQP_SOLVED, OSQP.OSQP_SOLVED_INACCURATE, OSQP.OSQP_MAX_ITER_REACHED),
                polished=polished, polished_raw=int(r["polished"]), iters=int(r["iters"]), input=inp, state=state, output=out,
                active_lower=al.astype(np.uint8), active_upper=au.astype(np.uint8), y=r["y"])


def solve_batch(sp, x0, u0, yref=None, dmeas=None, maximum_iteration=MAXIT, workers=None, pb=None):
    """solve_one over a batch (yref [B, ny] or [B, ny, ph], dmeas [B, ndu, ph]) as the dict helpers.assert_matches_oracle takes, plus
    'neq', 'ncon', 'is_feasible', 'input' [B, ph+1, nu], 'n_active' and 'n_rate_active' (active delta-u rows of the steps i <= ch)"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    pb = builder(sp) if pb is None else pb
    d = pb.d
    B = len(x0)
    workers = workers or max(1, min(4, os.cpu_count() or 1))      # (small dense solves under the GIL: more threads only get in each other's way)

    def job(b):
        return solve_one(pb, sp, x0[b], u0[b], None if yref is None else yref[b], None if dmeas is None else dmeas[b], maximum_iteration)
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(job, range(B)))
    res = {"neq": d.neq, "ncon": d.ncon}
    res["cmd"] = np.stack([p["cmd"] for p in parts]); res["cost"] = np.array([p["cost"] for p in parts])
    res["input"] = np.stack([p["input"] for p in parts])
    for k in ("status", "solver_status", "iters", "polished", "polished_raw", "is_feasible"):
        res[k] = np.array([int(p[k]) for p in parts], dtype=np.int32)
    for k in ("active_lower", "active_upper"):
        res[k] = np.stack([p[k] for p in parts])
        res[k][:, d.neq:d.neq + d.na] = 0          # the box rows of step 0 bound data, not decisions (helpers.oracle_batch_parallel_spec)
    act = (res["active_lower"] != 0) | (res["active_upper"] != 0)
    res["n_active"] = act[:, d.neq:].sum(axis=1)
    du0 = d.neq + d.off_du
    res["n_rate_active"] = act[:, du0:du0 + min(ph, ch + 1) * nu].sum(axis=1)
    return res


def compared_rows(sp):
    """the reference rows whose active bits are compared: with move blocking (ch < ph - 1) the rows test_lmpc_shapes_gpu.py leaves out --
    input, state and output rows past the control horizon, the pinned delta-u rows i > ch -- are left out here too"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    na = nx + nu
    d = LN.LmpcDims(nx, nu, ndu, ny, ph, ch)
    keep = np.zeros(d.ncon, bool)
    keep[d.neq:] = True
    du0 = d.neq + d.off_du
    keep[du0 + min(ph, ch + 1) * nu:du0 + ph * nu] = False
    if ch < ph - 1:
        for i in range(ch + 1, ph + 1):
            keep[d.neq + i * na:d.neq + (i + 1) * na] = False
            keep[d.neq + d.off_y + i * ny:d.neq + d.off_y + (i + 1) * ny] = False
    return keep


def condensed_rate_rows(sp):
    """numpy condensing of the rate rows, independent of the product: (G [m x nz], lo, hi, step, comp, refrow, u0 coefficient [m x nu])
    in the product's order among themselves (by step, then component); a row exists for a finite side only"""
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = LN.LmpcDims(nx, nu, ndu, ny, ph, ch)
    nf = min(ph, ch + 1)
    blk = [0] + [min(i, nf) - 1 for i in range(1, ph + 1)]
    G, lo, hi, step, comp, ref, U0 = [], [], [], [], [], [], []
    for i in range(nf):
        for j in range(nu):
            a, b = sp["dumin"][j, i], sp["dumax"][j, i]
            if not (np.isfinite(a) or np.isfinite(b)):
                continue
            g = np.zeros(nf * nu); c0 = np.zeros(nu)
            g[blk[i + 1] * nu + j] += 1.0
            if i >= 1:
                g[blk[i] * nu + j] -= 1.0
            else:
                c0[j] = -1.0
            G.append(g); lo.append(a); hi.append(b); step.append(i + 1); comp.append(j); ref.append(d.neq + d.off_du + i * nu + j); U0.append(c0)
    return (np.array(G).reshape(len(G), nf * nu), np.array(lo), np.array(hi), np.array(step, int), np.array(comp, int), np.array(ref, int),
            np.array(U0).reshape(len(G), nu))
