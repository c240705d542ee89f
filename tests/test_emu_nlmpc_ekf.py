"""The observed advance body of the NLMPC closed loop (include/mpcx/nlmpc_ekf.hpp: plant step, measurement, extended Kalman filter) stepped
through on the host by the lock-step interpreter of tests/emu (TEST INFRASTRUCTURE, see tests/emu/hip/hip_runtime.h): the header is compiled
unchanged with g++, and every one of three ticks of a fixed command sequence, taken from the body's own logged xhat_k, P_k, must give what
nlmpc_ekf_ref.py gives within its tolerances, in both orders in which the interpreter may run the threads of a block.  No GPU, nothing of
libmpcx.so, no solve: the runner (tests/emu/run_nlmpc_ekf.cpp) feeds the commands and the solve's results of every tick.

Batches (nlmpc_ekf_ref.BATCH): 23 Van der Pol instances at 10 per block, 13 UGVs at 6, 5 six-oscillator networks at 2 -- at least two blocks,
the last partial."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import nlmpc_ekf_ref as E
import nlmpc_plant_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -777
TICKS = E.TICKS
CASES = [c for c in E.cases() if c[0] != "osc8"]


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("emu") / "run_nlmpc_ekf")
    subprocess.run(["g++", "-O1", "-std=c++20", "-DHIPEMU_WITH_WG", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), "-fpermissive", "-w", "-o", exe,
                    os.path.join(EMU, "run_nlmpc_ekf.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)

    def run(args, numbers, env=None):
        e = dict(os.environ); e.update(env or {})
        inp = " ".join(repr(float(v)) for v in numbers) + "\n"
        r = subprocess.run([exe] + [str(a) for a in args], input=inp, capture_output=True, text=True, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[:2000]
        return json.loads(r.stdout)
    return run


def _run_body(runner, model, substeps, d, order, Ts=0.1):
    nx, nu = E.DIMS[model]
    B = d["x0"].shape[0]
    d = dict(d, Cm=np.eye(nx) if d["Cm"] is None else d["Cm"])          # (the identity is what the library makes of Cm = NULL)
    ny = d["Cm"].shape[0]
    numbers = [d["ctrl"].ravel(), d["x0"].ravel(), d["u0"].ravel()]
    for k in range(TICKS):
        numbers += [d["cmd"][k].ravel(), d["cost"][k], d["ints"][k].ravel()]
    numbers += [d[key].ravel(order="F") for key in ("Cm", "Q", "R", "P0")]
    for key in ("noise", "params", "plant", "meas_noise", "xhat0"):
        if d[key] is not None:
            numbers.append(d[key].ravel())
    o = runner([model, Ts, substeps, B, TICKS, ny] + [int(d[k] is not None) for k in ("noise", "params", "plant", "meas_noise", "xhat0")],
               np.concatenate(numbers), {"HIPEMU_ORDER": order})

    def split(name, shape, guard=GUARD):
        a = np.array(o[name])
        n = int(np.prod(shape))
        assert a.size == n + PAD and (a[n:] == guard).all(), name          # nothing behind the array: no lane without an instance stores anything
        return a[:n].reshape(shape)
    return split


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("model,substeps,variant", CASES)
def test_three_ticks_of_the_observed_body_against_numpy(runner, model, substeps, variant, order):
    nx, nu = E.DIMS[model]
    d = E.inputs(model, variant)
    B, ny, Ts = d["x0"].shape[0], d["R"].shape[0], 0.1
    split = _run_body(runner, model, substeps, d, order)
    tx = split("traj_x", (TICKS + 1, B, nx)); txh = split("traj_xhat", (TICKS + 1, B, nx)); ty = split("traj_y", (TICKS, B, ny))
    tP = split("traj_P", (TICKS + 1, B, nx, nx)); tu = split("traj_u", (TICKS, B, nu)); plain = split("plain_traj_x", (TICKS + 1, B, nx))
    flags = split("flags", (B,), GUARD_I)
    split("cb", (ny * nx + nx * nx + ny * ny + nx * nx,))                   # the constant block is read only
    pc = d["ctrl"] if d["params"] is None else d["params"]
    pp = d["plant"] if d["plant"] is not None else pc
    tol_x, tol_P = E.TOL[model]
    assert np.array_equal(tx[0], d["x0"]) and np.array_equal(txh[0], d["x0"] if d["xhat0"] is None else d["xhat0"])
    worst = [0.0, 0.0, 0.0]
    for k in range(TICKS):
        w = None if d["noise"] is None else d["noise"][k]
        v = None if d["meas_noise"] is None else d["meas_noise"][k]
        # the truth: the plant step's own bound, from the state the body itself started the tick at -- against numpy and against the unobserved body
        want, bound = P.step(model, tx[k], d["cmd"][k], pp, Ts, substeps, w)
        err = np.abs(tx[k + 1] - want)
        worst[0] = max(worst[0], float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, float(err.max()))
        assert (np.abs(tx[k + 1] - plain[k + 1]) <= bound).all(), k
        # the measurement: a dot product of nx terms and the noise, (nx + 1) 2^-52 sum |terms|
        Cm = np.eye(nx) if d["Cm"] is None else d["Cm"]
        ywant = tx[k + 1] @ Cm.T + (0.0 if v is None else v)
        ybound = (nx + 1) * P.U * (np.abs(tx[k + 1]) @ np.abs(Cm).T + (0.0 if v is None else np.abs(v)))
        assert (np.abs(ty[k] - ywant) <= ybound).all(), k
        # the filter, from the body's own xhat_k, P_k and its own measurement
        xh, Pn, fl = E.ekf_step(model, txh[k], tP[k], d["cmd"][k], ty[k], pc, Ts, substeps, d["Cm"], d["Q"], d["R"])
        ex, eP = E.rel_x(txh[k + 1], xh), E.rel_P(tP[k + 1], Pn)
        worst[1] = max(worst[1], ex / tol_x); worst[2] = max(worst[2], eP / tol_P)
        assert ex <= tol_x and eP <= tol_P, (k, ex, tol_x, eP, tol_P)
        assert not fl.any()
        assert np.array_equal(tP[k + 1], np.swapaxes(tP[k + 1], 1, 2))       # symmetric, bit for bit
        assert np.array_equal(tu[k], d["cmd"][k])                          # the command as it is
    print("%s substeps %d %s %s: worst error / bound: truth %.3f, xhat %.3f, P %.3f" % ((model, substeps, variant, order) + tuple(worst)))
    assert not flags.any()
    assert np.array_equal(split("x", (B, nx)), txh[TICKS]) and np.array_equal(split("xt", (B, nx)), tx[TICKS])
    assert np.array_equal(split("P", (B, nx, nx)), tP[TICKS]) and np.array_equal(split("u", (B, nu)), d["cmd"][TICKS - 1])
    assert np.array_equal(split("traj_cost", (TICKS, B)), d["cost"])
    for j, name in enumerate(("traj_status", "traj_solver_status", "traj_is_feasible", "traj_iterations")):
        assert np.array_equal(split(name, (TICKS, B), GUARD_I), d["ints"][:, j]), name
    if d["noise"] is None and d["plant"] is None:
        assert np.array_equal(txh, tx)                                     # certainty equivalence: one call site, equal inputs, equal bits


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_a_failed_cholesky_skips_the_update(runner, order):
    """P0 = Q = R = 0: the first pivot of S is 0.  The estimate is the prediction, P stays 0, the flag is set, nothing is non-finite"""
    model = "ugv"
    d = E.inputs(model, "noise")
    for key in ("Q", "R", "P0"):
        d[key] = np.zeros_like(d[key])
    B, nx = d["x0"].shape
    split = _run_body(runner, model, 1, d, order)
    txh = split("traj_xhat", (TICKS + 1, B, nx)); tP = split("traj_P", (TICKS + 1, B, nx, nx))
    assert (split("flags", (B,), GUARD_I) == 1).all()
    assert (tP == 0).all() and np.isfinite(txh).all()
    for k in range(TICKS):
        want, bound = P.step(model, txh[k], d["cmd"][k], d["ctrl"], 0.1, 1, None)
        assert (np.abs(txh[k + 1] - want) <= bound).all(), k
