"""The advance body of the NLMPC closed loop (include/mpcx/nlmpc_loop.hpp) stepped through on the host by the lock-step interpreter of tests/emu
(TEST INFRASTRUCTURE, see tests/emu/hip/hip_runtime.h): the header is compiled unchanged with g++ and three ticks of a fixed command sequence must
give the trajectories of the same formulas in numpy float64, in both orders in which the interpreter may run the threads of a block.  No GPU,
nothing of libmpcx.so, no solve: the runner (tests/emu/run_nlmpc_loop.cpp) feeds the commands and the solve's results of every tick."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import nlmpc_plant_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
B, TICKS, PAD = 70, 3, 64                       # two tiles, the second partial; PAD: the runner's guard behind every array
GUARD, GUARD_I = -7.25e300, -777
DIMS = {"vanderpol": (2, 1), "ugv": (4, 2)}


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("emu") / "run_nlmpc_loop")
    subprocess.run(["g++", "-O1", "-std=c++20", "-DHIPEMU_WITH_WG", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), "-fpermissive", "-w", "-o", exe,
                    os.path.join(EMU, "run_nlmpc_loop.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)

    def run(args, numbers, env=None):
        e = dict(os.environ); e.update(env or {})
        inp = " ".join(repr(float(v)) for v in numbers) + "\n"
        r = subprocess.run([exe] + [str(a) for a in args], input=inp, capture_output=True, text=True, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[:2000]
        return json.loads(r.stdout)
    return run


def _inputs(model, variant):
    """seeded inputs of a case: states and commands in the range the controllers work in, the solve's logs as recognisable numbers"""
    nx, nu = DIMS[model]
    rng = np.random.default_rng(41)
    d = dict(x0=rng.uniform(-1.0, 1.0, size=(B, nx)), u0=rng.uniform(-0.5, 0.5, size=(B, nu)), cmd=rng.uniform(-0.5, 0.5, size=(TICKS, B, nu)),
             cost=rng.uniform(0.0, 10.0, size=(TICKS, B)), ints=rng.integers(-5, 200, size=(TICKS, 4, B)),
             ctrl=np.array(P.DEFAULT_PARAMS[model]), noise=None, params=None, plant=None)
    if "noise" in variant:
        d["noise"] = rng.normal(scale=1e-2, size=(TICKS, B, nx))
    if "plant" in variant:                      # per-instance controller parameters AND other ones for the plant: the plant's must win
        base = np.tile(d["ctrl"], (B, 1))
        d["params"] = base * (1.0 + rng.uniform(-0.1, 0.1, size=base.shape))
        d["plant"] = base * (1.0 + rng.uniform(-0.1, 0.1, size=base.shape))
        if model == "ugv":
            d["plant"][:, 8] = rng.choice([0.05, 0.1, 0.2], size=B)            # the sample time is what the UGV's plant reads
    return d


CASES = [("vanderpol", 1, ""), ("vanderpol", 4, ""), ("vanderpol", 1, "noise"), ("vanderpol", 4, "noise"), ("ugv", 1, ""), ("ugv", 1, "noise"),
         ("ugv", 1, "plant"), ("ugv", 1, "noise+plant")]


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("model,substeps,variant", CASES)
def test_three_ticks_of_the_advance_body_against_numpy(runner, model, substeps, variant, order):
    nx, nu = DIMS[model]
    d = _inputs(model, variant)
    Ts = 0.1
    numbers = [d["ctrl"].ravel(), d["x0"].ravel(), d["u0"].ravel()]
    for k in range(TICKS):
        numbers += [d["cmd"][k].ravel(), d["cost"][k], d["ints"][k].ravel()]
    for key in ("noise", "params", "plant"):
        if d[key] is not None:
            numbers.append(d[key].ravel())
    o = runner([model, Ts, substeps, B, TICKS, int(d["noise"] is not None), int(d["params"] is not None), int(d["plant"] is not None)],
               np.concatenate(numbers), {"HIPEMU_ORDER": order})

    def split(name, n, guard):
        a = np.array(o[name])
        assert a.size == n + PAD and (a[n:] == guard).all(), name          # nothing behind the array: no lane past B stores anything
        return a[:n]
    tx = split("traj_x", (TICKS + 1) * B * nx, GUARD).reshape(TICKS + 1, B, nx)
    tu = split("traj_u", TICKS * B * nu, GUARD).reshape(TICKS, B, nu)
    x = split("x", B * nx, GUARD).reshape(B, nx)
    u = split("u", B * nu, GUARD).reshape(B, nu)
    p = d["plant"] if d["plant"] is not None else d["ctrl"]
    worst = 0.0
    assert np.array_equal(tx[0], d["x0"])
    for k in range(TICKS):
        # from the state the body itself started the tick at: the bound is that of one tick
        want, bound = P.step(model, tx[k], d["cmd"][k], p, Ts, substeps, None if d["noise"] is None else d["noise"][k])
        err = np.abs(tx[k + 1] - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, float(err.max()), float(bound.min()))
        assert np.array_equal(tu[k], d["cmd"][k])                          # the command as it is
    print("%s substeps %d %s %s: worst error / bound %.3f" % (model, substeps, variant, order, worst))
    assert np.array_equal(x, tx[TICKS]) and np.array_equal(u, d["cmd"][TICKS - 1])
    assert np.array_equal(split("traj_cost", TICKS * B, GUARD).reshape(TICKS, B), d["cost"])
    for j, name in enumerate(("traj_status", "traj_solver_status", "traj_is_feasible", "traj_iterations")):
        assert np.array_equal(split(name, TICKS * B, GUARD_I).reshape(TICKS, B), d["ints"][:, j]), name
