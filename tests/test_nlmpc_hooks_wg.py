"""Whole-vector hooks (mpcx::HookModel, the reference's hook signatures) on the workgroup form of the SQP (nlmpc_sqp_wg): the kernel
instantiated for four systems written as functors (tests/emu/run_hooks_wg.cpp), the controller's workspace laid out by engine::nlmpc_plan with
the form's hook buffers reserved.  Stepped through on the host by the lock-step interpreter of tests/emu, in both thread orders and at one and
four wavefronts per instance (no GPU, nothing of libmpcx.so); the same driver built by hipcc runs the kernels on the GPU (the gpu tests)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import nlmpc_numpy as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")

ORDERS_AND_WAVES = [{"HIPEMU_WAVES": "1"}, {"HIPEMU_WAVES": "1", "HIPEMU_ORDER": "reverse"},
                    {"HIPEMU_WAVES": "4"}, {"HIPEMU_WAVES": "4", "HIPEMU_ORDER": "reverse"}]


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("emu") / "run_hooks_wg")
    subprocess.run(["g++", "-O1", "-std=c++20", "-DHIPEMU_WITH_WG", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), "-fpermissive", "-w", "-o", exe,
                    os.path.join(EMU, "run_hooks_wg.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)

    def run(args, inst, env=None):
        e = dict(os.environ); e.update(env or {})
        inp = "\n".join(" ".join(repr(float(x)) for x in row) for row in inst) + "\n"
        r = subprocess.run([exe] + [str(a) for a in args], input=inp, capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 0, r.stderr[:2000]
        return [json.loads(l) for l in r.stdout.splitlines()]
    return run


def _check_against_oracle(rows, model, X0, U0, hard=True, max_iter=1000, **bounds):
    for b, y in enumerate(rows):
        o = model.solve(X0[b], U0[b], max_iter=max_iter, hard=hard, **bounds)
        assert y["status"] == (0 if o["success"] else 1), (b, y["status"], o["message"])
        if o["success"]:
            np.testing.assert_allclose(y["cmd"], o["cmd"], rtol=1e-5, atol=1e-5, err_msg="instance %d" % b)


@pytest.mark.parametrize("env", ORDERS_AND_WAVES)
def test_vanderpol_hooks_reach_the_oracle_optimum_on_the_workgroup_form(runner, env):
    rng = np.random.default_rng(11)
    X0 = rng.uniform(-1.0, 1.0, size=(3, 2)); X0[0] = [0.0, 1.0]          # examples/vanderpol_ex.cpp:67
    U0 = np.zeros((3, 1))
    r = runner(["vanderpol", 1, 200, "wg"], np.hstack([X0, U0]), env)
    _check_against_oracle(r, ref.vanderpol(ph=10, ch=5, Ts=0.1), X0, U0)
    assert all(y["solver_status"] == 4 for y in r)


@pytest.mark.parametrize("env", ORDERS_AND_WAVES)
def test_terminal_equality_and_output_hook_on_the_workgroup_form(runner, env):
    """setEqConFunction and setOutputFunction: x(ph) = 0, the cost written on the outputs y = x"""
    X0 = np.array([[0.1, 0.1], [0.05, -0.08]])
    U0 = np.zeros((2, 1))
    r = runner(["vanderpol_terminal", 1, 300, "wg"], np.hstack([X0, U0]), env)
    _check_against_oracle(r, ref.vanderpol_terminal(ph=10, ch=5, Ts=0.1), X0, U0)
    for y in r:
        X = np.asarray(y["seq_state"]).reshape(11, 2)
        assert np.abs(X[10]).max() <= 1e-9
        np.testing.assert_array_equal(np.asarray(y["seq_output"]), np.asarray(y["seq_state"]))       # y = x through the output hook


@pytest.mark.parametrize("env", ORDERS_AND_WAVES)
def test_ugv_hooks_with_soft_constraints_and_input_bounds_on_the_workgroup_form(runner, env):
    """the discrete UGV (ph 12, ch 4), obstacle rows as one black box, hard_constraints = 0 (the slack column), input bounds (short-list rows
    next to the hooks' dense ones)"""
    X0 = np.array([[0.0, 0.0, 0.0, 0.0], [0.2, -0.1, 0.0, 0.0]])
    U0 = np.zeros((2, 2))
    r = runner(["ugv", 0, 150, "wg", "lbu=-4", "ubu=4"], np.hstack([X0, U0]), env)
    _check_against_oracle(r, ref.ugv(ph=12, ch=4), X0, U0, hard=False, lb_u=[-4.0, -4.0], ub_u=[4.0, 4.0])
    for y in r:
        assert max(abs(c) for c in y["cmd"]) <= 4.0 + 1e-12


def test_workgroup_form_agrees_with_the_wavefront_form_of_the_same_hooks(runner):
    X0 = np.array([[0.0, 0.0, 0.0, 0.0], [0.2, -0.1, 0.0, 0.0]])
    inst = np.hstack([X0, np.zeros((2, 2))])
    a = runner(["ugv", 0, 150, "wave"], inst)
    b = runner(["ugv", 0, 150, "wg"], inst)
    for x, y in zip(a, b):
        assert x["status"] == y["status"] == 0 and x["solver_status"] == y["solver_status"]
        np.testing.assert_allclose(y["cmd"], x["cmd"], rtol=1e-6, atol=1e-6)
        assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(x["cost"])


def chain9_oracle():
    """the driver's chain9: nine discrete integrators in a chain driven at the first, |u| <= 1 + e as rows, x(ph, 0) = 0"""
    ph, ch = 6, 3
    m = ref.NlmpcRef(9, 1, 9, ph, ch, 2 * ph, eq=1)
    m.continuous = False

    def f(x, u, step):
        y = x.copy()
        y[0] = x[0] + 0.1 * u[0]
        y[1:] = x[1:] + 0.1 * x[:-1]
        return y
    m.f = f
    m.cost = lambda X, Y, U, e: float(np.sum(X * X) + 0.1 * np.sum(U * U) + 10.0 * e * e)
    m.ineq_fun = lambda X, Y, U, e: np.array([v for i in range(ph) for v in (U[i, 0] - 1.0 - e, -U[i, 0] - 1.0 - e)])
    m.eq_fun = lambda X, U: np.array([X[ph, 0]])
    return m


@pytest.mark.parametrize("env", [{"HIPEMU_WAVES": "1"}, {"HIPEMU_WAVES": "4", "HIPEMU_ORDER": "reverse"}])
def test_wide_state_with_an_equality_and_soft_constraints_on_the_workgroup_form(runner, env):
    """NX > 8: every sub-problem row is as long as the whole input part plus the slack column, equality rows included -- their slack entry is
    zero, not whatever the row's storage held (the interpreter starts LDS and the workspace as NaNs)"""
    X0 = np.array([[0.5, 0.3, -0.2, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0], [-0.8, 0.1, 0.2, -0.1, 0.3, 0.0, 0.0, 0.0, 0.0]])
    U0 = np.zeros((2, 1))
    a = runner(["chain9", 0, 200, "wave"], np.hstack([X0, U0]))
    b = runner(["chain9", 0, 200, "wg"], np.hstack([X0, U0]), env)
    _check_against_oracle(b, chain9_oracle(), X0, U0, hard=False)
    for x, y in zip(a, b):
        assert x["status"] == y["status"] == 0 and np.isfinite(y["cost"])
        np.testing.assert_allclose(y["cmd"], x["cmd"], rtol=1e-6, atol=1e-6)
        assert abs(np.asarray(y["seq_state"]).reshape(7, 9)[6, 0]) <= 1e-8


# ---- the same driver built by hipcc: the kernels on the GPU ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_runner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hip") / "run_hooks_wg")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++20", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-x", "hip",
                    os.path.join(EMU, "run_hooks_wg.cpp")], check=True, timeout=1200)

    def run(args, inst, env=None):
        e = dict(os.environ); e.update(env or {})
        inp = "\n".join(" ".join(repr(float(x)) for x in row) for row in inst) + "\n"
        r = subprocess.run([exe] + [str(a) for a in args], input=inp, capture_output=True, text=True, env=e, timeout=300)
        assert r.returncode == 0, r.stderr[:2000]
        return [json.loads(l) for l in r.stdout.splitlines()]
    return run


def _starts(name, B, seed):
    rng = np.random.default_rng(seed)
    if name == "vanderpol":
        X0 = rng.uniform(-1.0, 1.0, size=(B, 2)); X0[0] = [0.0, 1.0]
        return np.hstack([X0, np.zeros((B, 1))])
    if name == "vanderpol_terminal":
        X0 = rng.uniform(-0.12, 0.12, size=(B, 2)); X0[0] = [0.1, 0.1]
        return np.hstack([X0, np.zeros((B, 1))])
    X0 = np.zeros((B, 4)); X0[:, :2] = rng.uniform(-0.5, 0.5, size=(B, 2))
    return np.hstack([X0, np.zeros((B, 2))])


@pytest.mark.gpu
@pytest.mark.parametrize("name,hard,iters", [("vanderpol", 1, 200), ("vanderpol_terminal", 1, 300), ("ugv", 0, 150)])
@pytest.mark.parametrize("B", [1, 7, 257, 4096])
def test_workgroup_form_matches_the_wavefront_form_of_the_same_hooks_on_the_gpu(gpu_runner, name, hard, iters, B):
    """the same statuses and optimum as nlmpc_sqp on the same hooks, at the plan's own wavefront count and at four"""
    inst = _starts(name, B, 3 + B)
    a = gpu_runner([name, hard, iters, "wave"], inst)
    for env in ({}, {"HIPEMU_WAVES": "4"}):
        b = gpu_runner([name, hard, iters, "wg"], inst, env)
        sa = np.array([x["solver_status"] for x in a]); sb = np.array([y["solver_status"] for y in b])
        assert np.array_equal(sa, sb), (env, np.flatnonzero(sa != sb)[:10])
        ok = sa == 4
        assert ok[0] and ok.mean() >= 0.9
        ca = np.array([x["cmd"] for x in a])[ok]; cb = np.array([y["cmd"] for y in b])[ok]
        # (the two forms add in different orders and stop at the same step tolerance: the cross-form tolerance of tests/test_emu_nlmpc.py)
        np.testing.assert_allclose(cb, ca, rtol=1e-5, atol=1e-5, err_msg=str(env))


@pytest.mark.gpu
def test_workgroup_form_of_hooks_reaches_the_oracle_on_the_gpu(gpu_runner):
    X0 = np.array([[0.0, 1.0], [0.4, -0.3], [-0.7, 0.2]])
    r = gpu_runner(["vanderpol", 1, 200, "wg"], np.hstack([X0, np.zeros((3, 1))]), {"HIPEMU_WAVES": "4"})
    _check_against_oracle(r, ref.vanderpol(ph=10, ch=5, Ts=0.1), X0, np.zeros((3, 1)))
    X9 = np.array([[0.5, 0.3, -0.2, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0]])
    r = gpu_runner(["chain9", 0, 200, "wg"], np.hstack([X9, np.zeros((1, 1))]))
    _check_against_oracle(r, chain9_oracle(), X9, np.zeros((1, 1)), hard=False)


@pytest.mark.gpu
def test_twenty_launches_of_the_workgroup_form_give_the_same_bits(gpu_runner):
    inst = _starts("ugv", 257, 41)
    for env in ({}, {"HIPEMU_WAVES": "4"}):
        r = gpu_runner(["ugv", 0, 150, "wg", "repeat=20"], inst, env)
        assert all(y["same_bits"] == 1 for y in r), env
