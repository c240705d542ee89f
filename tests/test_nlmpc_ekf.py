"""The observed NLMPC loop's host layer without a GPU (a controller handle needs a device, so only what a null handle reaches): the library
exports the new entry points, the Python mirror of the filter's descriptor has the size and the field offsets of the C header, null arguments
come back with their code and a message.  What needs a handle is in test_nlmpc_ekf_gpu.py.  Then the reference's own checks (nlmpc_ekf_ref.py):
its committed tolerances are what it measures, and on the UGV, whose step is linear, its covariances are the linear Kalman filter's."""
import ctypes as C

import numpy as np
import pytest

import nlmpc_ekf_ref as E

NEW = ("mpcx_nlmpc_loop_create_observed", "mpcx_nlmpc_ekf_desc_size", "mpcx_nlmpc_ekf_step_batch")


def _loop_desc():
    from libmpc_amd import _capi
    d = _capi.NlmpcLoopDesc()
    d.batch, d.ticks, d.substeps, d.warm = 4, 3, 1, 1
    d.x0 = d.u0 = d.traj_x = d.traj_u = 0x1000
    return d


def _ekf_desc(**kw):
    """a filter descriptor that passes every check made ahead of the handle (no pointer is followed there), then the fields under test"""
    from libmpc_amd import _capi
    e = _capi.NlmpcEkfDesc()
    e.ny = 1
    e.Q = e.R = e.P0 = e.traj_xhat = e.traj_y = 0x1000
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_the_library_exports_the_new_symbols():
    from libmpc_amd import _capi
    lib = _capi.lib()
    for name in NEW:
        getattr(lib, name)
        assert name in _capi.EXPORTS


def test_the_python_descriptor_has_the_size_the_library_reports():
    from libmpc_amd import _capi
    assert _capi.lib().mpcx_nlmpc_ekf_desc_size() == C.sizeof(_capi.NlmpcEkfDesc)


def test_the_python_descriptor_has_the_field_offsets_of_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess
    from libmpc_amd import _capi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpcx.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mpcx_nlmpc_ekf_desc));']
    lines += [f'  printf(" %zu", offsetof(mpcx_nlmpc_ekf_desc, {f}));' for f, _ in _capi.NlmpcEkfDesc._fields_]
    lines += ['  printf(" %zu", sizeof(mpcx_nlmpc_loop_desc));', '  return 0;', '}']
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_capi.NlmpcEkfDesc)
    assert got[1:-1] == [getattr(_capi.NlmpcEkfDesc, f).offset for f, _ in _capi.NlmpcEkfDesc._fields_]
    assert got[-1] == C.sizeof(_capi.NlmpcLoopDesc)                    # the loop's descriptor stays frozen


def test_null_arguments_are_refused_with_a_message():
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    stream = C.c_void_p(0x10)
    fake = C.c_void_p(0x2000)            # stands for a handle where the argument under test is looked at first: never followed

    def refused(rc):
        assert rc == _capi.E_INVALID, rc
        assert lib.mpcx_last_error().decode()

    d = _loop_desc()
    # the filter's descriptor is judged ahead of any look at the handle
    refused(lib.mpcx_nlmpc_loop_create_observed(fake, C.byref(d), None, stream, C.byref(out)))
    for spoil in (dict(Q=None), dict(R=None), dict(P0=None), dict(ny=0), dict(ny=-2), dict(traj_xhat=None), dict(traj_y=None)):
        refused(lib.mpcx_nlmpc_loop_create_observed(fake, C.byref(d), C.byref(_ekf_desc(**spoil)), stream, C.byref(out)))
    refused(lib.mpcx_nlmpc_loop_create_observed(None, C.byref(d), C.byref(_ekf_desc()), stream, C.byref(out)))     # null handle
    refused(lib.mpcx_nlmpc_loop_create_observed(fake, None, C.byref(_ekf_desc()), stream, C.byref(out)))           # null loop descriptor
    refused(lib.mpcx_nlmpc_loop_create_observed(fake, C.byref(d), C.byref(_ekf_desc()), stream, None))             # null out argument
    assert not out.value
    p = C.c_void_p(0x1000)
    refused(lib.mpcx_nlmpc_ekf_step_batch(None, 4, p, p, p, p, None, None, p, p, 2, 1, p, p, p, stream))


def test_the_committed_tolerances_are_what_the_reference_measures():
    """TOL = 8 x MEASURED, and MEASURED is the float64 / long-double difference of this reference on the tests' own inputs, rounded up in its
    last digit (on a platform whose long double is wider than double: elsewhere the measurement says nothing and is not made)"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is double here")
    got = E.measure()
    for model, (ex, eP) in got.items():
        mx, mP = E.MEASURED[model]
        print("%-10s xhat %.3e (committed %.2e)  P %.3e (committed %.2e)" % (model, ex, mx, eP, mP))
        assert 0.98 * mx <= ex <= mx and 0.98 * mP <= eP <= mP, model
        assert E.TOL[model] == (8 * mx, 8 * mP)


def test_on_the_linear_ugv_the_covariances_are_the_riccati_recursion():
    """The UGV's step is x+ = A x + B u, so the central difference is A up to its round-off and the reference's P sequence must be the linear Kalman
    filter's (Joseph form with the exact A).  Six ticks, free-running; the bound is 8 x the largest difference between the reference's own float64
    and long-double runs over the same six ticks, relative to max |P|."""
    model, ticks, Ts = "ugv", 6, 0.1
    d = E.inputs(model, "noise")
    rng = np.random.default_rng(5)
    B, nx = d["x0"].shape
    ny = d["Cm"].shape[0]
    d["cmd"] = rng.uniform(-0.5, 0.5, size=(ticks, B, 2)); d["noise"] = rng.normal(scale=1e-2, size=(ticks, B, nx))
    d["meas_noise"] = rng.normal(scale=1e-1, size=(ticks, B, ny))
    d["Q"], d["R"], d["P0"] = 1e-4 * np.eye(nx), 1e-2 * np.eye(ny), 1e-2 * np.eye(nx)
    _, _, P64, _, f64 = E.run(model, 1, d, Ts)
    _, _, Pld, _, _ = E.run(model, 1, d, Ts, dtype=np.longdouble)
    assert not np.any(f64)
    A = np.eye(4); A[0, 2] = A[1, 3] = Ts
    Cm, Q, R = d["Cm"], d["Q"], d["R"]
    Pk = d["P0"].copy()
    worst = own = 0.0
    for k in range(ticks):
        Pm = A @ Pk @ A.T + Q
        K = Pm @ Cm.T @ np.linalg.inv(Cm @ Pm @ Cm.T + R)
        J = np.eye(4) - K @ Cm
        Pk = J @ Pm @ J.T + K @ R @ K.T
        Pk = (Pk + Pk.T) / 2
        worst = max(worst, E.rel_P(P64[k + 1], np.tile(Pk, (B, 1, 1))))
        own = max(own, E.rel_P(P64[k + 1], Pld[k + 1]))
    print("ugv, six ticks: reference against the Riccati recursion %.2e, float64 against long double %.2e" % (worst, own))
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert worst <= 8 * own, (worst, own)
    assert worst <= 8 * 6 * E.MEASURED[model][1]           # (where long double is double: six ticks of the committed one-step figure)
