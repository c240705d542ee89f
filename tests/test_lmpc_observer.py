"""Output feedback for the closed loop, the host layer without a GPU: the observer descriptor's mirror, the refusals of
mpcx_lmpc_loop_create_observed / mpcx_lmpc_hetero_loop_create_observed (which come ahead of any look at the handle's or the bank's state, so a
host-only handle and a bank pointer that is never followed reach them), the front-end's own shape checks, and LMPC.kalman_gain against scipy's
discrete algebraic Riccati solver."""
import ctypes as C

import numpy as np
import pytest

from helpers import configure_random, random_lmpc_spec


def _host_controller(spec=None):
    from libmpc_amd import LMPC
    sp = spec or random_lmpc_spec(3)
    return configure_random(LMPC(*sp["dims"], device=-1), sp)


def _desc(**kw):
    """a loop descriptor that passes every check (no pointer is followed on a host-only handle), then the fields under test"""
    from libmpc_amd import _capi
    d = _capi.LoopDesc()
    d.batch, d.ticks = 4, 3
    d.x0 = d.u0 = d.traj_x = d.traj_u = 0x1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _observer(**kw):
    from libmpc_amd import _capi
    o = _capi.ObserverDesc()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---------------------------------------------------------------------------------------------
# the struct and the symbols
# ---------------------------------------------------------------------------------------------
def test_the_observer_descriptor_has_the_size_the_library_reports():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.ObserverDesc) == _capi.lib().mpcx_lmpc_observer_desc_size()
    assert [f for f, _ in _capi.ObserverDesc._fields_] == ["gain", "gain_batch", "xhat0", "meas_noise", "traj_xhat", "traj_y"]


def test_the_observer_descriptor_has_the_field_offsets_of_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess
    from libmpc_amd import _capi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpcx.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mpcx_lmpc_observer_desc));']
    lines += [f'  printf(" %zu", offsetof(mpcx_lmpc_observer_desc, {f}));' for f, _ in _capi.ObserverDesc._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_capi.ObserverDesc)
    assert got[1:] == [getattr(_capi.ObserverDesc, f).offset for f, _ in _capi.ObserverDesc._fields_]


def test_the_new_entries_are_exported():
    from libmpc_amd import _capi
    lib = _capi.lib()
    for name in ("mpcx_lmpc_loop_create_observed", "mpcx_lmpc_hetero_loop_create_observed", "mpcx_lmpc_observer_desc_size", "mpcx_lmpc_kalman_gain"):
        assert name in _capi.EXPORTS and getattr(lib, name) is not None, name


# ---------------------------------------------------------------------------------------------
# the refusals, each MPCX_E_INVALID with a message naming the field
# ---------------------------------------------------------------------------------------------
def _create(c, d, o):
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    rc = lib.mpcx_lmpc_loop_create_observed(c._h, C.byref(d), None if o is None else C.byref(o), C.c_void_p(0x10), C.byref(out))
    msg = lib.mpcx_last_error().decode()
    assert not out.value
    return rc, msg


def test_an_invalid_observer_is_refused_with_a_message_on_a_host_only_handle():
    from libmpc_amd import _capi
    c = _host_controller()
    G = np.asfortranarray(np.zeros((3, 2)))
    rc, msg = _create(c, _desc(), None)
    assert rc == _capi.E_INVALID and "observer" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), _observer())
    assert rc == _capi.E_INVALID and "gain" in msg and "gain_batch" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), _observer(gain=G.ctypes.data, gain_batch=0x2000))
    assert rc == _capi.E_INVALID and "gain" in msg and "gain_batch" in msg and "exclude" in msg, (rc, msg)
    # the loop descriptor is looked at first, and the handle's state last: a good observer on a host-only handle is a state error
    rc, msg = _create(c, _desc(ticks=0), None)
    assert rc == _capi.E_INVALID and "ticks" in msg, (rc, msg)
    for o in (_observer(gain=G.ctypes.data), _observer(gain_batch=0x2000)):
        rc, msg = _create(c, _desc(), o)
        assert rc == _capi.E_STATE and "host-only" in msg, (rc, msg)
    # the unobserved entry does not look for an observer
    lib = _capi.lib()
    out = C.c_void_p()
    assert lib.mpcx_lmpc_loop_create(c._h, C.byref(_desc()), C.c_void_p(0x10), C.byref(out)) == _capi.E_STATE


def test_a_bank_refuses_one_gain_for_all_and_the_other_invalid_observers():
    from libmpc_amd import _capi
    lib = _capi.lib()
    bank = C.c_void_p(0x1000)          # never followed: the descriptor checks come first
    G = np.asfortranarray(np.zeros((3, 2)))

    def create(o):
        out = C.c_void_p()
        rc = lib.mpcx_lmpc_hetero_loop_create_observed(bank, C.byref(_desc()), None if o is None else C.byref(o), None, C.c_void_p(0x10), C.byref(out))
        assert not out.value
        return rc, lib.mpcx_last_error().decode()
    rc, msg = create(_observer(gain=G.ctypes.data))
    assert rc == _capi.E_INVALID and "bank" in msg and "gain_batch" in msg, (rc, msg)
    rc, msg = create(None)
    assert rc == _capi.E_INVALID and "observer" in msg, (rc, msg)
    rc, msg = create(_observer())
    assert rc == _capi.E_INVALID and "gain" in msg, (rc, msg)
    rc, msg = create(_observer(gain=G.ctypes.data, gain_batch=0x2000))
    assert rc == _capi.E_INVALID and "exclude" in msg, (rc, msg)
    out = C.c_void_p()
    assert lib.mpcx_lmpc_hetero_loop_create_observed(None, C.byref(_desc()), C.byref(_observer(gain_batch=0x2000)), None, C.c_void_p(0x10), C.byref(out)) == _capi.E_INVALID


# ---------------------------------------------------------------------------------------------
# the front-end's shape checks: ValueError ahead of any device call (the handle is host-only: the device layer would raise MpcxError)
# ---------------------------------------------------------------------------------------------
BAD_SHAPES = {
    "gain transposed": dict(observer=np.zeros((2, 3))),
    "gain batch": dict(observer=np.zeros((5, 3, 2))),
    "gain rows": dict(observer=np.zeros((4, 2, 2))),
    "gain 1-D": dict(observer=np.zeros(6)),
    "xhat0 batch": dict(observer=np.zeros((3, 2)), xhat0=np.zeros((3, 3))),
    "xhat0 cols": dict(observer=np.zeros((3, 2)), xhat0=np.zeros((4, 2))),
    "meas_noise ticks": dict(observer=np.zeros((3, 2)), meas_noise=np.zeros((4, 4, 2))),
    "meas_noise outputs": dict(observer=np.zeros((4, 3, 2)), meas_noise=np.zeros((5, 4, 3))),
    "xhat0 without an observer": dict(xhat0=np.zeros((4, 3))),
    "meas_noise without an observer": dict(meas_noise=np.zeros((5, 4, 2))),
}


@pytest.mark.parametrize("bad", sorted(BAD_SHAPES))
def test_a_wrong_observer_shape_raises_a_value_error_before_any_device_call(bad):
    c = _host_controller()
    with pytest.raises(ValueError):
        c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, **BAD_SHAPES[bad])
    with pytest.raises(ValueError):
        c.simulate(np.zeros((4, 3)), np.zeros((4, 2)), 5, **BAD_SHAPES[bad])


def test_well_shaped_observer_arguments_reach_the_device_layer():
    from libmpc_amd import MpcxError
    c = _host_controller()
    for obs in (np.zeros((3, 2)), np.zeros((4, 3, 2))):
        with pytest.raises(MpcxError):
            c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, observer=obs, xhat0=np.zeros((4, 3)), meas_noise=np.zeros((5, 4, 2)))


def test_the_bank_front_end_refuses_one_gain_for_all_before_any_device_call():
    """LMPCHetero.make_loop's checks need no bank: they are run here on an object that has only the dimensions"""
    from libmpc_amd import LMPCHetero
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h = 3, 2, 2, 1, 6, 0, None
    with pytest.raises(ValueError, match="bank"):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, observer=np.zeros((3, 2)))
    with pytest.raises(ValueError):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, observer=np.zeros((4, 2, 3)))
    with pytest.raises(ValueError):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, observer=np.zeros((4, 3, 2)), xhat0=np.zeros((4, 2)))


def test_results_without_an_observer_keep_their_constructor():
    from libmpc_amd import ClosedLoopResult
    r = ClosedLoopResult(1, 2, 3, 4, 5, 6, 7, 8)
    assert r.xhat is None and r.y is None and r.active_count == 8


# ---------------------------------------------------------------------------------------------
# the Kalman gain
# ---------------------------------------------------------------------------------------------
def _quadrotor_host():
    from libmpc_amd.workloads import quadrotor_lmpc, quadrotor_matrices
    A, _, Cm = quadrotor_matrices()
    return quadrotor_lmpc(10, device=-1), A, Cm


def _random_host(seed, **kw):
    sp = random_lmpc_spec(seed, **kw)
    return _host_controller(sp), sp["A"], sp["C"]


MODELS = {"random3": lambda: _random_host(3), "random100": lambda: _random_host(100), "random3_ny3": lambda: _random_host(3, nx=2, ny=3),
          "quadrotor": _quadrotor_host}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_kalman_gain_matches_the_riccati_solution_of_scipy(name):
    """tolerance 1e-10 relative in the max norm: the iteration stops at 1e-14, the rest is the conditioning of the Riccati equation"""
    from scipy.linalg import solve_discrete_are
    c, A, Cm = MODELS[name]()
    nx, ny = A.shape[0], Cm.shape[0]
    Qw, Rv = 0.01 * np.eye(nx), 0.04 * np.eye(ny)
    L, P, it = c.kalman_gain(Qw, Rv, want_P=True)
    assert np.array_equal(L, c.kalman_gain(Qw, Rv))
    Pref = solve_discrete_are(A.T, Cm.T, Qw, Rv)
    Lref = A @ Pref @ Cm.T @ np.linalg.inv(Cm @ Pref @ Cm.T + Rv)
    eL = np.abs(L - Lref).max() / np.abs(Lref).max()
    eP = np.abs(P - Pref).max() / np.abs(Pref).max()
    rho = np.abs(np.linalg.eigvals(A - L @ Cm)).max()
    print("%s: %d iterations, gain error %.2e, P error %.2e, spectral radius of A - L C %.4f" % (name, it, eL, eP, rho))
    assert L.shape == (nx, ny) and 0 < it < 100000
    assert eL <= 1e-10 and eP <= 1e-10, (name, eL, eP)
    assert np.array_equal(P, P.T)
    assert rho < 1.0, (name, rho)


def test_kalman_gain_error_returns():
    from libmpc_amd import LMPC, MpcxError, _capi
    sp = random_lmpc_spec(3)
    Qw, Rv = 0.01 * np.eye(3), 0.04 * np.eye(2)
    with pytest.raises(MpcxError) as e:
        LMPC(*sp["dims"], device=-1).kalman_gain(Qw, Rv)
    assert e.value.code == _capi.E_STATE and "model" in str(e.value)
    c = _host_controller(sp)
    skew = Qw.copy(); skew[0, 1] = 0.005
    with pytest.raises(MpcxError) as e:
        c.kalman_gain(skew, Rv)
    assert e.value.code == _capi.E_INVALID and "Qw" in str(e.value)
    skew = Rv.copy(); skew[1, 0] = 0.01
    with pytest.raises(MpcxError) as e:
        c.kalman_gain(Qw, skew)
    assert e.value.code == _capi.E_INVALID and "Rv" in str(e.value)
    with pytest.raises(MpcxError) as e:
        c.kalman_gain(Qw, np.array([[1.0, 2.0], [2.0, 1.0]]))          # symmetric, indefinite
    assert e.value.code == _capi.E_INVALID and "positive definite" in str(e.value)
    with pytest.raises(ValueError):
        c.kalman_gain(np.eye(2), Rv)
    # an unstable mode no output sees: the covariance grows without bound and the iteration cannot converge
    A = np.diag([1.5, 0.5, 0.2]); Cm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    u = LMPC(*sp["dims"], device=-1)
    assert u.setStateSpaceModel(A, sp["B"], Cm)
    with pytest.raises(MpcxError) as e:
        u.kalman_gain(Qw, Rv)
    assert e.value.code == _capi.E_NUMERIC, str(e.value)
