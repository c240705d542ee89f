"""Offset-free loops, the host layer without a GPU: the disturbance observer descriptor's mirror, the refusals of
mpcx_lmpc_loop_create_offset_free / mpcx_lmpc_hetero_loop_create_offset_free (ahead of any look at the handle's or the bank's state, so a
host-only handle and a bank pointer that is never followed reach them), the front-end's shape checks and the detectability check of the
augmented pair, all of which come before any device call."""
import ctypes as C

import numpy as np
import pytest

from helpers import configure_random, random_lmpc_spec

FIELDS = ["gain", "gain_batch", "xhat0", "dhat0", "meas_noise", "traj_xhat", "traj_dhat", "traj_y"]


def _host_controller(spec=None, **kw):
    from libmpc_amd import LMPC
    sp = spec or random_lmpc_spec(3, **kw)
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
    o = _capi.DisturbanceObserverDesc()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---------------------------------------------------------------------------------------------
# the struct and the symbols
# ---------------------------------------------------------------------------------------------
def test_the_descriptor_has_the_size_the_library_reports():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.DisturbanceObserverDesc) == _capi.lib().mpcx_lmpc_disturbance_observer_desc_size()
    assert [f for f, _ in _capi.DisturbanceObserverDesc._fields_] == FIELDS


def test_the_descriptor_has_the_field_offsets_of_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess
    from libmpc_amd import _capi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpcx.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mpcx_lmpc_disturbance_observer_desc));']
    lines += [f'  printf(" %zu", offsetof(mpcx_lmpc_disturbance_observer_desc, {f}));' for f in FIELDS]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_capi.DisturbanceObserverDesc)
    assert got[1:] == [getattr(_capi.DisturbanceObserverDesc, f).offset for f in FIELDS]


def test_the_new_entries_are_exported():
    from libmpc_amd import _capi
    lib = _capi.lib()
    for name in ("mpcx_lmpc_loop_create_offset_free", "mpcx_lmpc_hetero_loop_create_offset_free", "mpcx_lmpc_disturbance_observer_desc_size"):
        assert name in _capi.EXPORTS and getattr(lib, name) is not None, name


# ---------------------------------------------------------------------------------------------
# the refusals, each MPCX_E_INVALID with a message
# ---------------------------------------------------------------------------------------------
def _create(c, d, o):
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    rc = lib.mpcx_lmpc_loop_create_offset_free(c._h, C.byref(d), None if o is None else C.byref(o), C.c_void_p(0x10), C.byref(out))
    msg = lib.mpcx_last_error().decode()
    assert not out.value
    return rc, msg


def test_an_invalid_disturbance_observer_is_refused_with_a_message_on_a_host_only_handle():
    from libmpc_amd import _capi
    c = _host_controller()
    G = np.asfortranarray(np.zeros((4, 2)))
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


def test_a_controller_without_exogenous_inputs_is_refused_on_a_host_only_handle():
    """ndu = 0: there is no disturbance model; the refusal needs the handle's dimensions, not its state (no model has been set)"""
    from libmpc_amd import LMPC, _capi
    c = LMPC(3, 2, 0, 2, 6, 3, device=-1)
    for o in (_observer(gain=np.zeros((3, 2), order="F").ctypes.data), _observer(gain_batch=0x2000)):
        rc, msg = _create(c, _desc(), o)
        assert rc == _capi.E_INVALID and "ndu" in msg, (rc, msg)
    with pytest.raises(ValueError, match="ndu"):
        c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=np.zeros((3, 2)))


def test_a_bank_refuses_one_gain_for_all_and_the_other_invalid_disturbance_observers():
    from libmpc_amd import _capi
    lib = _capi.lib()
    bank = C.c_void_p(0x1000)          # never followed: the descriptor checks come first
    G = np.asfortranarray(np.zeros((4, 2)))

    def create(o):
        out = C.c_void_p()
        rc = lib.mpcx_lmpc_hetero_loop_create_offset_free(bank, C.byref(_desc()), None if o is None else C.byref(o), None, C.c_void_p(0x10), C.byref(out))
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
    assert lib.mpcx_lmpc_hetero_loop_create_offset_free(None, C.byref(_desc()), C.byref(_observer(gain_batch=0x2000)), None, C.c_void_p(0x10),
                                                        C.byref(out)) == _capi.E_INVALID


# ---------------------------------------------------------------------------------------------
# the front-end's shape checks: ValueError ahead of any device call (the handle is host-only: the device layer would raise MpcxError)
# ---------------------------------------------------------------------------------------------
BAD_SHAPES = {          # nx = 3, ndu = 1, ny = 2; B = 4, ticks = 5
    "gain without the disturbance rows": dict(disturbance_observer=np.zeros((3, 2))),
    "gain transposed": dict(disturbance_observer=np.zeros((2, 4))),
    "gain batch": dict(disturbance_observer=np.zeros((5, 4, 2))),
    "gain rows": dict(disturbance_observer=np.zeros((4, 3, 2))),
    "gain 1-D": dict(disturbance_observer=np.zeros(8)),
    "xhat0 batch": dict(disturbance_observer=np.zeros((4, 2)), xhat0=np.zeros((3, 3))),
    "dhat0 batch": dict(disturbance_observer=np.zeros((4, 2)), dhat0=np.zeros((3, 1))),
    "dhat0 cols": dict(disturbance_observer=np.zeros((4, 2)), dhat0=np.zeros((4, 2))),
    "dhat0 1-D": dict(disturbance_observer=np.zeros((4, 4, 2)), dhat0=np.zeros(4)),
    "meas_noise ticks": dict(disturbance_observer=np.zeros((4, 2)), meas_noise=np.zeros((4, 4, 2))),
    "meas_noise outputs": dict(disturbance_observer=np.zeros((4, 4, 2)), meas_noise=np.zeros((5, 4, 3))),
    "dhat0 without a disturbance observer": dict(dhat0=np.zeros((4, 1))),
    "dhat0 with a state observer": dict(observer=np.zeros((3, 2)), dhat0=np.zeros((4, 1))),
    "both observers": dict(observer=np.zeros((3, 2)), disturbance_observer=np.zeros((4, 2))),
}


@pytest.mark.parametrize("bad", sorted(BAD_SHAPES))
def test_a_wrong_shape_raises_a_value_error_before_any_device_call(bad):
    c = _host_controller()
    with pytest.raises(ValueError):
        c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, **BAD_SHAPES[bad])
    with pytest.raises(ValueError):
        c.simulate(np.zeros((4, 3)), np.zeros((4, 2)), 5, **BAD_SHAPES[bad])


def test_both_observers_together_are_refused_by_name():
    c = _host_controller()
    with pytest.raises(ValueError, match="exclude"):
        c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, observer=np.zeros((3, 2)), disturbance_observer=np.zeros((4, 2)))


def test_well_shaped_arguments_reach_the_device_layer():
    from libmpc_amd import MpcxError
    c = _host_controller()
    for gain in (np.zeros((4, 2)), np.zeros((4, 4, 2))):
        with pytest.raises(MpcxError):
            c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=gain, xhat0=np.zeros((4, 3)), dhat0=np.zeros((4, 1)),
                        meas_noise=np.zeros((5, 4, 2)))


def test_the_bank_front_end_refuses_one_gain_for_all_before_any_device_call():
    """LMPCHetero.make_loop's checks need no bank: they are run here on an object that has only the dimensions"""
    from libmpc_amd import LMPCHetero
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h = 3, 2, 2, 1, 6, 0, None
    with pytest.raises(ValueError, match="bank"):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=np.zeros((4, 3, 2)))
    with pytest.raises(ValueError):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=np.zeros((4, 4, 2)), dhat0=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="exclude"):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, observer=np.zeros((4, 3, 2)), disturbance_observer=np.zeros((4, 4, 2)))


def test_results_of_other_loops_keep_their_constructor():
    from libmpc_amd import ClosedLoopResult
    r = ClosedLoopResult(1, 2, 3, 4, 5, 6, 7, 8)
    assert r.xhat is None and r.y is None and r.dhat is None and r.active_count == 8
    r = ClosedLoopResult(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
    assert r.xhat == 9 and r.y == 10 and r.dhat is None


# ---------------------------------------------------------------------------------------------
# the detectability of the augmented pair, checked on the host before any device call (device=-1 handles: a device call would fail otherwise)
# ---------------------------------------------------------------------------------------------
def _covariances(c):
    return 0.01 * np.eye(c.nx), 0.01 * np.eye(c.ndu), 0.04 * np.eye(c.ny)


def test_more_disturbances_than_outputs_are_refused_by_the_rank_check():
    c = _host_controller(ndu=3)                     # ny = 2
    with pytest.raises(ValueError, match="rank") as e:
        c.disturbance_gain(*_covariances(c))
    assert "detectable" in str(e.value) and "nx + ndu" in str(e.value)


def test_a_disturbance_model_that_reaches_nothing_is_refused_by_the_rank_check():
    from libmpc_amd import LMPC
    sp = dict(random_lmpc_spec(3), Bd=np.zeros((3, 1)), Dd=np.zeros((2, 1)))
    c = configure_random(LMPC(*sp["dims"], device=-1), sp)
    with pytest.raises(ValueError, match="rank"):
        c.disturbance_gain(*_covariances(c))


def test_the_bank_names_the_controller_that_fails_the_rank_check():
    """LMPCHetero.disturbance_gains on an object that has only the models: the check is the host's"""
    from libmpc_amd import LMPCHetero
    good, bad = random_lmpc_spec(3), dict(random_lmpc_spec(4), Bd=np.zeros((3, 1)), Dd=np.zeros((2, 1)))
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h = 3, 2, 2, 1, 6, 0, None
    het._models = [(sp["A"], sp["B"], sp["Bd"]) for sp in (good, bad)]
    het._outputs = [sp["C"] for sp in (good, bad)]
    het._feedthrough = [sp["Dd"] for sp in (good, bad)]
    with pytest.raises(ValueError, match="instance 1"):
        het.disturbance_gains(0.01 * np.eye(3), 0.01 * np.eye(1), 0.04 * np.eye(2))


def test_the_size_limit_of_the_riccati_kernel_is_reported_before_any_device_call():
    from libmpc_amd.utils import disturbance_gains
    nx, ndu, ny = 31, 2, 3
    with pytest.raises(ValueError, match="1 <= n <= 32"):
        disturbance_gains(0.5 * np.eye(nx), np.ones((nx, ndu)), np.ones((ny, nx)), np.zeros((ny, ndu)), np.eye(nx), np.eye(ndu), np.eye(ny))
    with pytest.raises(ValueError):
        disturbance_gains(0.5 * np.eye(3), np.ones((4, 1)), np.ones((2, 3)), np.zeros((2, 1)), np.eye(3), np.eye(1), np.eye(2))
