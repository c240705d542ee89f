"""Per-instance plants and bank loops, the host layer without a GPU: the descriptor's new field and its exclusion rule, the null checks of
mpcx_lmpc_hetero_loop_create, and the front-end's own argument checks, which come before any device call."""
import ctypes as C

import numpy as np
import pytest

from helpers import configure_random, random_lmpc_spec


def _host_controller():
    from libmpc_amd import LMPC
    sp = random_lmpc_spec(3)
    return configure_random(LMPC(*sp["dims"], device=-1), sp)


def _desc(**kw):
    """a descriptor that passes every check (no pointer is followed on a host-only handle), then the fields under test"""
    from libmpc_amd import _capi
    d = _capi.LoopDesc()
    d.batch, d.ticks = 4, 3
    d.x0 = d.u0 = d.traj_x = d.traj_u = 0x1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_plant_batch_together_with_a_uniform_plant_is_refused_with_a_message():
    from libmpc_amd import _capi
    lib = _capi.lib()
    c = _host_controller()
    A = np.asfortranarray(np.eye(3))
    for name in ("plant_A", "plant_B", "plant_Bd"):
        out = C.c_void_p()
        d = _desc(plant_batch=0x2000, **{name: A.ctypes.data})
        rc = lib.mpcx_lmpc_loop_create(c._h, C.byref(d), C.c_void_p(0x10), C.byref(out))
        msg = lib.mpcx_last_error().decode()
        assert rc == _capi.E_INVALID and "plant_batch" in msg and not out.value, (name, rc, msg)
    # the descriptor is looked at ahead of the handle's state: with plant_batch alone the host-only handle is what is refused
    out = C.c_void_p()
    rc = lib.mpcx_lmpc_loop_create(c._h, C.byref(_desc(plant_batch=0x2000)), C.c_void_p(0x10), C.byref(out))
    assert rc == _capi.E_STATE and "host-only" in lib.mpcx_last_error().decode()


def test_hetero_loop_create_refuses_null_arguments():
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    d = _desc()
    bank = C.c_void_p(0x1000)          # never followed: the null checks come first
    assert lib.mpcx_lmpc_hetero_loop_create(None, C.byref(d), None, C.c_void_p(0x10), C.byref(out)) == _capi.E_INVALID
    assert lib.mpcx_last_error()
    assert lib.mpcx_lmpc_hetero_loop_create(bank, None, None, C.c_void_p(0x10), C.byref(out)) == _capi.E_INVALID
    assert lib.mpcx_lmpc_hetero_loop_create(bank, C.byref(d), None, C.c_void_p(0x10), None) == _capi.E_INVALID
    assert not out.value


def test_plant_batch_is_the_last_field_of_the_descriptor():
    from libmpc_amd import _capi
    names = [f for f, _ in _capi.LoopDesc._fields_]
    assert "plant_batch" in names and names[-1] == "plant_batch"
    assert _capi.LoopDesc.plant_batch.offset + C.sizeof(C.c_void_p) == C.sizeof(_capi.LoopDesc)
    assert _capi.LoopDesc.plant_batch.offset == max(getattr(_capi.LoopDesc, f).offset for f in names)
    assert C.sizeof(_capi.LoopDesc) == _capi.lib().mpcx_lmpc_loop_desc_size()


def test_plant_and_plants_together_raise_a_value_error():
    c = _host_controller()
    A = np.broadcast_to(np.eye(3), (2, 3, 3))
    with pytest.raises(ValueError):
        c.make_loop(np.zeros((2, 3)), np.zeros((2, 2)), 3, plant=(np.eye(3), None), plants=(A, None, None))
    with pytest.raises(ValueError):
        c.simulate(np.zeros((2, 3)), np.zeros((2, 2)), 3, plant=(np.eye(3), None), plants=(A, None, None))


@pytest.mark.parametrize("bad", ["A batch", "A rows", "B cols", "Bd cols", "four entries"])
def test_a_wrong_plants_shape_raises_a_value_error_before_any_device_call(bad):
    """the handle is host-only: anything that reached the device layer would raise MpcxError instead"""
    c = _host_controller()
    B = 2
    A, Bm, Bd = np.zeros((B, 3, 3)), np.zeros((B, 3, 2)), np.zeros((B, 3, 1))
    plants = {"A batch": (np.zeros((B + 1, 3, 3)), None, None), "A rows": (np.zeros((B, 2, 3)), None, None),
              "B cols": (A, np.zeros((B, 3, 3)), None), "Bd cols": (A, Bm, np.zeros((B, 3, 2))), "four entries": (A, Bm, Bd, Bd)}[bad]
    with pytest.raises(ValueError):
        c.make_loop(np.zeros((B, 3)), np.zeros((B, 2)), 3, plants=plants)
