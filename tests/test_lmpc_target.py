"""Steady-state targets, the host layer without a GPU: the target descriptor's mirror, the exports, the refusals of
mpcx_lmpc_loop_create_offset_free_target / mpcx_lmpc_hetero_loop_create_offset_free_target (ahead of any look at the handle's or the bank's
state, so a host-only handle and a bank pointer that is never followed reach them), the argument checks of mpcx_target_map_batch and
mpcx_target_apply_batch with the LDS limit among them, the front-end's shape checks and the two rank conditions, all of which come before any
device call."""
import ctypes as C

import numpy as np
import pytest

from helpers import configure_random, random_lmpc_spec

FIELDS = ["map", "map_batch", "traj_us"]
NEW = ("mpcx_lmpc_loop_create_offset_free_target", "mpcx_lmpc_hetero_loop_create_offset_free_target", "mpcx_lmpc_target_desc_size",
       "mpcx_target_map_batch", "mpcx_target_apply_batch")


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


def _target(**kw):
    from libmpc_amd import _capi
    t = _capi.TargetDesc()
    for k, v in kw.items():
        setattr(t, k, v)
    return t


# ---------------------------------------------------------------------------------------------
# the struct and the symbols
# ---------------------------------------------------------------------------------------------
def test_the_descriptor_has_the_size_the_library_reports():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.TargetDesc) == _capi.lib().mpcx_lmpc_target_desc_size()
    assert [f for f, _ in _capi.TargetDesc._fields_] == FIELDS


def test_the_descriptor_has_the_field_offsets_of_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess
    from libmpc_amd import _capi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpcx.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mpcx_lmpc_target_desc));']
    lines += [f'  printf(" %zu", offsetof(mpcx_lmpc_target_desc, {f}));' for f in FIELDS]
    lines += ['  printf(" %zu", sizeof(mpcx_lmpc_disturbance_observer_desc));', '  return 0;', '}']
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_capi.TargetDesc)
    assert got[1:-1] == [getattr(_capi.TargetDesc, f).offset for f in FIELDS]
    assert got[-1] == C.sizeof(_capi.DisturbanceObserverDesc)          # the existing descriptor is frozen


def test_the_new_entries_are_exported_and_declared():
    import os
    from libmpc_amd import _capi
    lib = _capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcx.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTS and getattr(lib, name) is not None, name
        assert name + "(" in header, name


# ---------------------------------------------------------------------------------------------
# the refusals of the create entries, each MPCX_E_INVALID with a message
# ---------------------------------------------------------------------------------------------
def _create(c, d, o, t):
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    rc = lib.mpcx_lmpc_loop_create_offset_free_target(c._h, C.byref(d), None if o is None else C.byref(o), None if t is None else C.byref(t),
                                                      C.c_void_p(0x10), C.byref(out))
    msg = lib.mpcx_last_error().decode()
    assert not out.value
    return rc, msg


def test_an_invalid_target_is_refused_with_a_message_on_a_host_only_handle():
    from libmpc_amd import _capi
    c = _host_controller()                         # nx = 3, nu = 2, ndu = 1, ny = 2
    G = np.asfortranarray(np.zeros((4, 2)))
    T = np.asfortranarray(np.zeros((2, 5)))
    good = _observer(gain=G.ctypes.data)
    rc, msg = _create(c, _desc(), good, None)
    assert rc == _capi.E_INVALID and "target" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), good, _target())
    assert rc == _capi.E_INVALID and "map" in msg and "map_batch" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), good, _target(map=T.ctypes.data, map_batch=0x2000))
    assert rc == _capi.E_INVALID and "map_batch" in msg and "exclude" in msg, (rc, msg)
    # everything the offset-free entry refuses, in its order: the loop descriptor, then the observer, then the target
    rc, msg = _create(c, _desc(ticks=0), None, None)
    assert rc == _capi.E_INVALID and "ticks" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), None, _target(map=T.ctypes.data))
    assert rc == _capi.E_INVALID and "observer" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), _observer(), _target(map=T.ctypes.data))
    assert rc == _capi.E_INVALID and "gain" in msg, (rc, msg)
    rc, msg = _create(c, _desc(), _observer(gain=G.ctypes.data, gain_batch=0x2000), _target(map=T.ctypes.data))
    assert rc == _capi.E_INVALID and "exclude" in msg, (rc, msg)
    # the handle's state last: a good descriptor on a host-only handle is a state error
    for t in (_target(map=T.ctypes.data), _target(map_batch=0x2000), _target(map_batch=0x2000, traj_us=0x3000)):
        rc, msg = _create(c, _desc(), good, t)
        assert rc == _capi.E_STATE and "host-only" in msg, (rc, msg)


def test_a_controller_without_exogenous_inputs_is_refused_on_a_host_only_handle():
    from libmpc_amd import LMPC, _capi
    c = LMPC(3, 2, 0, 2, 6, 3, device=-1)
    rc, msg = _create(c, _desc(), _observer(gain_batch=0x2000), _target(map_batch=0x2000))
    assert rc == _capi.E_INVALID and "ndu" in msg, (rc, msg)


def test_a_bank_refuses_one_map_for_all_and_the_other_invalid_targets():
    from libmpc_amd import _capi
    lib = _capi.lib()
    bank = C.c_void_p(0x1000)          # never followed: the descriptor checks come first
    T = np.asfortranarray(np.zeros((2, 5)))
    good = _observer(gain_batch=0x2000)

    def create(o, t, f=bank):
        out = C.c_void_p()
        rc = lib.mpcx_lmpc_hetero_loop_create_offset_free_target(f, C.byref(_desc()), None if o is None else C.byref(o),
                                                                 None if t is None else C.byref(t), None, C.c_void_p(0x10), C.byref(out))
        assert not out.value
        return rc, lib.mpcx_last_error().decode()
    rc, msg = create(good, _target(map=T.ctypes.data))
    assert rc == _capi.E_INVALID and "bank" in msg and "map_batch" in msg, (rc, msg)
    rc, msg = create(good, None)
    assert rc == _capi.E_INVALID and "target" in msg, (rc, msg)
    rc, msg = create(good, _target())
    assert rc == _capi.E_INVALID and "map" in msg, (rc, msg)
    rc, msg = create(good, _target(map=T.ctypes.data, map_batch=0x2000))
    assert rc == _capi.E_INVALID and "exclude" in msg, (rc, msg)
    rc, msg = create(_observer(gain=T.ctypes.data), _target(map_batch=0x2000))
    assert rc == _capi.E_INVALID and "gain_batch" in msg, (rc, msg)
    rc, msg = create(None, _target(map_batch=0x2000))
    assert rc == _capi.E_INVALID and "observer" in msg, (rc, msg)
    assert create(good, _target(map_batch=0x2000), f=None)[0] == _capi.E_INVALID


# ---------------------------------------------------------------------------------------------
# mpcx_target_map_batch / mpcx_target_apply_batch: every refusal comes before anything touches a device (the pointers are never followed)
# ---------------------------------------------------------------------------------------------
def _map_call(nx=3, nu=2, ndu=1, ny=2, batch=4, **null):
    from libmpc_amd import _capi
    lib = _capi.lib()
    p = dict(A=0x1000, B=0x1000, Bd=0x1000, C=0x1000, Dd=0x1000, map_u=0x1000, map_x=None, flags=None)
    p.update(null)
    rc = lib.mpcx_target_map_batch(0, nx, nu, ndu, ny, batch, p["A"], p["B"], p["Bd"], p["C"], p["Dd"], p["map_u"], p["map_x"], p["flags"], None)
    return rc, lib.mpcx_last_error().decode()


@pytest.mark.parametrize("kw", [dict(nx=0), dict(nu=0), dict(ny=0), dict(ndu=-1), dict(batch=-1), dict(A=None), dict(B=None), dict(C=None),
                                dict(map_u=None), dict(Bd=None), dict(Dd=None)], ids=lambda k: "%s=%s" % next(iter(k.items())))
def test_invalid_map_arguments_are_refused_before_any_device_call(kw):
    from libmpc_amd import _capi
    rc, msg = _map_call(**kw)
    assert rc == _capi.E_INVALID and msg, (rc, msg)


def test_no_disturbance_model_needs_no_disturbance_matrices_and_an_empty_batch_is_fine():
    from libmpc_amd import _capi
    assert _map_call(ndu=0, Bd=None, Dd=None, batch=0)[0] == _capi.OK
    assert _map_call(batch=0)[0] == _capi.OK


def test_past_the_lds_limit_the_shape_is_unsupported():
    """(58, 8, 4, 8) is the largest tested shape: 132 x 152 doubles = 160 512 bytes of the 163 840 a workgroup may request; one more state is
    134 x 154 doubles = 165 088 bytes.  The check precedes every device call (batch = 0 returns behind it)."""
    from libmpc_amd import _capi
    assert _map_call(58, 8, 4, 8, batch=0)[0] == _capi.OK
    rc, msg = _map_call(59, 8, 4, 8, batch=0)
    assert rc == _capi.E_UNSUPPORTED and "LDS" in msg, (rc, msg)
    rc, msg = _map_call(200, 2, 1, 2)
    assert rc == _capi.E_UNSUPPORTED and "LDS" in msg, (rc, msg)
    assert _map_call(1 << 20, 1 << 20, 1, 1)[0] == _capi.E_UNSUPPORTED          # (no overflow on the way to the comparison)


@pytest.mark.parametrize("kw", [dict(nu=0), dict(ny=0), dict(ndu=-1), dict(batch=-1), dict(map_u=None), dict(r=None), dict(ubar=None),
                                dict(us=None), dict(dhat=None)], ids=lambda k: "%s=%s" % next(iter(k.items())))
def test_invalid_product_arguments_are_refused_before_any_device_call(kw):
    from libmpc_amd import _capi
    lib = _capi.lib()
    p = dict(nu=2, ndu=1, ny=2, batch=4, map_u=0x1000, r=0x1000, dhat=0x1000, ubar=0x1000, us=0x1000)
    p.update(kw)
    rc = lib.mpcx_target_apply_batch(0, p["nu"], p["ndu"], p["ny"], p["batch"], p["map_u"], 1, p["r"], p["dhat"], p["ubar"], p["us"], None)
    assert rc == _capi.E_INVALID and lib.mpcx_last_error().decode(), rc


# ---------------------------------------------------------------------------------------------
# the front-end's checks: ValueError ahead of any device call (the handle is host-only: the device layer would raise MpcxError)
# ---------------------------------------------------------------------------------------------
GAIN = np.zeros((4, 2))
BAD_SHAPES = {          # nx = 3, nu = 2, ndu = 1, ny = 2: nrhs = 5; B = 4, ticks = 5
    "map transposed": dict(disturbance_observer=GAIN, target=np.zeros((5, 2))),
    "map without ubar's columns": dict(disturbance_observer=GAIN, target=np.zeros((2, 3))),
    "map batch": dict(disturbance_observer=GAIN, target=np.zeros((5, 2, 5))),
    "map rows": dict(disturbance_observer=GAIN, target=np.zeros((4, 3, 5))),
    "map 1-D": dict(disturbance_observer=GAIN, target=np.zeros(10)),
    "target without a disturbance observer": dict(target=np.zeros((2, 5))),
    "target with a state observer": dict(observer=np.zeros((3, 2)), target=np.zeros((2, 5))),
}


@pytest.mark.parametrize("bad", sorted(BAD_SHAPES))
def test_a_wrong_shape_raises_a_value_error_before_any_device_call(bad):
    c = _host_controller()
    with pytest.raises(ValueError):
        c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, **BAD_SHAPES[bad])
    with pytest.raises(ValueError):
        c.simulate(np.zeros((4, 3)), np.zeros((4, 2)), 5, **BAD_SHAPES[bad])


def test_a_target_without_a_disturbance_observer_is_refused_by_name():
    c = _host_controller()
    with pytest.raises(ValueError, match="disturbance_observer"):
        c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, target=np.zeros((2, 5)))


def test_well_shaped_arguments_reach_the_device_layer():
    from libmpc_amd import MpcxError
    c = _host_controller()
    for target in (np.zeros((2, 5)), np.zeros((4, 2, 5))):
        with pytest.raises(MpcxError):
            c.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=GAIN, target=target)


def test_the_bank_front_end_refuses_one_map_for_all_before_any_device_call():
    """LMPCHetero.make_loop's checks need no bank: they are run here on an object that has only the dimensions"""
    from libmpc_amd import LMPCHetero
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h = 3, 2, 2, 1, 6, 0, None
    gains = np.zeros((4, 4, 2))
    with pytest.raises(ValueError, match="bank"):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=gains, target=np.zeros((2, 5)))
    with pytest.raises(ValueError):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, disturbance_observer=gains, target=np.zeros((4, 2, 4)))
    with pytest.raises(ValueError, match="disturbance_observer"):
        het.make_loop(np.zeros((4, 3)), np.zeros((4, 2)), 5, target=np.zeros((4, 2, 5)))


def test_results_of_other_loops_keep_their_constructor():
    from libmpc_amd import ClosedLoopResult
    r = ClosedLoopResult(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
    assert r.dhat == 11 and r.us is None
    assert ClosedLoopResult(1, 2, 3, 4, 5, 6, 7, 8, us=12).us == 12


# ---------------------------------------------------------------------------------------------
# the two rank conditions, checked on the host before any device call (a device call would fail here: these tests run without a GPU)
# ---------------------------------------------------------------------------------------------
def _model(nx=3, nu=2, ndu=1, ny=2, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(nx, nx)); A *= 0.8 / max(abs(np.linalg.eigvals(A)))
    return A, rng.normal(size=(nx, nu)), rng.normal(size=(nx, ndu)), rng.normal(size=(ny, nx)), rng.normal(size=(ny, ndu))


def test_more_outputs_than_inputs_are_refused_by_the_reachability_rank():
    from libmpc_amd.utils import target_maps
    with pytest.raises(ValueError, match="rank") as e:
        target_maps(*_model(nu=1, ny=2))
    assert "[[I - A, -B], [C, 0]]" in str(e.value) and "reached" in str(e.value) and "instance 0" in str(e.value)


def test_an_input_matrix_that_reaches_nothing_is_refused_by_the_reachability_rank():
    from libmpc_amd.utils import target_maps
    A, B, Bd, Cm, Dd = _model()
    with pytest.raises(ValueError, match=r"\[\[I - A, -B\], \[C, 0\]\]"):
        target_maps(A, np.zeros_like(B), Bd, Cm, Dd)


def test_an_unobservable_integrator_is_refused_by_the_observability_rank():
    """A has the eigenvalue 1 with an eigenvector C does not see.  That is a zero column of S; with an input to spare (nu = 3 > ny = 2) S keeps
    its row rank all the same, and only the second condition fails"""
    from libmpc_amd.utils import target_maps
    A = np.diag([1.0, 0.5, 0.25]); B = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    Cm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    S = np.block([[np.eye(3) - A, -B], [Cm, np.zeros((2, 3))]])
    assert np.linalg.matrix_rank(S) == 5
    with pytest.raises(ValueError, match="rank") as e:
        target_maps(A, B, np.ones((3, 1)), Cm, np.zeros((2, 1)))
    assert "[I - A; C]" in str(e.value) and "integrator" in str(e.value)


def test_the_instance_that_fails_is_named_and_shapes_are_checked():
    from libmpc_amd.utils import steady_state_inputs, target_maps
    good, bad = _model(seed=1), _model(seed=2)
    stack = [np.stack([g, b]) for g, b in zip(good, bad)]
    stack[1][1] = 0.0
    with pytest.raises(ValueError, match="instance 1"):
        target_maps(*stack)
    A, B, Bd, Cm, Dd = good
    for args in ((A, B[:2], Bd, Cm, Dd), (A, B, Bd, Cm[:, :2], Dd), (A, B, Bd, Cm, np.zeros((2, 2))), (A[:2], B, Bd, Cm, Dd),
                 (A, B, np.zeros((2, 1)), Cm, Dd)):
        with pytest.raises(ValueError):
            target_maps(*args)
    for args in ((np.zeros((2, 4)), np.zeros((4, 2)), np.zeros((4, 1)), np.zeros((4, 2))),
                 (np.zeros((3, 2, 5)), np.zeros((4, 2)), np.zeros((4, 1)), np.zeros((4, 2))),
                 (np.zeros((2, 5)), np.zeros((4, 2)), np.zeros((3, 1)), np.zeros((4, 2))),
                 (np.zeros((2, 5)), np.zeros(2), np.zeros((4, 1)), np.zeros((4, 2)))):
        with pytest.raises(ValueError):
            steady_state_inputs(*args)


def test_the_controller_and_the_bank_run_the_rank_check_on_their_own_models():
    from libmpc_amd import LMPC, LMPCHetero
    sp = dict(random_lmpc_spec(3), B=np.zeros((3, 2)))
    c = configure_random(LMPC(*sp["dims"], device=-1), sp)
    with pytest.raises(ValueError, match="rank"):
        c.target_map()
    good = random_lmpc_spec(3)
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h = 3, 2, 2, 1, 6, 0, None
    het._models = [(s["A"], s["B"], s["Bd"]) for s in (good, sp)]
    het._outputs = [s["C"] for s in (good, sp)]
    het._feedthrough = [s["Dd"] for s in (good, sp)]
    with pytest.raises(ValueError, match="instance 1"):
        het.target_maps()
