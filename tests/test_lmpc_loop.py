"""The closed loop's host layer without a GPU: every validation error of mpcx_lmpc_loop_create on a host-only handle comes back with its
code and a message, and the Python mirror of the descriptor has the size the library reports."""
import ctypes as C

import numpy as np
import pytest

from helpers import configure_random, random_lmpc_spec


def _host_controller(with_model=True):
    from libmpc_amd import LMPC
    sp = random_lmpc_spec(3)
    c = LMPC(*sp["dims"], device=-1)
    if with_model:
        configure_random(c, sp)
    return c


def _desc(**kw):
    """a descriptor that passes every check (the pointers are never followed on a host-only handle), then the fields under test"""
    from libmpc_amd import _capi
    d = _capi.LoopDesc()
    d.batch, d.ticks = 4, 3
    d.x0 = d.u0 = d.traj_x = d.traj_u = 0x1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _create(c, d):
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    rc = lib.mpcx_lmpc_loop_create(c._h, C.byref(d), C.c_void_p(0x10), C.byref(out))
    msg = lib.mpcx_last_error().decode()
    assert not out.value
    return rc, msg


BAD = {
    "ticks zero": dict(ticks=0), "ticks negative": dict(ticks=-2),
    "batch zero": dict(batch=0), "batch negative": dict(batch=-1),
    "x0 null": dict(x0=None), "u0 null": dict(u0=None), "traj_x null": dict(traj_x=None), "traj_u null": dict(traj_u=None),
    "yref mode": dict(yref_mode=4), "uref mode": dict(uref_mode=-1), "duref mode": dict(duref_mode=7), "dmeas mode": dict(dmeas_mode=99),
    "yref missing": dict(yref_mode=1), "uref missing": dict(uref_mode=2), "duref missing": dict(duref_mode=3), "dmeas preview missing": dict(dmeas_mode=3),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_an_invalid_descriptor_is_refused_with_a_message(name):
    from libmpc_amd import _capi
    rc, msg = _create(_host_controller(), _desc(**BAD[name]))
    assert rc == _capi.E_INVALID, (name, rc, msg)
    assert msg, name


def test_a_handle_that_cannot_run_a_loop_is_a_state_error():
    from libmpc_amd import _capi
    rc, msg = _create(_host_controller(with_model=False), _desc())
    assert rc == _capi.E_STATE and "model" in msg, (rc, msg)
    rc, msg = _create(_host_controller(), _desc())
    assert rc == _capi.E_STATE and "host-only" in msg, (rc, msg)
    # the descriptor is looked at first: a bad one on a handle without a model is still a bad descriptor
    rc, msg = _create(_host_controller(with_model=False), _desc(ticks=0))
    assert rc == _capi.E_INVALID and msg, (rc, msg)


def test_null_arguments_and_null_loops():
    from libmpc_amd import _capi
    lib = _capi.lib()
    c = _host_controller()
    out = C.c_void_p()
    assert lib.mpcx_lmpc_loop_create(c._h, None, C.c_void_p(0x10), C.byref(out)) == _capi.E_INVALID and lib.mpcx_last_error()
    assert lib.mpcx_lmpc_loop_create(None, C.byref(_desc()), C.c_void_p(0x10), C.byref(out)) == _capi.E_INVALID
    assert lib.mpcx_lmpc_loop_run(None, None) == _capi.E_INVALID and lib.mpcx_last_error()
    assert lib.mpcx_lmpc_loop_debug_replay(None, None) == _capi.E_INVALID
    assert lib.mpcx_lmpc_loop_destroy(None) == _capi.OK


def test_the_python_descriptor_has_the_size_the_library_reports():
    from libmpc_amd import _capi
    assert C.sizeof(_capi.LoopDesc) == _capi.lib().mpcx_lmpc_loop_desc_size()
    assert _capi.REF_PREVIEW == 3


def test_the_python_descriptor_has_the_field_offsets_of_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess
    from libmpc_amd import _capi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpcx.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mpcx_lmpc_loop_desc));']
    lines += [f'  printf(" %zu", offsetof(mpcx_lmpc_loop_desc, {f}));' for f, _ in _capi.LoopDesc._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_capi.LoopDesc)
    assert got[1:] == [getattr(_capi.LoopDesc, f).offset for f, _ in _capi.LoopDesc._fields_]


def test_the_front_end_raises_without_a_device():
    from libmpc_amd import MpcxError
    c = _host_controller()
    with pytest.raises(MpcxError):
        c.simulate(np.zeros((2, 3)), np.zeros((2, 2)), 3)
