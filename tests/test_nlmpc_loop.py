"""The NLMPC closed loop's host layer without a GPU (a controller handle needs a device, so only what a null handle reaches): the library
exports the new entry points, the Python mirror of the descriptor has the size and the field offsets of the C header, null arguments come
back with their code and a message.  What needs a handle is in test_nlmpc_loop_gpu.py."""
import ctypes as C

import pytest

NEW = ("mpcx_nlmpc_loop_create", "mpcx_nlmpc_loop_run", "mpcx_nlmpc_loop_destroy", "mpcx_nlmpc_loop_desc_size", "mpcx_nlmpc_loop_debug_replay",
       "mpcx_nlmpc_loop_debug_tick", "mpcx_nlmpc_plant_step_batch")


def _desc(**kw):
    """a descriptor that passes every check (no pointer is followed before the handle has been looked at), then the fields under test"""
    from libmpc_amd import _capi
    d = _capi.NlmpcLoopDesc()
    d.batch, d.ticks, d.substeps, d.warm = 4, 3, 1, 1
    d.x0 = d.u0 = d.traj_x = d.traj_u = 0x1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_library_exports_the_new_symbols():
    from libmpc_amd import _capi
    lib = _capi.lib()
    for name in NEW:
        getattr(lib, name)
        assert name in _capi.EXPORTS


def test_the_python_descriptor_has_the_size_the_library_reports():
    from libmpc_amd import _capi
    assert _capi.lib().mpcx_nlmpc_loop_desc_size() == C.sizeof(_capi.NlmpcLoopDesc)


def test_the_python_descriptor_has_the_field_offsets_of_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess
    from libmpc_amd import _capi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpcx.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mpcx_nlmpc_loop_desc));']
    lines += [f'  printf(" %zu", offsetof(mpcx_nlmpc_loop_desc, {f}));' for f, _ in _capi.NlmpcLoopDesc._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_capi.NlmpcLoopDesc)
    assert got[1:] == [getattr(_capi.NlmpcLoopDesc, f).offset for f, _ in _capi.NlmpcLoopDesc._fields_]


def test_null_arguments_are_refused_with_a_message():
    from libmpc_amd import _capi
    lib = _capi.lib()
    out = C.c_void_p()
    stream = C.c_void_p(0x10)
    fake = C.c_void_p(0x2000)            # stands for a handle where the argument under test is looked at first: never followed

    def refused(rc):
        assert rc == _capi.E_INVALID, rc
        assert lib.mpcx_last_error().decode()

    refused(lib.mpcx_nlmpc_loop_create(None, C.byref(_desc()), stream, C.byref(out)))            # null handle
    refused(lib.mpcx_nlmpc_loop_create(fake, None, stream, C.byref(out)))                        # null descriptor
    refused(lib.mpcx_nlmpc_loop_create(fake, C.byref(_desc()), stream, None))                    # null out argument
    refused(lib.mpcx_nlmpc_loop_create(None, None, stream, None))
    assert not out.value
    refused(lib.mpcx_nlmpc_loop_run(None, stream))
    refused(lib.mpcx_nlmpc_loop_debug_replay(None, stream))
    tick = C.c_int(-1)
    refused(lib.mpcx_nlmpc_loop_debug_tick(None, C.byref(tick)))
    refused(lib.mpcx_nlmpc_plant_step_batch(None, 4, C.c_void_p(0x1000), C.c_void_p(0x1000), None, None, 1, C.c_void_p(0x1000), stream))


def test_destroying_a_null_loop_is_ok():
    from libmpc_amd import _capi
    assert _capi.lib().mpcx_nlmpc_loop_destroy(None) == _capi.OK
