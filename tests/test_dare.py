"""mpcx_dare_batch and its Python front ends without a GPU: the export, every MPCX_E_INVALID return (checked before anything touches a device:
device = -1 and pointers that are never followed reach them), and the front ends' own shape checks, which raise before any device call."""
import os

import numpy as np
import pytest

from libmpc_amd import _capi


def test_the_symbol_is_exported():
    lib = _capi.lib()
    assert "mpcx_dare_batch" in _capi.EXPORTS and "mpcx_dare_debug_product" in _capi.EXPORTS
    assert lib.mpcx_dare_batch is not None and lib.mpcx_dare_debug_product is not None
    assert (_capi.DARE_CONTROL, _capi.DARE_ESTIMATOR) == (0, 1)
    header = open(os.path.join(os.path.dirname(_capi._HERE), "include", "mpcx.h")).read()
    assert "#define MPCX_DARE_CONTROL   0" in header and "#define MPCX_DARE_ESTIMATOR 1" in header and "int mpcx_dare_batch(" in header


GOOD = dict(device=-1, form=0, n=3, m=2, batch=4, A=0x1000, BorC=0x2000, Q=0x3000, R=0x4000, qper=0, rper=1, X=0x5000, gain=0x6000,
            flags=0x7000, iterations=0x8000, stream=None)
ORDER = ("device", "form", "n", "m", "batch", "A", "BorC", "Q", "R", "qper", "rper", "X", "gain", "flags", "iterations", "stream")


def _call(**kw):
    a = dict(GOOD, **kw)
    return _capi.lib().mpcx_dare_batch(*[a[k] for k in ORDER])


@pytest.mark.parametrize("kw, word", [
    (dict(form=2), "form"), (dict(form=-1), "form"),
    (dict(n=0), "n"), (dict(n=-3), "n"), (dict(n=33), "32"), (dict(m=0), "m"), (dict(m=33), "32"), (dict(n=33, m=33), "32"),
    (dict(batch=-1), "batch"),
    (dict(A=None), "A"), (dict(BorC=None), "BorC"), (dict(Q=None), "Q"), (dict(R=None), "R"), (dict(X=None), "X"),
], ids=lambda v: "-".join("%s=%s" % i for i in v.items()) if isinstance(v, dict) else None)
def test_invalid_arguments_are_refused_before_any_device_call(kw, word):
    assert _call(**kw) == _capi.E_INVALID, kw
    assert word in _capi.lib().mpcx_last_error().decode(), kw


def test_valid_arguments_get_as_far_as_the_device():
    """the same call with nothing wrong with it is not MPCX_E_INVALID: an empty batch returns at once, device = -1 is a device error; gain,
    flags and iterations may be null"""
    assert _call(batch=0) == _capi.OK
    assert _call(batch=0, gain=None, flags=None, iterations=None) == _capi.OK
    assert _call(gain=None, flags=None, iterations=None) == _capi.E_DEVICE
    assert _call(n=32, m=32) == _capi.E_DEVICE and _call(n=1, m=32, form=1) == _capi.E_DEVICE


def test_the_product_form_knob():
    lib = _capi.lib()
    assert lib.mpcx_dare_debug_product(2) == 0 and lib.mpcx_dare_debug_product(7) == 2 and lib.mpcx_dare_debug_product(0) == 2
    assert lib.mpcx_dare_debug_product(0) == 0


def test_front_end_shape_errors():
    from libmpc_amd.utils import dare, kalman_gains, lqr_gains
    rng = np.random.default_rng(0)
    A, B, Cm = rng.normal(size=(4, 3, 3)), rng.normal(size=(4, 3, 2)), rng.normal(size=(4, 2, 3))
    Q, Rm = np.eye(3), np.eye(2)
    bad = [
        (dare, (A, B, Q, Rm, "filter")),                                    # no such form
        (dare, (A[:, :, :2], B, Q, Rm)),                                    # A not square
        (dare, (A, B[:3], Q, Rm)),                                          # batch sizes differ
        (dare, (A, Cm, Q, Rm)),                                             # C where B belongs
        (dare, (A, B, Q, Rm, "estimator")),                                 # B where C belongs
        (dare, (A[0], B, Q, Rm)),                                           # 2-D A with 3-D B
        (dare, (A, B, np.eye(2), Rm)), (dare, (A, B, Q, np.eye(3))),        # Q, R of the wrong size
        (dare, (A, B, np.stack([Q] * 3), Rm)), (dare, (A, B, Q, np.stack([Rm] * 5))),        # per instance, but not one per instance
        (dare, (A, B, Q[0], Rm)),                                           # 1-D
        (dare, (rng.normal(size=(2, 33, 33)), rng.normal(size=(2, 33, 1)), np.eye(33), np.eye(1))),      # n above the limit
        (dare, (A, rng.normal(size=(4, 3, 33)), Q, np.eye(33))),            # m above the limit
        (dare, (np.zeros((2, 0, 0)), np.zeros((2, 0, 1)), np.zeros((0, 0)), np.eye(1))),                   # n = 0
        (kalman_gains, (A, B, Q, Rm)), (lqr_gains, (A, Cm, Q, Rm)),
    ]
    for f, args in bad:
        with pytest.raises(ValueError):
            f(*args)


def test_bank_kalman_gains_shape_errors():
    """LMPCHetero.kalman_gains is utils.kalman_gains on the controllers' own (A, C): the checks come with it.  (A bank needs a device to be
    created, so the bound method is called on a stand-in holding what it reads.)"""
    import types
    from libmpc_amd import LMPCHetero
    rng = np.random.default_rng(1)
    stand_in = types.SimpleNamespace(_models=[(rng.normal(size=(3, 3)), None, None)] * 2, _outputs=[rng.normal(size=(2, 3))] * 2, device=0)
    for Qw, Rv in ((np.eye(2), np.eye(2)), (np.eye(3), np.eye(3)), (np.stack([np.eye(3)] * 3), np.eye(2))):
        with pytest.raises(ValueError):
            LMPCHetero.kalman_gains(stand_in, Qw, Rv)
    with pytest.raises(_capi.MpcxError) as e:
        LMPCHetero.kalman_gains(types.SimpleNamespace(_models=[(None, None, None)], _outputs=[None], device=0), np.eye(3), np.eye(2))
    assert e.value.code == _capi.E_STATE
