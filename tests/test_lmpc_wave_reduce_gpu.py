"""The wave-wide sums of the lean LMPC kernels (csrc/lmpc_fast.hip): wave_sum_full -- lane swaps and DPP moves -- against the ds_bpermute
butterfly it replaces on the path outside the rounds, and the two-level sum of lmpc_solve_group's head in both forms, through
mpcx_lmpc_debug_wave_reduce: one wavefront per vector of 64 values, every lane of every form returned.  The new forms keep the butterfly's
pairing tree, so every lane must carry the butterfly's bits: compared as 64-bit patterns, a NaN matching any NaN."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NVEC = 512


def _vectors():
    r = np.random.default_rng(1311)
    sign = lambda shape: np.where(r.random(shape) < 0.5, -1.0, 1.0)
    parts = []
    # mixed magnitudes, 1e-300 .. 1e300
    parts.append(sign((128, 64)) * 10.0 ** r.uniform(-300, 300, size=(128, 64)))
    # sums that cancel to a few ulps: 32 values and their negatives, each off by 0..3 ulps, in a random lane order
    a = sign((128, 32)) * 10.0 ** r.uniform(-3, 3, size=(128, 32))
    b = -a * (1.0 + r.integers(0, 4, size=(128, 32)) * np.finfo(float).eps)
    c = np.concatenate([a, b], axis=1)
    parts.append(np.take_along_axis(c, np.argsort(r.random((128, 64)), axis=1), axis=1))
    # signed zeros: all +0, all -0, mixtures, and a few lanes with a value and its negative
    z = np.where(r.random((64, 64)) < 0.5, -0.0, 0.0)
    z[0] = 0.0; z[1] = -0.0
    z[2:16, 5] = 1.5; z[2:16, 37] = -1.5
    parts.append(z)
    # denormals
    parts.append(sign((64, 64)) * r.integers(0, 1 << 20, size=(64, 64)) * 5e-324)
    # one +-inf, one NaN
    inf = sign((64, 64)) * 10.0 ** r.uniform(-5, 5, size=(64, 64))
    inf[np.arange(64), r.integers(0, 64, size=64)] = np.where(np.arange(64) % 2 == 0, np.inf, -np.inf)
    parts.append(inf)
    nan = sign((64, 64)) * 10.0 ** r.uniform(-5, 5, size=(64, 64))
    nan[np.arange(64), np.arange(64)] = np.nan          # every lane position once
    parts.append(nan)
    v = np.ascontiguousarray(np.concatenate(parts, axis=0))
    assert v.shape == (NVEC, 64)
    return v


def _butterfly(v, levels):
    """the pairing tree of the __shfl_xor butterfly in IEEE double arithmetic"""
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for o in levels:
            v = v + v[:, lane ^ o]
    return v


def _same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def forms():
    import torch
    from libmpc_amd import _capi
    lib = _capi.lib()
    v = _vectors()
    d_in = torch.from_numpy(v).cuda()
    d_out = torch.zeros((NVEC, 4, 64), dtype=torch.float64, device="cuda")
    _capi.check(lib.mpcx_lmpc_debug_wave_reduce(C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), NVEC, None))
    torch.cuda.synchronize()
    return v, d_out.cpu().numpy()


def test_the_symbol_is_exported():
    from libmpc_amd import _capi
    assert "mpcx_lmpc_debug_wave_reduce" in _capi.EXPORTS


@pytest.mark.parametrize("old,new,levels", [(0, 1, (32, 16, 8, 4, 2, 1)), (2, 3, (16, 32))], ids=["wave_sum_full", "two_level"])
def test_every_lane_bit_for_bit(forms, old, new, levels):
    v, out = forms
    same = _same_bits(out[:, new], out[:, old])
    assert same.all(), ("vector, lane", np.argwhere(~same)[:8].tolist())
    # ... and the old form is the tree this test believes it is
    tree = _same_bits(out[:, old], _butterfly(v, levels))
    assert tree.all(), ("vector, lane", np.argwhere(~tree)[:8].tolist())
    # the six-level sum is the same in every lane; the two-level one within its four lanes
    if new == 1:
        assert _same_bits(out[:, new], np.repeat(out[:, new, :1], 64, axis=1)).all()


def test_the_vectors_reach_the_edges(forms):
    v, out = forms
    full = out[:, 0, 0]
    assert np.isnan(full[448:]).all() and np.isinf(full[384:448]).all()
    assert (np.abs(v[320:384]) < 2.3e-308).all() and (v[320:384] != 0).any()
    assert np.signbit(full[257]) and full[257] == 0 and not np.signbit(full[256])
    scale = np.abs(v[128:256]).max(axis=1)
    assert (np.abs(full[128:256]) <= 64 * 4 * np.finfo(float).eps * scale).all()
