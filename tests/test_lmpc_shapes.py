"""The workloads of test_lmpc_shapes_gpu.py reach the edges they are there for: working sets on both sides of the lean kernels'
16 rows and of the fallback polish's register / LDS capacities, and every template variant of the solve kernels.  Oracle and host
set-up only (no GPU), so that the GPU tests cannot silently stop reaching those branches."""
import numpy as np
import pytest

from helpers import SHAPES_EDGES as SHAPES, SHAPES_MAIN as MAIN, SHAPES_MAXIT as MAXIT, SHAPES_VARIANTS as VARIANTS
from helpers import axes_batch, axes_spec, configure_axes, oracle_batch_parallel_spec


@pytest.fixture(scope="module")
def main_ref():
    sp = axes_spec(*MAIN[:2])
    x0, u0, _ = axes_batch(sp, MAIN[2])
    return oracle_batch_parallel_spec(sp, x0, u0, maximum_iteration=MAXIT)


def test_main_batch_fills_every_working_set_bucket(main_ref):
    na = main_ref["n_active"]
    B = len(na)
    assert B == 1024
    small, mid, big = (na <= 16).mean(), ((na > 16) & (na <= 28)).mean(), (na > 28).mean()
    assert small >= 0.10 and mid >= 0.10 and big >= 0.10, (small, mid, big)
    assert (na == 16).any() and (na == 17).any()                  # both sides of the lean kernels' capacity
    assert (main_ref["polished"] == 1).mean() >= 0.95
    assert (main_ref["status"] == 0).all()


def _host(spec):
    from libmpc_amd import LMPC
    return configure_axes(LMPC(*spec["dims"], device=-1), spec, MAXIT)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variant_shapes_select_their_kernel_template(name):
    """the condensed sizes put each shape in the template it is named for: <1,1> up to 128 variables and rows, <2,2> to 256, <4,4> to 512;
    'ldg' is sized by its constraint rows, not its variables"""
    kw, want, cost_direct = VARIANTS[name]
    sp = axes_spec(**kw)
    i = _host(sp).info()
    nz, mg = i["nz"], i["mg"]
    ldz, ldg = nz + (nz & 1), mg + (mg & 1)
    n = max(ldz, ldg)
    got = 1 if n <= 128 else (2 if n <= 256 else (4 if n <= 512 else -1))
    assert got == want and i["kernel_variant"] == want, (nz, mg, i["kernel_variant"])
    if name == "ldg":
        assert ldz <= 128 < ldg
    assert int(_host(sp).debug_get("flags")[0]) == cost_direct


def test_shape_edges_cover_what_they_name():
    dims = {k: axes_spec(**kw)["dims"] for k, kw in SHAPES.items()}
    nus = {d[1] for d in dims.values()}
    assert {1, 3, 5} <= nus
    assert any(d[0] % 4 for d in dims.values())
    assert any(d[3] < d[0] for d in dims.values()) and any(d[3] > d[0] for d in dims.values())
    assert any(d[5] < d[4] for d in dims.values())
    nzs = {_host(axes_spec(**kw)).info()["nz"] for k, kw in SHAPES.items() if k.startswith("nz")}
    assert nzs == {47, 48, 49}
    sp = axes_spec(**SHAPES["kin72"])
    kin = int(_host(sp).debug_get("dims_maps")[0])
    assert kin > 64, kin


def test_too_large_a_controller_is_refused_on_the_host():
    from libmpc_amd import LMPC
    from libmpc_amd._capi import MpcxError, E_UNSUPPORTED
    sp = axes_spec(11, 50)
    c = configure_axes(LMPC(*sp["dims"], device=-1), sp, MAXIT)
    with pytest.raises(MpcxError) as e:
        c.info()
    assert e.value.code == E_UNSUPPORTED
