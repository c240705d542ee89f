"""-m gpu: the discretisation kernel (mpcx_discretize_batch, kernel c2d_expm of libmpc_amd/csrc/c2d_kernels.hip, libmpc_amd.utils.discretization)
at every shape and edge it has, against the 60-digit truths of tests/golden/c2d_truth.npz (tests/golden/make_c2d_golden.py).

The accuracy check is element-wise, |out - E| <= 3 n 2^-52 2^s max(1, max|E|) with s the documented number of squarings (tests/c2d_ref.py has
the derivation); the chain and zero families must come out bit-exact.  Beside it: the LDS limit (n = 45 is the last shape under 64 KiB, 46 and
48 are over it, 49 is refused), the grid-stride loop (more than 4096 instances: a block computes a second instance in the LDS of the first),
shared against per-instance sampling times, a non-finite neighbour, the C ABI's argument checks and the Python front end's forms of Ts."""
import numpy as np
import pytest

import c2d_ref as R
from oracle.utils_numpy import discretization as ref_c2d

pytestmark = pytest.mark.gpu


def _run(A, B, Ts):
    """numpy in, numpy out, through the Python front end"""
    import torch
    from libmpc_amd.utils import discretization
    Ad, Bd = discretization(torch.from_numpy(np.array(A, dtype=float)), torch.from_numpy(np.array(B, dtype=float)),
                            torch.from_numpy(np.array(Ts, dtype=float)) if isinstance(Ts, np.ndarray) else Ts)
    torch.cuda.synchronize()
    return Ad.cpu().numpy(), Bd.cpu().numpy()


def _equal(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("name", [f for f in R.FAMILIES if f != "be"])
def test_family_against_the_truth(name):
    c = R.case(name)
    Ad, Bd = _run(c["A"], c["B"], c["Ts"])
    R.check_family(name, Ad, Bd)


def test_disturbance_matrix_appended_to_b():
    """Utils.hpp:63-89 through the same call: [B Be] in, [Bd Bed] out"""
    c = R.case("be")
    Ad, Bd = _run(c["A"], np.concatenate([c["B2"], c["Be"]], axis=2), c["Ts"])
    R.check_family("be", Ad, Bd)
    # ... and B's own columns do not depend on what is appended
    Ad2, Bd2 = _run(c["A"], c["B2"], c["Ts"])
    b = R.bound(c["A"], c["B"], c["Ts"], c["Ad"], c["Bd"])[:, None, None]
    assert (np.abs(Ad2 - c["Ad"]) <= b).all() and (np.abs(Bd2 - c["Bd"][:, :, :2]) <= b).all()


def test_the_lds_limit():
    """n = 45, 46, 48 run and meet the bound (the families limit_*); n = 49 is refused with MPCX_E_UNSUPPORTED and leaves the process usable"""
    from libmpc_amd import _capi
    for name in R.LIMIT:
        c = R.case(name)
        R.check_family(name, *_run(c["A"], c["B"], c["Ts"]))
    rng = np.random.default_rng(49)
    with pytest.raises(_capi.MpcxError) as e:
        _run(rng.normal(size=(2, 40, 40)), rng.normal(size=(2, 40, 9)), 0.1)
    assert e.value.code == _capi.E_UNSUPPORTED and "48" in str(e.value)
    c = R.case("random_g1")
    R.check_family("random_g1", *_run(c["A"], c["B"], c["Ts"]), where=" (after the refused call)")


def _check_against_oracle(A, B, Ts, Ad, Bd, which):
    worst = 0.0
    for i in which:
        ra, rb = ref_c2d(A[i], B[i], Ts[i])
        worst = max(worst, R.worst_ratio(A[i:i + 1], B[i:i + 1], Ts[i:i + 1], ra[None], rb[None], Ad[i:i + 1], Bd[i:i + 1]))
    return worst


def test_grid_stride_and_lds_reuse():
    """4096 + 37 instances at (nx, nu) = (2, 1): instances 0..4095 are stiff (8 squarings and more), the tail needs none and runs in the blocks
    and the LDS that the stiff instances 0..36 have just left.  Every instance against the numpy oracle within the bound; the tail bit-equal
    to the same inputs at positions 5..41 of a small call"""
    rng = np.random.default_rng(4133)
    m, tail = 4096 + 37, 37
    A, B, Ts = R.grid_stride_inputs(rng, m, tail)
    s = R.squarings(A, B, Ts)
    assert s[:4096].min() >= 8 and s[4096:].max() == 0
    Ad, Bd = _run(A, B, Ts)
    w = _check_against_oracle(A, B, Ts, Ad, Bd, range(m))
    print("c2d grid-stride 4133: worst error / bound against the numpy oracle %.4f" % w)
    assert w <= 1.0
    sel = np.concatenate([np.arange(100, 105), np.arange(4096, m), np.arange(200, 208)])       # the tail at 5..41 of 50 instances
    sa, sb = _run(A[sel], B[sel], Ts[sel])
    assert np.array_equal(Ad[4096:], sa[5:42]) and np.array_equal(Bd[4096:], sb[5:42])
    assert np.array_equal(Ad[sel], sa) and np.array_equal(Bd[sel], sb)
    # one instance, and exactly as many as there are blocks
    one = _run(A[:1], B[:1], Ts[:1])
    assert np.array_equal(one[0], Ad[:1]) and np.array_equal(one[1], Bd[:1])
    full = _run(A[:4096], B[:4096], Ts[:4096])
    assert np.array_equal(full[0], Ad[:4096]) and np.array_equal(full[1], Bd[:4096])


def test_shared_and_per_instance_sampling_time():
    rng = np.random.default_rng(70)
    A = rng.normal(size=(70, 9, 9)) * rng.uniform(0.1, 30.0, size=(70, 1, 1)); B = rng.normal(size=(70, 9, 4))
    shared = _run(A, B, 0.07)
    per = _run(A, B, np.full(70, 0.07))
    assert _equal(shared, per)
    assert _equal(per, _run(A, B, np.full(70, 0.07))) and _equal(shared, _run(A, B, 0.07))        # bit-reproducible
    assert _check_against_oracle(A, B, np.full(70, 0.07), shared[0], shared[1], range(70)) <= 1.0


@pytest.mark.parametrize("m", [4100, 4104])
def test_a_poisoned_neighbour(m):
    """a NaN in instance 3 and +inf in instance 7 of A: those two come out non-finite, the call returns, and every other instance -- 4099 (and
    4103 where the batch has it), which run in the same blocks behind them, included -- has the bits of the clean run.  (The squaring count stays
    bounded: NaN fails `cs > 0.5`, the count that +inf gives is clamped to 60.)"""
    rng = np.random.default_rng(m)
    A = rng.normal(size=(m, 2, 2)) * rng.uniform(0.1, 30.0, size=(m, 1, 1)); B = rng.normal(size=(m, 2, 1))
    Ts = rng.uniform(0.005, 0.3, size=m)
    clean = _run(A, B, Ts)
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    Ap = A.copy(); Ap[3, 0, 0] = np.nan; Ap[7, 1, 0] = np.inf
    bad = _run(Ap, B, Ts)
    for i in (3, 7):
        assert not (np.isfinite(bad[0][i]).all() and np.isfinite(bad[1][i]).all()), i
    keep = np.ones(m, bool); keep[[3, 7]] = False
    assert np.array_equal(bad[0][keep], clean[0][keep]) and np.array_equal(bad[1][keep], clean[1][keep])


def test_c_abi_argument_checks():
    import torch
    from libmpc_amd import _capi
    lib = _capi.lib()
    dev = torch.device("cuda", 0)
    c = R.case("tiny_2_1")
    A = torch.from_numpy(np.swapaxes(c["A"], 1, 2).copy()).to(dev); B = torch.from_numpy(np.swapaxes(c["B"], 1, 2).copy()).to(dev)        # column-major
    Ts = torch.from_numpy(c["Ts"].copy()).to(dev)
    Ad = torch.full_like(A, -7.25); Bd = torch.full_like(B, -7.25)
    good = dict(device=0, nx=2, nu=1, batch=3, A=A.data_ptr(), B=B.data_ptr(), Ts=Ts.data_ptr(), per=1, Ad=Ad.data_ptr(), Bd=Bd.data_ptr(), stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mpcx_discretize_batch(*[a[k] for k in ("device", "nx", "nu", "batch", "A", "B", "Ts", "per", "Ad", "Bd", "stream")])
    for kw in (dict(nx=0), dict(nx=-1), dict(nu=-1), dict(batch=-1), dict(A=None), dict(Ts=None), dict(Ad=None), dict(B=None), dict(Bd=None)):
        assert call(**kw) == _capi.E_INVALID, kw
        assert lib.mpcx_last_error(), kw
    assert call(nx=40, nu=9) == _capi.E_UNSUPPORTED and b"48" in lib.mpcx_last_error()
    # an empty batch is fine and touches nothing -- not even null pointers
    assert call(batch=0) == _capi.OK and call(batch=0, A=None, B=None, Ts=None, Ad=None, Bd=None) == _capi.OK
    torch.cuda.synchronize()
    assert (Ad == -7.25).all() and (Bd == -7.25).all()
    # ... and the good call is good: the same bits as the front end's
    assert call() == _capi.OK
    torch.cuda.synchronize()
    want = _run(c["A"], c["B"], c["Ts"])
    assert np.array_equal(Ad.transpose(1, 2).cpu().numpy(), want[0]) and np.array_equal(Bd.transpose(1, 2).cpu().numpy(), want[1])


def test_python_front_end_forms_of_ts():
    import torch
    from libmpc_amd.utils import discretization
    c = R.case("random_g1")
    A, B, Ts = c["A"], c["B"], c["Ts"]
    m = A.shape[0]
    want = _run(A, B, Ts)

    def get(a, b, ts):
        o = discretization(a, b, ts)
        torch.cuda.synchronize()
        return o[0].cpu().numpy(), o[1].cpu().numpy()
    # per instance: a tensor (on the host, on the device), a numpy array, a list
    for ts in (torch.from_numpy(Ts.copy()), torch.from_numpy(Ts.copy()).cuda(), Ts.copy(), [float(t) for t in Ts]):
        assert _equal(get(A.copy(), B.copy(), ts), want), type(ts)
    # one value: a float, a numpy scalar, a 0-d and a 1-element tensor, a 1-element array and list
    t0 = float(Ts[1])
    shared = get(A.copy(), B.copy(), t0)
    assert _equal(shared, _run(A, B, np.full(m, t0)))
    for ts in (np.float64(t0), torch.tensor(t0, dtype=torch.float64), torch.tensor([t0], dtype=torch.float64), np.array([t0]), [t0]):
        assert _equal(get(A.copy(), B.copy(), ts), shared), type(ts)
    # a single model as 2-D matrices
    single = get(A[1].copy(), B[1].copy(), t0)
    assert single[0].shape == (1, 9, 9) and single[1].shape == (1, 9, 4)
    assert np.array_equal(single[0][0], shared[0][1]) and np.array_equal(single[1][0], shared[1][1])
    # no inputs at all
    c0 = R.case("nu0")
    o = get(c0["A"].copy(), np.zeros((4, 5, 0)), c0["Ts"].copy())
    assert o[1].shape == (4, 5, 0)
    R.check_family("nu0", o[0], o[1], " (front end)")
    # a sampling-time vector of any other length is refused before anything is launched
    for bad in (Ts[:m - 1].copy(), np.concatenate([Ts, Ts]), torch.from_numpy(Ts[:2].copy()), [0.1, 0.2], np.zeros(0)):
        with pytest.raises(ValueError):
            discretization(A.copy(), B.copy(), bad)
