"""-m gpu: the Riccati kernel (mpcx_dare_batch, kernel dare_sda of libmpc_amd/csrc/dare_kernels.hip, libmpc_amd.utils.dare / kalman_gains /
lqr_gains, LMPCHetero.kalman_gains) in both forms, at every shape and conditioning of tests/dare_ref.py, against the 60-digit truths of
tests/golden/dare_truth.npz (tests/golden/make_dare_golden.py) and within the bound derived there.  Beside it: the per-instance flags and the
NaN outputs of a failed instance, position independence (the grid-stride loop: more than 4096 instances), shared against per-instance Q and
R, the device gains of two banks against the host routine of each controller, and an observed bank loop fed with the device gains as they
come against the same numbers passed as numpy."""
import numpy as np
import pytest

import dare_ref as R

pytestmark = pytest.mark.gpu


def _run(form, A, M, Q, Rm, want_iterations=False):
    """numpy in, numpy out, through the Python front end"""
    import torch
    from libmpc_amd.utils import dare
    out = dare(A, M, Q, Rm, form, want_iterations=want_iterations)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


# (a) accuracy
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_family_against_the_truth(name, form):
    A, M, Q, Rm = R.inputs(name, form)
    shared = R.case(name)["shared"]
    G, X, flags, its = _run(form, A, M, Q[0] if shared else Q, Rm[0] if shared else Rm, True)
    assert (flags == 0).all() and (its >= 1).all() and (its <= R.MAX_DOUBLINGS).all(), (flags, its)
    R.check_family(name, form, X, G)


@pytest.mark.parametrize("form", R.FORMS)
def test_shared_and_per_instance_q_and_r(form):
    A, M, Q, Rm = R.inputs("rho_098", form)
    assert R.case("rho_098")["shared"]
    shared, per = _run(form, A, M, Q[0], Rm[0]), _run(form, A, M, Q, Rm)
    mixed = _run(form, A, M, Q, Rm[0])
    assert all(np.array_equal(a, b) for a, b in zip(shared, per)) and all(np.array_equal(a, b) for a, b in zip(shared, mixed))
    # the named front ends are the two forms
    from libmpc_amd.utils import kalman_gains, lqr_gains
    named = (lqr_gains if form == "control" else kalman_gains)(A, M, Q[0], Rm[0])
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(shared, named))
    one = _run(form, A[1], M[1], Q[0], Rm[0])              # 2-D: a batch of one
    assert one[0].shape == (1,) + shared[0].shape[1:] and np.array_equal(one[0][0], shared[0][1]) and np.array_equal(one[1][0], shared[1][1])


# (b) flags
def test_flags_and_nan_outputs():
    """R not positive definite -> 1.  An unstable mode that the output does not see (A = diag(1.5, 0.5), C = [0 1]) -> 3, not 2: a squares
    its entries every step, 1.5^(2^k) overflows at the eleventh doubling, long before the cap of 40, and the non-finite check ends the
    instance there.  A NaN in A -> 3.  The failing instances are NaN throughout; the good ones have the bits of a call of their own."""
    A, M, Q, Rm = (np.concatenate([np.array(a)] * 3, axis=0) for a in R.inputs("shape_2_1", "estimator"))      # 9 instances
    bad = [1, 4, 6]
    Rm[1] = -0.04
    A[4] = np.diag([1.5, 0.5]); M[4] = [[0.0, 1.0]]
    A[6, 1, 0] = np.nan
    G, X, flags, its = _run("estimator", A, M, Q, Rm, True)
    good = [i for i in range(9) if i not in bad]
    assert list(flags[bad]) == [1, 3, 3] and (flags[good] == 0).all(), flags
    assert its[1] == 0 and 5 <= its[4] <= 12, its
    assert np.isnan(X[bad]).all() and np.isnan(G[bad]).all()
    assert np.isfinite(X[good]).all() and np.isfinite(G[good]).all()
    alone = _run("estimator", A[good], M[good], Q[good], Rm[good], True)
    assert np.array_equal(G[good], alone[0]) and np.array_equal(X[good], alone[1]) and np.array_equal(its[good], alone[3])
    Xt, Gt = R.truth("shape_2_1", "estimator")
    # instances 0 and 2 against the truth (the failing instance 1 between them replaced by its truth)
    R.check_family("shape_2_1", "estimator", np.stack([X[0], Xt[1], X[2]]), np.stack([G[0], Gt[1], G[2]]), " (beside failing instances)")


# (c) position independence
def test_one_instance_at_four_positions_of_a_large_batch():
    """positions 0, 63, 64 and 4100 of 4101 instances (the last in block 4 behind instance 4: the grid-stride loop reuses its LDS): identical
    bits, and those of a call of its own"""
    rng = np.random.default_rng(4101)
    k, n, m = 4101, 5, 2
    A = rng.normal(size=(k, n, n)) * 0.4; C = rng.normal(size=(k, m, n))
    Q = 0.01 * np.eye(n); Rm = 0.04 * np.eye(m)
    c = R.case("shape_5_2")
    at = [0, 63, 64, 4100]
    A[at] = c["A"][0].T; C[at] = c["B"][0].T
    G, X, flags, its = _run("estimator", A, C, Q, Rm, True)
    assert (flags == 0).all()
    alone = _run("estimator", A[:1], C[:1], Q, Rm, True)
    for i in at:
        assert np.array_equal(X[i], alone[1][0]) and np.array_equal(G[i], alone[0][0]) and its[i] == alone[3][0], i
    # the others are solutions too: the residual of the equation, at the bound's scale (cond-free: relative to the terms of the equation)
    for i in range(1, k, 97):
        P, L = X[i], G[i]
        S = C[i] @ P @ C[i].T + Rm
        res = A[i] @ P @ A[i].T - L @ S @ L.T + Q - P
        assert np.abs(res).max() <= R.C_BOUND * n * R.U * max(np.abs(A[i] @ P @ A[i].T).max(), np.abs(P).max()), i


# (d) the device gains of a bank against the host routine of each controller
def _bank_controllers(name):
    from libmpc_amd import LMPC
    from libmpc_amd.workloads import quadrotor_variant
    from helpers import configure_random, random_lmpc_spec
    if name == "quadrotor8":
        return [quadrotor_variant(k, 10, device=-1) for k in range(8)]
    return [configure_random(LMPC(*sp["dims"], device=-1), sp) for sp in (random_lmpc_spec(100 + k) for k in range(7))]


@pytest.mark.parametrize("name", ["quadrotor8", "random7"])
def test_bank_gains_against_the_host_routine(name):
    import torch
    from libmpc_amd import LMPCHetero, MpcxError
    ctrls = _bank_controllers(name)
    het = LMPCHetero(ctrls, device=0)
    Qw, Rv = 0.01 * np.eye(het.nx), 0.04 * np.eye(het.ny)
    L = het.kalman_gains(Qw, Rv)
    assert isinstance(L, torch.Tensor) and L.is_cuda and tuple(L.shape) == (het.count, het.nx, het.ny)
    L = L.cpu().numpy()
    for k, c in enumerate(ctrls):
        want = c.kalman_gain(Qw, Rv)
        rel = np.abs(L[k] - want).max() / np.abs(want).max()
        print("dare %s controller %d: device gain against the host routine, relative %.3e" % (name, k, rel))
        assert rel <= 1e-10, (name, k, rel)
    # a covariance per controller; and a failing controller is named
    per = het.kalman_gains(np.stack([Qw] * het.count), np.stack([Rv] * het.count)).cpu().numpy()
    assert np.array_equal(per, L)
    Rbad = np.stack([Rv] * het.count); Rbad[2] = -Rv
    with pytest.raises(MpcxError) as e:
        het.kalman_gains(Qw, Rbad)
    assert "controller 2" in str(e.value)


# (e) end to end: the device gains as they come into an observed bank loop
@pytest.mark.parametrize("name", ["random7_mixed", "quadrotor8"])
def test_observed_bank_loop_takes_the_device_gains(name):
    import torch
    from test_lmpc_loop_fleet_gpu import _bank_case
    het, _, B, x0, u0, refs = _bank_case(name)
    ticks = 7
    gains = het.kalman_gains(0.01 * np.eye(het.nx), 0.04 * np.eye(het.ny))
    idx = torch.as_tensor(refs["model"] if "model" in refs else np.arange(B), device=gains.device)
    L = gains[idx]
    assert L.is_cuda and tuple(L.shape) == (B, het.nx, het.ny)
    r = np.random.default_rng(32)
    dx, v, w = 0.05 * r.normal(size=(B, het.nx)), 0.02 * r.normal(size=(ticks, B, het.ny)), 0.02 * r.normal(size=(ticks, B, het.nx))
    dev = het.simulate(x0, u0, ticks, observer=L, xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    host = het.simulate(x0, u0, ticks, observer=L.cpu().numpy(), xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    assert int((dev.status == 0).sum()) > 0
    for f in ("x", "u", "xhat", "y", "cost", "status", "solver_status", "iterations", "polish_rounds", "active_count"):
        a, b = getattr(dev, f), getattr(host, f)
        assert torch.equal(a, b), (name, f, int((a != b).sum()))
    loop = het.make_loop(x0, u0, ticks, observer=L, xhat0=x0 + dx, meas_noise=v, noise=w, **refs)
    try:
        again = het.run_loop(loop)
        torch.cuda.synchronize()
        assert torch.equal(again.xhat, dev.xhat) and torch.equal(again.u, dev.u)
        assert torch.equal(loop.gains, het.pack_gains(L))
    finally:
        het.destroy_loop(loop)


def test_c_abi_on_the_device():
    """the raw entry: null gain, flags and iterations are allowed; an empty batch touches nothing; the result is the front end's"""
    import torch
    from libmpc_amd import _capi
    lib = _capi.lib()
    A, M, Q, Rm = R.inputs("shape_3_2", "control")
    cm = lambda a: torch.from_numpy(np.swapaxes(a, -1, -2).copy()).cuda()
    Ad, Bd, Qd, Rd = cm(A), cm(M), cm(Q), cm(Rm)
    X = torch.full((3, 3, 3), -7.25, dtype=torch.float64, device="cuda")
    args = lambda batch, x: (0, _capi.DARE_CONTROL, 3, 2, batch, Ad.data_ptr(), Bd.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), 1, 1, x, None, None, None, None)
    assert lib.mpcx_dare_batch(*args(0, X.data_ptr())) == _capi.OK
    torch.cuda.synchronize()
    assert (X == -7.25).all()
    assert lib.mpcx_dare_batch(*args(3, X.data_ptr())) == _capi.OK
    torch.cuda.synchronize()
    want = _run("control", A, M, Q, Rm)
    assert np.array_equal(X.transpose(1, 2).cpu().numpy(), want[1])
