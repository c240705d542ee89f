"""The bank's condensing kernel (libmpc_amd/csrc/lmpc_hetero.hip, lmpc_condense_models) against the 60-digit truths of
tests/golden/condense_truth_*.npz within the bound of tests/condense_ref.py: every family -- shapes on either side of the MFMA tiles and
k-steps, row counts from none to more row tiles than column tiles, all features at once, the last LDS shape, the first scratch shape, the
scratch form by bytes, a Hessian of condition 1e6 and a regularised one -- with the padding of every array, cost_direct and one solve held to
the bank that condensed on the host.  Then the grid-stride loop of both forms: a workgroup that condenses a second controller behind a
different one gives that controller the bits of its twin on a first trip.  And a bank beyond the kernel's LDS plan condenses on the host."""
import numpy as np
import pytest

import condense_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_family_against_the_truth(name):
    import torch
    from libmpc_amd import LMPCHetero
    fam = R.family(name)
    ctrls = R.host_controllers(name)
    host = LMPCHetero(ctrls, device=0, condense_on_host=True)
    dev = LMPCHetero(ctrls, device=0)
    assert host.debug_get(0, "flags")[1] == 0.0 and dev.debug_get(0, "flags")[1] == 1.0
    gots = [R.arrays_of(lambda n, k=k: dev.debug_get(k, n)) for k in range(len(fam))]
    R.check_family(name, gots, " (device)")
    for k, (ctl, lay, tr) in enumerate(fam):
        for n, mask in R.written(lay).items():
            a, b = gots[k][n], host.debug_get(k, n)
            assert a.size == b.size == mask.size and np.array_equal(_bits(a[~mask]), _bits(b[~mask])), (k, n)
        assert dev.debug_get(k, "flags")[0] == host.debug_get(k, "flags")[0] == ctrls[k].debug_get("flags")[0]
        assert not tr["reg"] or dev.debug_get(k, "flags")[0] == 1.0
    nx, nu = fam[0][0]["dims"][:2]
    r = np.random.default_rng(17)
    x0 = 0.3 * r.normal(size=(len(fam), nx)); u0 = r.uniform(-0.2, 0.2, size=(len(fam), nu))
    ra = host.optimizeBatch(x0, u0, want_active=True); rb = dev.optimizeBatch(x0, u0, want_active=True)
    torch.cuda.synchronize()
    assert torch.equal(ra.status, rb.status) and torch.equal(ra.active_lower, rb.active_lower) and torch.equal(ra.active_upper, rb.active_upper)
    np.testing.assert_allclose(rb.cmd.cpu().numpy(), ra.cmd.cpu().numpy(), rtol=1e-8, atol=1e-10)


def _tiny(seed):
    """nx = 2, nu = 1, ph = 3 with an input box and a bound on the first state"""
    r = np.random.default_rng(seed)
    A = r.normal(size=(2, 2)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
    return dict(dims=(2, 1, 1, 3, 3), A=A, B=r.normal(size=(2, 1)), C=r.normal(size=(1, 2)), OW=r.uniform(0.5, 2.0, size=(1, 3)),
                UW=r.uniform(0.05, 0.2, size=(1, 3)), DUW=r.uniform(0.01, 0.1, size=(1, 3)), umin=np.array([-0.6]), umax=np.array([0.6]),
                xmin=np.array([-2.0, -R.INF]), xmax=np.array([2.0, R.INF]))


def _second_trip_equals_its_twin(ctrls, grid, tail):
    """a bank of grid + tail controllers, controller i with spec i mod len(ctrls) and the tail shifted by one: workgroup j condenses controller j
    (spec j) and then controller grid + j (spec j + 1), whose arrays must be those of controller j + 1, bit for bit"""
    from libmpc_amd import LMPCHetero
    S = len(ctrls)
    assert grid % S == 0 and tail <= S
    spec = [i % S for i in range(grid)] + [(j + 1) % S for j in range(tail)]
    dev = LMPCHetero([ctrls[s] for s in spec], device=0)
    assert dev.debug_get(0, "flags")[1] == 1.0 and dev.count == grid + tail
    for j in range(tail):
        second, twin, before = grid + j, j + 1, j
        assert spec[second] == spec[twin] != spec[before]
        for n in R.ARRAYS:
            a = dev.debug_get(second, n)
            assert np.array_equal(_bits(a), _bits(dev.debug_get(twin, n))), (j, n)
            assert not np.array_equal(a, dev.debug_get(before, n)) or n in ("Gc", "Gr") and not a.any(), (j, n)      # (another controller's arrays are other numbers)
        assert dev.debug_get(second, "flags")[0] == dev.debug_get(twin, "flags")[0]
    return dev


def test_grid_stride_in_the_lds_form():
    """1024 + 8 controllers of 8 specs at nz = 3: the launch has 1024 workgroups, the last 8 controllers are second trips"""
    from libmpc_amd import LMPC
    ctrls = [R.configure(LMPC(2, 1, 0, 1, 3, 3, device=-1), _tiny(40 + s), seed=s) for s in range(8)]
    assert not R.condense_lds(2, 1, 3, int(ctrls[0].debug_get("dims")[1]))[1]
    dev = _second_trip_equals_its_twin(ctrls, 1024, 8)
    # ... and what a twin holds is the host's set-up of that controller
    for s in range(8):
        for n, tol in (("H", 1e-14), ("Gr", 1e-14), ("Y", 1e-12), ("rho_b", 1e-12), ("rho_g", 1e-12), ("Kinv", 1e-12)):
            a, b = ctrls[s].debug_get(n), dev.debug_get(s, n)
            assert np.abs(a - b).max() <= tol * np.abs(a).max(), (s, n)


def test_grid_stride_in_the_scratch_form():
    """512 + 4 controllers at nz = 98, the four of the family edge_big98 cycled: 512 workgroups, each with its scratch block, the last 4
    controllers are second trips in a block another controller has used"""
    ctrls = R.host_controllers("edge_big98")
    ctl, lay, _ = R.family("edge_big98")[0]
    assert R.condense_lds(ctl["dims"][0], ctl["dims"][2], lay["nz"], len(lay["kind"]))[1]
    dev = _second_trip_equals_its_twin(ctrls, 512, 4)
    R.check_family("edge_big98", [R.arrays_of(lambda n, k=k: dev.debug_get(512 + (k - 1) % 4, n)) for k in range(4)], " (device, second trips)")


def test_a_bank_beyond_the_lds_plan_condenses_on_the_host_and_solves():
    """nx = 32 with 336 variables: the roll-out's two S blocks, 2 x 32 x 337 doubles, alone exceed the LDS, in the scratch form too (the solve
    kernels' own plan, which grows with nx^2 and not with nx nz, has room)"""
    import torch
    from libmpc_amd import LMPC, LMPCHetero
    nx, nu, ny, ph = 32, 8, 2, 42
    assert R.condense_lds(nx, ny, nu * ph, 0)[0] > R.LDS_LIMIT - 64

    def spec(seed):
        r = np.random.default_rng(seed)
        A = r.normal(size=(nx, nx)); A *= 0.8 / max(abs(np.linalg.eigvals(A)))
        return dict(dims=(nx, nu, ny, ph, ph), A=A, B=r.normal(size=(nx, nu)), C=r.normal(size=(ny, nx)) / np.sqrt(nx), OW=r.uniform(0.5, 2.0, size=(ny, ph)),
                    UW=r.uniform(0.05, 0.2, size=(nu, ph)), DUW=r.uniform(0.01, 0.1, size=(nu, ph)), umin=np.full(nu, -0.5), umax=np.full(nu, 0.5))
    specs = [spec(70), spec(71)]
    bank = LMPCHetero([R.configure(LMPC(nx, nu, 0, ny, ph, ph, device=-1), sp, seed=k) for k, sp in enumerate(specs)], device=0)
    assert bank.debug_get(0, "flags")[1] == 0.0
    r = np.random.default_rng(3)
    x0 = 0.3 * r.normal(size=(2, nx)); u0 = r.uniform(-0.2, 0.2, size=(2, nu))
    rb = bank.optimizeBatch(x0, u0); torch.cuda.synchronize()
    assert (rb.status.cpu().numpy() == 0).all()
    for k, sp in enumerate(specs):
        one = R.configure(LMPC(nx, nu, 0, ny, ph, ph, device=0), sp, seed=k).optimizeBatch(x0[k:k + 1], u0[k:k + 1]); torch.cuda.synchronize()
        assert int(one.status[0]) == 0
        np.testing.assert_allclose(rb.cmd.cpu().numpy()[k], one.cmd.cpu().numpy()[0], rtol=1e-8, atol=1e-10)
