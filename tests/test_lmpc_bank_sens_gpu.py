"""Sensitivities of a solved batch of a bank on the GPU, through the C ABI and the Python front-end: the Jacobians of every
family against the KKT system of each instance's own reference QP (tests/bank_sens_ref.py) at bank_sens_ref.BANK_KERNEL_TOL, the bank's launch
against each member's own single-controller launch, vector-Jacobian products, flags, NULL outputs and guards, determinism, autograd, and the
affine law against the oracle's solve of a perturbed instance."""
import ctypes as C
import functools

import numpy as np
import pytest

import bank_sens_ref as BR
import linear_ref as LR
import sens_ref as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def bank(name):
    from libmpc_amd import LMPC, LMPCHetero
    ctl = [BR.configure(LMPC(*sp["dims"], device=-1), sp) for sp in BR.reference(name)["specs"]]
    return LMPCHetero(ctl, device=0)


@functools.lru_cache(maxsize=None)
def solved(name):
    """the family's bank on the device, its solve under the shuffled instance -> controller map and the Jacobians of its active sets"""
    import torch
    R = BR.reference(name)
    h = bank(name)
    model = torch.as_tensor(R["model"].astype(np.int32)).cuda()
    r = h.optimizeBatch(R["x0"], R["u0"], model=model, yref=R["yref"], want_active=True)
    s = h.sensitivityBatch(r.active_lower, r.active_upper, model=model, status=r.status)
    torch.cuda.synchronize()
    return h, model, r, s


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _same_sets(R, r, rows=None):
    """per instance: the device's active set equals the oracle's on the compared rows"""
    keep = LR.compared_rows(R["specs"][0])
    m = R["active_lower"].shape[1]
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    ol, ou = R["active_lower"] != 0, R["active_upper"] != 0
    if rows is not None:
        ol, ou = ol[rows], ou[rows]
    return (lo[:, keep] == ol[:, keep]).all(axis=1) & (up[:, keep] == ou[:, keep]).all(axis=1)


def _usable(name):
    """instances whose reference Jacobian exists, that the bank solved and whose active set on the device equals the oracle's"""
    R = BR.reference(name)
    h, model, r, s = solved(name)
    same = _same_sets(R, r)
    st = r.status.cpu().numpy()
    use = [b for b in range(len(st)) if R["jac"][b] is not None and same[b] and st[b] == 0]
    assert len(st) - len(use) <= BR.SKIP_CAP * len(st), (name, len(use), len(st))
    return use


def _jac(s):
    return np.concatenate([s.d_x0.cpu().numpy(), s.d_u0.cpu().numpy(), s.d_yref.cpu().numpy()], axis=-1)


@pytest.mark.parametrize("name", BR.FAMILIES)
def test_jacobians_match_the_kkt_system(name):
    import torch
    R = BR.reference(name)
    h, model, r, s = solved(name)
    use = _usable(name)
    J = _jac(s)
    flags = s.flags.cpu().numpy()
    assert (flags[use] == 0).all()
    worst = max(BR.error(J[b], R["jac"][b]["cmd"]) for b in use)
    print(f"{name}: worst error / bound {worst:.2e} / {BR.BANK_KERNEL_TOL:.2e}, {len(use)} of {len(flags)} instances")
    assert worst <= BR.BANK_KERNEL_TOL
    # every instance its own controller: no map, the batch is the bank
    pick = np.array([int(np.nonzero(R["model"] == k)[0][0]) for k in range(h.count)])
    r1 = h.optimizeBatch(R["x0"][pick], R["u0"][pick], yref=R["yref"][pick], want_active=True, sensitivities=True)
    torch.cuda.synchronize()
    same = _same_sets(R, r1, pick)
    st = r1.status.cpu().numpy()
    J1 = _jac(r1.sensitivities)
    use1 = [k for k, b in enumerate(pick) if R["jac"][b] is not None and same[k] and st[k] == 0]
    assert len(pick) - len(use1) <= BR.SKIP_CAP * len(pick)
    assert (r1.sensitivities.flags.cpu().numpy()[use1] == 0).all()
    worst1 = max(BR.error(J1[k], R["jac"][pick[k]]["cmd"]) for k in use1)
    print(f"{name}: without a map {worst1:.2e}")
    assert worst1 <= BR.BANK_KERNEL_TOL


@pytest.mark.parametrize("name", BR.FAMILIES)
def test_the_bank_gives_what_each_controller_gives(name):
    """for every controller a device LMPC of the same spec differentiates the same active sets: both lie within their tolerance of one truth"""
    import torch
    from libmpc_amd import LMPC
    R = BR.reference(name)
    h, model, r, s = solved(name)
    use = set(_usable(name))
    J = _jac(s)
    flags = s.flags.cpu().numpy()
    worst = 0.0
    for k, sp in enumerate(R["specs"]):
        idx = np.nonzero(R["model"] == k)[0]
        c = BR.configure(LMPC(*sp["dims"], device=0), sp)
        it = torch.as_tensor(idx).cuda()
        own = c.sensitivityBatch(r.active_lower[it].contiguous(), r.active_upper[it].contiguous(), status=r.status[it].contiguous())
        torch.cuda.synchronize()
        Jo = _jac(own)
        assert np.array_equal(own.flags.cpu().numpy(), flags[idx])
        for t, b in enumerate(idx):
            if b in use:
                worst = max(worst, np.abs(J[b] - Jo[t]).max() / max(1.0, np.abs(R["jac"][b]["cmd"]).max()))
    print(f"{name}: bank against its members {worst:.2e} / {BR.BANK_KERNEL_TOL + S.KERNEL_TOL:.2e}")
    assert worst <= BR.BANK_KERNEL_TOL + S.KERNEL_TOL


def test_vector_jacobian_products():
    R = BR.reference("full")
    h, model, r, s = solved("full")
    use = _usable("full")
    B, nu, ph = len(R["model"]), h.nu, h.ph
    rg = np.random.default_rng(23)
    sc, sq = rg.normal(size=(B, nu)), rg.normal(size=(B, ph + 1, nu))
    for kw in (dict(seed_cmd=sc), dict(seed_input=sq), dict(seed_cmd=sc, seed_input=sq)):
        v = h.sensitivityBatch(r.active_lower, r.active_upper, model=model, status=r.status, **kw)
        g = _jac(v)
        assert g.shape == (B, h.nx + nu + h.ny) and np.array_equal(v.flags.cpu().numpy(), s.flags.cpu().numpy())
        for b in use:
            ref, mass = 0.0, 0.0
            if "seed_cmd" in kw:
                ref = ref + np.einsum("r,rc->c", sc[b], R["jac"][b]["cmd"]); mass += np.abs(sc[b]).sum()
            if "seed_input" in kw:
                ref = ref + np.einsum("ir,irc->c", sq[b], R["jac"][b]["input"]); mass += np.abs(sq[b]).sum()
            bound = BR.BANK_KERNEL_TOL * max(1.0, np.abs(R["jac"][b]["input"]).max()) * mass
            assert np.abs(g[b] - ref).max() <= bound, (sorted(kw), b)


def test_flags_nan_and_untouched_neighbours():
    """a status that is not SUCCESS: flag 1; the box row and the step-0 rate row of one input, which are parallel: flag 2; both NaN, and the
    other instances keep their bits"""
    import torch
    R = BR.reference("full")
    h, model, r, s = solved("full")
    words = h.info()["active_words"]
    status = r.status.clone(); status[5] = 2
    d = R["pbs"][0].d
    lo = np.zeros((1, 32 * words), bool); up = np.zeros((1, 32 * words), bool)
    lo[0, d.neq + d.na + h.nx] = True; up[0, d.neq + d.off_du] = True
    al = r.active_lower.clone(); au = r.active_upper.clone()
    al[7] = torch.as_tensor(S.pack_bits(lo, words)).cuda()[0]; au[7] = torch.as_tensor(S.pack_bits(up, words)).cuda()[0]
    out = h.sensitivityBatch(al, au, model=model, status=status)
    torch.cuda.synchronize()
    flags, clean = out.flags.cpu().numpy(), s.flags.cpu().numpy()
    assert flags[5] == 1 and flags[7] == 2
    others = [b for b in range(len(flags)) if b not in (5, 7)]
    assert np.array_equal(flags[others], clean[others])
    for n in ("d_x0", "d_u0", "d_yref"):
        a, a0 = getattr(out, n).cpu().numpy(), getattr(s, n).cpu().numpy()
        assert np.isnan(a[5]).all() and np.isnan(a[7]).all()
        assert a[others].tobytes() == a0[others].tobytes(), n


def test_null_outputs_guards_and_a_batch_that_ends_inside_a_workgroup():
    """every output is optional; nothing is written outside the arrays (a guard of 64 elements behind each) or in place of an output that was
    not asked for; 19 instances leave the last workgroup of four wavefronts with one idle"""
    import torch
    from libmpc_amd import _capi
    h, model, r, s = solved("full")
    B, nx, nu, ny = 19, h.nx, h.nu, h.ny
    sizes = {"d_x0": B * nu * nx, "d_u0": B * nu * nu, "d_yref": B * nu * ny}
    full = {n: getattr(s, n).cpu().numpy()[:B].reshape(-1) for n in sizes}
    for present in (("d_x0",), ("d_u0", "d_yref"), (), ("d_x0", "d_u0", "d_yref")):
        bufs = {n: torch.full((sizes[n] + 64,), 777.0, dtype=torch.float64, device="cuda") for n in sizes}
        flags = torch.full((B + 64,), 777, dtype=torch.int32, device="cuda")
        d = _capi.Sens()
        d.batch = B
        d.active_lower, d.active_upper, d.status = r.active_lower.data_ptr(), r.active_upper.data_ptr(), r.status.data_ptr()
        d.mode = _capi.SENS_JACOBIAN
        for n in present:
            setattr(d, n, bufs[n].data_ptr())
        d.flags = flags.data_ptr() if present else None
        _capi.check(_capi.lib().mpcx_lmpc_hetero_sensitivity_batch(h._h, C.byref(d), C.c_void_p(model.data_ptr()),
                                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for n in sizes:
            got = bufs[n].cpu().numpy()
            if n in present:
                assert (got[sizes[n]:] == 777.0).all(), n
                assert got[:sizes[n]].tobytes() == full[n].tobytes(), n
            else:
                assert (got == 777.0).all(), n
        f = flags.cpu().numpy()
        assert (f[B:] == 777).all()
        assert (f[:B] == (s.flags.cpu().numpy()[:B] if present else 777)).all()


def test_argument_errors():
    import torch
    from libmpc_amd import _capi
    h, model, r, s = solved("full")
    lib = _capi.lib()

    def call(mi=model, **kw):
        d = _capi.Sens()
        d.batch = 32
        d.active_lower, d.active_upper = r.active_lower.data_ptr(), r.active_upper.data_ptr()
        d.mode = _capi.SENS_JACOBIAN
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.mpcx_lmpc_hetero_sensitivity_batch(h._h, C.byref(d), None if mi is None else C.c_void_p(mi.data_ptr()), None)
    assert lib.mpcx_lmpc_hetero_sensitivity_batch(h._h, None, None, None) == _capi.E_INVALID
    assert call(mode=7) == _capi.E_INVALID and call(batch=0) == _capi.E_INVALID and call(active_upper=None) == _capi.E_INVALID
    assert call(mode=_capi.SENS_VJP) == _capi.E_INVALID and call(mi=None) == _capi.E_INVALID
    with pytest.raises(ValueError):
        h.sensitivityBatch(r.active_lower, r.active_upper, model=torch.full((32,), h.count, dtype=torch.int32))
    with pytest.raises(ValueError):
        h.sensitivityBatch(r.active_lower, r.active_upper, model=model[:5])
    with pytest.raises(ValueError):
        h.sensitivityBatch(r.active_lower, r.active_upper)                  # no map, and the batch is not the bank


@pytest.mark.parametrize("name", ["full", "soft", "nz17"])
def test_two_launches_give_the_same_bits(name):
    h, model, r, s = solved(name)
    again = h.sensitivityBatch(r.active_lower, r.active_upper, model=model, status=r.status)
    for n in ("d_x0", "d_u0", "d_yref", "flags"):
        a, b = getattr(s, n).cpu().numpy(), getattr(again, n).cpu().numpy()
        assert a.tobytes() == b.tobytes(), n


def test_autograd_gives_the_vjp():
    import torch
    from libmpc_amd import lmpc_cmd
    R = BR.reference("full")
    h, model, r, s = solved("full")
    use = _usable("full")
    rg = np.random.default_rng(29)
    seed = rg.normal(size=(len(R["model"]), h.nu))
    x0 = torch.tensor(R["x0"], device="cuda", requires_grad=True); u0 = torch.tensor(R["u0"], device="cuda", requires_grad=True)
    yref = torch.tensor(R["yref"], device="cuda", requires_grad=True)
    cmd = lmpc_cmd(h, x0, u0, yref, model=model)
    assert torch.equal(cmd, r.cmd)
    (cmd * torch.as_tensor(seed).cuda()).sum().backward()
    v = h.sensitivityBatch(r.active_lower, r.active_upper, model=model, status=r.status, seed_cmd=seed)
    for a, n in zip((x0.grad, u0.grad, yref.grad), ("d_x0", "d_u0", "d_yref")):
        assert torch.equal(a, getattr(v, n)), n
    got = np.concatenate([a.cpu().numpy() for a in (x0.grad, u0.grad, yref.grad)], axis=1)
    for b in use:
        ref = np.einsum("r,rc->c", seed[b], R["jac"][b]["cmd"])
        assert np.abs(got[b] - ref).max() <= BR.BANK_KERNEL_TOL * max(1.0, np.abs(R["jac"][b]["input"]).max()) * np.abs(seed[b]).sum(), b


@pytest.mark.parametrize("name", ["full", "terminal"])
def test_affine_law_predicts_the_oracle_at_a_perturbed_point(name):
    """cmd + J delta against the oracle's cmd at (x0, lastU, yref) + delta on the instance's own controller, for a delta that keeps the oracle's
    active set: 1e-5 relative, 4.8's figure for the same check"""
    R = BR.reference(name)
    h, model, r, s = solved(name)
    nx, nu = h.nx, h.nu
    J = _jac(s)
    cmd = r.cmd.cpu().numpy()
    rg = np.random.default_rng(17)
    use = _usable(name)[:16]
    done = 0
    for b in use:
        k = R["model"][b]
        sp, pb = R["specs"][k], R["pbs"][k]
        d = 1e-3 * rg.normal(size=J.shape[-1])       # (keeps the oracle's set on all sixteen: checked on the CPU)
        o = S.solve_one(pb, sp, R["x0"][b] + d[:nx], R["u0"][b] + d[nx:nx + nu], R["yref"][b] + d[nx + nu:])
        if not (o["polished"] == 1 and np.array_equal(o["active_lower"] != 0, R["active_lower"][b] != 0)
                and np.array_equal(o["active_upper"] != 0, R["active_upper"][b] != 0)):
            continue
        pred = cmd[b] + J[b] @ d
        assert np.abs(pred - o["cmd"]).max() <= 1e-5 * max(np.abs(o["cmd"]).max(), 1e-12), (name, b)
        done += 1
    assert len(use) - done <= BR.SKIP_CAP * len(use), (name, done, len(use))
