"""Sensitivities of a solved batch on the GPU, through the C ABI and the Python front-end: the Jacobians of every family against
the KKT system of the reference QP (tests/sens_ref.py) at sens_ref.KERNEL_TOL, the affine law against the oracle's solve of a perturbed
instance, vector-Jacobian products, flags, NULL outputs and guards, autograd, determinism."""
import ctypes as C
import functools

import numpy as np
import pytest

import linear_ref as LR
import rate_ref as RR
import sens_ref as S
import terminal_ref as TR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name):
    return S.reference(name)


@functools.lru_cache(maxsize=None)
def solved(name):
    """the family's controller on the device, its solve and the Jacobians of its active sets"""
    import torch
    from libmpc_amd import LMPC
    R = reference(name)
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    s = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status)
    torch.cuda.synchronize()
    return c, r, s


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _usable(name):
    """instances whose reference Jacobian exists and whose active set on the device equals the oracle's on the compared rows"""
    R = reference(name)
    c, r, s = solved(name)
    res, sp = R["res"], R["sp"]
    keep = LR.compared_rows(sp)
    m = int(res["ncon"])
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == (res["active_lower"][:, keep] != 0)).all(axis=1) & (up[:, keep] == (res["active_upper"][:, keep] != 0)).all(axis=1)
    st = r.status.cpu().numpy()
    use = [b for b in range(len(st)) if R["jac"][b] is not None and same[b] and st[b] == 0]
    assert len(st) - len(use) <= S.SKIP_CAP * len(st), (name, len(use), len(st))
    return use


def _jac(s):
    return np.concatenate([s.d_x0.cpu().numpy(), s.d_u0.cpu().numpy(), s.d_yref.cpu().numpy()], axis=-1)


@pytest.mark.parametrize("name", S.FAMILIES)
def test_jacobians_match_the_kkt_system(name):
    R = reference(name)
    c, r, s = solved(name)
    use = _usable(name)
    J = _jac(s)
    flags = s.flags.cpu().numpy()
    assert (flags[use] == 0).all()
    worst = max(np.abs(J[b] - R["jac"][b]["cmd"]).max() / max(1.0, np.abs(R["jac"][b]["cmd"]).max()) for b in use)
    count = r.active_count.cpu().numpy()
    print(f"{name}: worst error / bound {worst:.2e} / {S.KERNEL_TOL:.2e}, {len(use)} of {len(flags)} instances, active rows {count[use].min()} .. {count[use].max()}")
    assert worst <= S.KERNEL_TOL
    nx, nu = c.nx, c.nu
    if name == "smallest":
        assert (count == 0).all() and c.info()["nz"] == 1
    if name == "full":
        # instances the fallback solved are among them (the lean kernels hold sixteen rows), and sets on both sides of that limit
        assert (count[use] > 16).any() and (count[use] <= 16).any()
        rate0 = boxed = 0
        for b in use:
            Kx, Ku, Ky = S.split(J[b], nx, nu)
            for row in range(nu):
                e = np.zeros(nu); e[row] = 1.0
                if np.abs(Kx[row]).max() <= S.KERNEL_TOL and np.abs(Ky[row]).max() <= S.KERNEL_TOL:
                    rate0 += np.abs(Ku[row] - e).max() <= S.KERNEL_TOL
                    boxed += np.abs(Ku[row]).max() <= S.KERNEL_TOL
        assert rate0 >= 1 and boxed >= 1
    if name == "soft":
        assert (count[use] > c.info()["nz"]).any()


@pytest.mark.parametrize("name", S.FAMILIES)
def test_affine_law_predicts_the_oracle_at_a_perturbed_point(name):
    """cmd + J delta against the oracle's cmd at (x0, lastU, yref) + delta, for a delta that keeps the oracle's active set: 1e-5 relative, the
    suite's tolerance on cmd"""
    R = reference(name)
    c, r, s = solved(name)
    sp, pb, res = R["sp"], R["pb"], R["res"]
    nx, nu = c.nx, c.nu
    J = _jac(s)
    cmd = r.cmd.cpu().numpy()
    rg = np.random.default_rng(17)
    done = 0
    for b in _usable(name)[:8]:
        d = 1e-3 * rg.normal(size=J.shape[-1])
        o = S.solve_one(pb, sp, R["x0"][b] + d[:nx], R["u0"][b] + d[nx:nx + nu], R["yref"][b] + d[nx + nu:])
        if not (o["polished"] == 1 and np.array_equal(o["active_lower"] != 0, res["active_lower"][b] != 0)
                and np.array_equal(o["active_upper"] != 0, res["active_upper"][b] != 0)):
            continue
        pred = cmd[b] + J[b] @ d
        assert np.abs(pred - o["cmd"]).max() <= 1e-5 * max(np.abs(o["cmd"]).max(), 1e-12), (name, b)
        done += 1
    assert done >= 4, (name, done)


def test_lqr_gain_on_the_device():
    import torch
    from libmpc_amd import LMPC
    sp, Q, Rm = TR.lqr_spec("stable", 3)
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    x0, u0, _ = RR.random_batch(sp, 16, 3)
    r = c.optimizeBatch(x0, u0, want_active=True, sensitivities=True)
    torch.cuda.synchronize()
    s = r.sensitivities
    assert (s.flags.cpu().numpy() == 0).all() and (r.active_count.cpu().numpy() == 0).all()
    Kx = s.d_x0.cpu().numpy()
    assert np.abs(Kx + sp["K"][None]).max() <= 1e-9 * np.abs(sp["K"]).max()
    # ... and what optimizeBatch attaches is what the call on its active sets returns
    again = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status)
    for n in ("d_x0", "d_u0", "d_yref", "flags"):
        assert torch.equal(getattr(s, n), getattr(again, n))


def test_vector_jacobian_products():
    import torch
    R = reference("full")
    c, r, s = solved("full")
    use = _usable("full")
    J = _jac(s)
    B, nu, ph = J.shape[0], c.nu, c.ph
    rg = np.random.default_rng(23)
    seed = rg.normal(size=(B, nu))
    v = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_cmd=seed)
    g = _jac(v)
    assert g.shape == (B, J.shape[-1])
    want = np.einsum("br,brc->bc", seed, J)
    scale = np.maximum(1.0, np.abs(J).max(axis=(1, 2))) * np.abs(seed).sum(axis=1)
    assert (np.abs(g - want).max(axis=1)[use] <= S.KERNEL_TOL * scale[use]).all()
    # a cotangent on the whole input sequence, against the reference's sequence Jacobian from the same dz
    sq = rg.normal(size=(B, ph + 1, nu))
    vi = _jac(c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_input=sq))
    for b in use:
        ref = np.einsum("ir,irc->c", sq[b], R["jac"][b]["input"])
        bound = S.KERNEL_TOL * max(1.0, np.abs(R["jac"][b]["input"]).max()) * np.abs(sq[b]).sum()
        assert np.abs(vi[b] - ref).max() <= bound, b
    # row 0 of the sequence is the first move: a seed there alone is a seed on cmd
    only0 = np.zeros((B, ph + 1, nu)); only0[:, 0] = seed
    v0 = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_input=only0)
    for n in ("d_x0", "d_u0", "d_yref"):
        assert torch.equal(getattr(v0, n), getattr(v, n)), n
    # both seeds at once add up
    both = _jac(c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_cmd=seed, seed_input=sq))
    assert (np.abs(both - (g + vi)).max(axis=1)[use] <= S.KERNEL_TOL * (scale[use] + np.abs(sq).sum(axis=(1, 2))[use] * np.maximum(1.0, np.abs(J).max(axis=(1, 2)))[use])).all()


def test_unsolved_instance_gets_flag_1_and_leaves_its_neighbours_alone():
    """an instance infeasible by its data (lastU outside the input box) inside a batch of 37"""
    import torch
    R = reference("full")
    c, r, s = solved("full")
    B = len(R["x0"])
    assert B == 36
    at = 20
    x0 = np.insert(R["x0"], at, R["x0"][0], axis=0); u0 = np.insert(R["u0"], at, [0.9, 0.0], axis=0); yref = np.insert(R["yref"], at, R["yref"][0], axis=0)
    r2 = c.optimizeBatch(x0, u0, yref=yref, want_active=True)
    s2 = c.sensitivityBatch(r2.active_lower, r2.active_upper, status=r2.status)
    torch.cuda.synchronize()
    st = r2.status.cpu().numpy()
    assert st[at] != 0 and (np.delete(st, at) == 0).all()
    flags = s2.flags.cpu().numpy()
    assert flags[at] == 1 and (np.delete(flags, at) == s.flags.cpu().numpy()).all()
    others = [b for b in range(B + 1) if b != at]
    for n in ("d_x0", "d_u0", "d_yref"):
        a2 = getattr(s2, n).cpu().numpy()
        assert np.isnan(a2[at]).all()
        assert a2[others].tobytes() == getattr(s, n).cpu().numpy().tobytes(), n
    # without the status array the kernel cannot know: the flag is then whatever the active words say
    s3 = c.sensitivityBatch(r2.active_lower, r2.active_upper)
    assert s3.flags.cpu().numpy()[at] != 1


def test_dependent_working_set_gets_flag_2():
    """hand-made active words: the box row of the first move's input 0 and the step-0 rate row of the same input are parallel (both are e_0'
    on the decision vector); the same row named on both sides is one row and fine; no row at all is the unconstrained gain"""
    import torch
    R = reference("full")
    c, r, s = solved("full")
    sp = R["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    d = R["pb"].d
    words = c.info()["active_words"]
    box = d.neq + 1 * d.na + nx
    rate = d.neq + d.off_du
    lo = np.zeros((4, 32 * words), bool); up = np.zeros((4, 32 * words), bool)
    lo[0, box] = True; up[0, rate] = True                      # parallel rows
    lo[1, box] = True; up[1, box] = True                        # one row, both sides
    up[3, box] = True; up[3, rate] = True; lo[3, rate] = True   # parallel rows and a duplicate
    al = torch.as_tensor(S.pack_bits(lo, words)).cuda(); au = torch.as_tensor(S.pack_bits(up, words)).cuda()
    out = c.sensitivityBatch(al, au)
    torch.cuda.synchronize()
    flags = out.flags.cpu().numpy()
    assert flags.tolist() == [2, 0, 0, 2]
    J = _jac(out)
    assert np.isnan(J[0]).all() and np.isnan(J[3]).all() and np.isfinite(J[1]).all() and np.isfinite(J[2]).all()
    a = S.arrays(c)
    for b in (1, 2):
        ref = S.condensed_jacobian(a, lo[b], up[b])["cmd"]
        assert np.abs(J[b] - ref).max() <= S.KERNEL_TOL * max(1.0, np.abs(ref).max())
    assert np.abs(J[1][0]).max() <= S.KERNEL_TOL                        # the pinned input does not move


def test_null_outputs_and_guards():
    """every output is optional; nothing is written outside the arrays (a guard of 64 elements behind each)"""
    import torch
    from libmpc_amd import _capi
    c, r, s = solved("full")
    B, nx, nu, ny = r.cmd.shape[0], c.nx, c.nu, c.ny
    sizes = {"d_x0": B * nu * nx, "d_u0": B * nu * nu, "d_yref": B * nu * ny}
    full = {n: getattr(s, n).cpu().numpy().reshape(-1) for n in sizes}
    for present in (("d_x0",), ("d_u0", "d_yref"), (), ("d_x0", "d_u0", "d_yref")):
        bufs = {n: torch.full((sizes[n] + 64,), 777.0, dtype=torch.float64, device="cuda") for n in present}
        flags = torch.full((B + 64,), 777, dtype=torch.int32, device="cuda")
        d = _capi.Sens()
        d.batch = B
        d.active_lower, d.active_upper, d.status = r.active_lower.data_ptr(), r.active_upper.data_ptr(), r.status.data_ptr()
        d.mode = _capi.SENS_JACOBIAN
        for n in present:
            setattr(d, n, bufs[n].data_ptr())
        d.flags = flags.data_ptr() if present else None
        _capi.check(_capi.lib().mpcx_lmpc_sensitivity_batch(c._h, C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for n in present:
            got = bufs[n].cpu().numpy()
            assert (got[sizes[n]:] == 777.0).all(), n
            assert got[:sizes[n]].tobytes() == full[n].tobytes(), n
        f = flags.cpu().numpy()
        assert (f[B:] == 777).all()
        assert (f[:B] == (s.flags.cpu().numpy() if present else 777)).all()


def test_autograd_gives_the_vjp():
    import torch
    from libmpc_amd import lmpc_cmd
    R = reference("full")
    c, r, s = solved("full")
    use = _usable("full")

    def grads():
        x0 = torch.tensor(R["x0"], device="cuda", requires_grad=True); u0 = torch.tensor(R["u0"], device="cuda", requires_grad=True)
        yref = torch.tensor(R["yref"], device="cuda", requires_grad=True)
        cmd = lmpc_cmd(c, x0, u0, yref)
        assert torch.equal(cmd, r.cmd)
        cmd.sum().backward()
        return x0.grad, u0.grad, yref.grad
    g1 = grads()
    ones = torch.ones_like(r.cmd)
    v = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_cmd=ones)
    for a, n in zip(g1, ("d_x0", "d_u0", "d_yref")):
        assert torch.equal(a, getattr(v, n)), n
    J = _jac(s)
    want = J.sum(axis=1)
    got = np.concatenate([a.cpu().numpy() for a in g1], axis=1)
    scale = np.maximum(1.0, np.abs(J).max(axis=(1, 2))) * c.nu
    assert (np.abs(got - want).max(axis=1)[use] <= S.KERNEL_TOL * scale[use]).all()
    for b in use:
        ref = R["jac"][b]["cmd"].sum(axis=0)
        assert np.abs(got[b] - ref).max() <= S.KERNEL_TOL * c.nu * max(1.0, np.abs(R["jac"][b]["cmd"]).max())
    # a second backward pass on a fresh graph: the same bits
    g2 = grads()
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    # no gradient asked for the reference: none computed
    x0 = torch.tensor(R["x0"], device="cuda", requires_grad=True)
    lmpc_cmd(c, x0, R["u0"], R["yref"]).sum().backward()
    assert torch.equal(x0.grad, g1[0])


@pytest.mark.parametrize("name", ["full", "soft", "nz17"])
def test_two_launches_give_the_same_bits(name):
    import torch
    c, r, s = solved(name)
    again = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status)
    for n in ("d_x0", "d_u0", "d_yref", "flags"):
        a, b = getattr(s, n).cpu().numpy(), getattr(again, n).cpu().numpy()
        assert a.tobytes() == b.tobytes(), n


def test_host_array_form_gives_the_device_form():
    """mpcx_lmpc_sensitivity_host after mpcx_lmpc_solve_host: the Jacobians of that batch, refused without such a solve"""
    from libmpc_amd import LMPC, _capi
    R = reference("nz15")
    sp = R["sp"]
    c, r, s = solved("nz15")
    lib = _capi.lib()
    fresh = S.configure(LMPC(*sp["dims"], device=0), sp)
    B, nx, nu, ny = len(R["x0"]), fresh.nx, fresh.nu, fresh.ny
    kx = np.zeros((B, nu, nx)); ku = np.zeros((B, nu, nu)); ky = np.zeros((B, nu, ny)); fl = np.full(B, -1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mpcx_lmpc_sensitivity_host(fresh._h, p(kx), p(ku), p(ky), p(fl)) == _capi.E_STATE
    # (the host call solves with the controller's own reference; the device form below does the same)
    x0 = np.ascontiguousarray(R["x0"]); u0 = np.ascontiguousarray(R["u0"])
    cmd = np.zeros((B, nu)); cost = np.zeros(B); st = np.zeros(B, np.int32); sst = np.zeros(B, np.int32); fe = np.zeros(B, np.int32)
    lib.mpcx_lmpc_solve_host.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
    _capi.check(lib.mpcx_lmpc_solve_host(fresh._h, B, p(x0), p(u0), p(cmd), p(cost), p(st), p(sst), p(fe), None, None, None))
    _capi.check(lib.mpcx_lmpc_sensitivity_host(fresh._h, p(kx), p(ku), p(ky), p(fl)))
    r2 = fresh.optimizeBatch(x0, u0, want_active=True, sensitivities=True)
    assert np.array_equal(cmd, r2.cmd.cpu().numpy())
    s2 = r2.sensitivities
    assert np.array_equal(fl, s2.flags.cpu().numpy()) and (fl == 0).all()
    for a, n in ((kx, "d_x0"), (ku, "d_u0"), (ky, "d_yref")):
        assert a.tobytes() == getattr(s2, n).cpu().numpy().tobytes(), n
    # a NULL output is left alone
    _capi.check(lib.mpcx_lmpc_sensitivity_host(fresh._h, None, p(ku), None, None))
