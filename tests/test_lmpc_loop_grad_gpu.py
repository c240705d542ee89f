"""The backward pass of the closed loop on the GPU, through the C ABI and the Python front-end: every output of every case of
tests/loop_grad_ref.py against the truth at loop_grad_ref.KERNEL_TOL -- the only bound here, none comes from a GPU run --, per instance and summed,
the two kernel forms bit for bit, determinism, seeds refilled in place, warm and cold forward loops, the single step against sensitivityBatch, a
flagged instance, NULL outputs and the error codes, the autograd function and one descent step."""
import ctypes as C
import functools

import numpy as np
import pytest

import loop_grad_ref as G
import sens_ref as S

pytestmark = pytest.mark.gpu

BASIC = ("x0", "u0", "yref", "noise", "plant")
ALL = BASIC + ("oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")


@functools.lru_cache(maxsize=None)
def controller(fam):
    from libmpc_amd import LMPC
    sp = G.family(fam)[0]
    return S.configure(LMPC(*sp["dims"], device=0), sp)


def loop_kwargs(R, T, warm=True):
    kind, Ap, Bp, Bdp = T["plant"]
    kw = dict(yref=T["yref"], preview=R["preview"], noise=T["noise"], warm=warm)
    if kind == "other":
        kw["plant"] = (Ap, Bp, Bdp)
    elif kind == "batch":
        kw["plants"] = (Ap, Bp, Bdp)
    return kw


def run(name, B=None, reduce=False, warm=True, want=None, **over):
    """simulate + gradient of a case on a batch of B (the case's distinct instances repeated): (ClosedLoopResult, tiled inputs)"""
    import torch
    R = G.reference(name)
    T = G.tiled(R, B or R["n"])
    T.update(over)
    c = controller(G.CASES[name][0])
    want = want or (ALL if R["theta"] else BASIC)
    r = c.simulate(T["x0"], T["u0"], R["ticks"], gradient=dict(seed_x=T["seed_x"], seed_u=T["seed_u"], reduce=reduce, want=want), **loop_kwargs(R, T, warm))
    torch.cuda.synchronize()
    return r, T


def outputs(g):
    return {n: getattr(g, n).cpu().numpy() for n in G.PER_INSTANCE + G.SUMMED if getattr(g, n) is not None and getattr(g, n).numel()}


def check_case(name, B):
    R = G.reference(name)
    r, T = run(name, B)
    of = T["of"]
    truth, use = G.stacked(R, of, G.PER_INSTANCE + G.SUMMED)
    assert len(of) - len(use) <= G.SKIP_CAP * len(of)
    o = outputs(r.gradient)
    flags = r.gradient.flags.cpu().numpy()
    assert (flags[use] == 0).all() and (r.status.cpu().numpy()[:, use] == 0).all()
    # the device ran the truth's loop (a check of the test's own wiring, at the loosest tolerance the solve kernels are held to; no accuracy claim)
    fx = np.stack([R["fwd"][of[i]]["x"] for i in use], axis=1)
    ferr = np.abs(r.x.cpu().numpy()[:, use] - fx).max() / max(1.0, np.abs(fx).max())
    assert ferr <= 1e-7, ferr
    worst = {}
    for n, t in truth.items():
        got = o[n][:, use] if n == "d_noise" else o[n][use]
        assert got.shape == t.shape, (n, got.shape, t.shape)
        ax = tuple(a for a in range(t.ndim) if a != (1 if n == "d_noise" else 0))
        scale = np.maximum(1.0, np.abs(t).max(axis=ax, keepdims=True))           # per instance and output
        worst[n] = float((np.abs(got - t) / scale).max())
    print(f"{name} B={B}: forward {ferr:.1e}; worst error / bound {max(worst.values()):.2e} / {G.KERNEL_TOL:.2e} ({max(worst, key=worst.get)}), {len(use)} of {len(of)} instances")
    assert max(worst.values()) <= G.KERNEL_TOL, worst
    # the summed form: the per-instance bound added up over the instances that enter
    rr, _ = run(name, B, reduce=True)
    assert int(rr.gradient.n_used.item()) == int((flags == 0).sum()) and np.array_equal(rr.gradient.flags.cpu().numpy(), flags)
    orr = outputs(rr.gradient)
    for n in G.PER_INSTANCE:
        assert orr[n].tobytes() == o[n].tobytes(), n                              # the per-instance outputs do not depend on the form
    if len(use) == len(of):
        for n in G.SUMMED:
            if n in truth:
                bound = G.KERNEL_TOL * np.maximum(1.0, np.abs(truth[n]).max(axis=tuple(range(1, truth[n].ndim)))).sum()
                assert orr[n].shape == truth[n].shape[1:] and np.abs(orr[n] - truth[n].sum(axis=0)).max() <= bound, n
    return r, rr


@pytest.mark.parametrize("name,B", [(n, b) for n in G.CASES for b in G.BATCHES.get(n, (G.CASES[n][1],))])
def test_every_output_matches_the_truth(name, B):
    check_case(name, B)


def test_smallest_is_the_closed_form():
    """nz = 1 and nothing active: the loop is linear in [x; lastU] with cmd = -K x + Ku lastU + const, K and Ku from the Jacobian mode, so d_x0 and
    d_u0 are a matrix recursion -- with Ku = 0 it is d_x0 = sum_k ((A_p - B_p K)')^k (seed_x[k] - K' seed_u[k]); the rate weight makes Ku non-zero"""
    import torch
    R = G.reference("smallest")
    r, T = run("smallest", 16)
    c = controller("smallest")
    s = c.optimizeBatch(T["x0"], T["u0"], yref=T["yref"], want_active=True, sensitivities=True)
    torch.cuda.synchronize()
    K = -s.sensitivities.d_x0.cpu().numpy()                                       # [B, nu, nx]
    Ku = s.sensitivities.d_u0.cpu().numpy()
    sp = R["sp"]
    got, gotu = r.gradient.d_x0.cpu().numpy(), r.gradient.d_u0.cpu().numpy()
    assert (s.sensitivities.flags.cpu().numpy() == 0).all()
    for b in range(16):
        # state [x; lastU]: x+ = (A - B K) x + B Ku u, u+ = -K x + Ku u
        M = np.block([[sp["A"] - sp["B"] @ K[b], sp["B"] @ Ku[b]], [-K[b], Ku[b]]])
        lam = np.concatenate([T["seed_x"][R["ticks"], b], np.zeros(1)])
        for k in range(R["ticks"] - 1, -1, -1):
            lam = M.T @ (lam + np.concatenate([np.zeros(1), T["seed_u"][k, b]])) + np.concatenate([T["seed_x"][k, b], np.zeros(1)])
        assert abs(got[b, 0] - lam[0]) <= G.KERNEL_TOL * max(1.0, abs(lam[0])) and abs(gotu[b, 0] - lam[1]) <= G.KERNEL_TOL * max(1.0, abs(lam[1])), b


def test_the_two_forms_agree_bit_for_bit():
    """one plant for the batch through the uniform kernels, and plant_batch filled with that plant through the (instance, row) kernels"""
    R = G.reference("full_t2")
    for B in (7, 65):
        T = G.tiled(R, B)
        sp = R["sp"]
        nx = sp["dims"][0]
        same = ("batch", np.broadcast_to(sp["A"], (B,) + sp["A"].shape).copy(), np.broadcast_to(sp["B"], (B,) + sp["B"].shape).copy(),
                np.broadcast_to(sp["Bd"], (B,) + sp["Bd"].shape).copy())
        for reduce in (False, True):
            a, _ = run("full_t2", B, reduce)
            b, _ = run("full_t2", B, reduce, plant=same)
            oa, ob = outputs(a.gradient), outputs(b.gradient)
            assert a.x.cpu().numpy().tobytes() == b.x.cpu().numpy().tobytes()
            assert set(oa) == set(ob) and len(oa) == len(G.PER_INSTANCE + G.SUMMED)
            for n in oa:
                assert oa[n].tobytes() == ob[n].tobytes(), (B, reduce, n)


def test_two_runs_agree_and_refilled_seeds_are_followed():
    import torch
    R = G.reference("full_batch")
    T = G.tiled(R, 65)
    c = controller("full")
    loop = c.make_loop(T["x0"], T["u0"], R["ticks"], **loop_kwargs(R, T))
    other = np.random.default_rng(5).normal(size=T["seed_x"].shape)
    try:
        c.run_loop(loop)
        for reduce in (True, False):
            g = c.make_loop_gradient(loop, T["seed_x"], T["seed_u"], reduce=reduce)
            g2 = c.make_loop_gradient(loop, other, T["seed_u"], reduce=reduce)
            try:
                first = outputs(c.run_loop_gradient(g)); torch.cuda.synchronize()
                second = outputs(c.run_loop_gradient(g)); torch.cuda.synchronize()
                for n in first:
                    assert first[n].tobytes() == second[n].tobytes(), n            # the same bits
                fresh = outputs(c.run_loop_gradient(g2)); torch.cuda.synchronize()
                g.seed_x.copy_(torch.as_tensor(other))                             # in place: the next run reads the new seeds
                third = outputs(c.run_loop_gradient(g)); torch.cuda.synchronize()
                assert any(third[n].tobytes() != first[n].tobytes() for n in third)
                for n in third:
                    assert third[n].tobytes() == fresh[n].tobytes(), n
            finally:
                c.destroy_loop_gradient(g); c.destroy_loop_gradient(g2)
    finally:
        c.destroy_loop(loop)


def test_warm_and_cold_forward_loops():
    """the backward pass re-solves cold: carried working sets in the forward run change nothing beyond the solves' own rounding"""
    w, _ = run("full")
    k, _ = run("full", warm=False)
    ow, ok_ = outputs(w.gradient), outputs(k.gradient)
    assert (w.gradient.flags.cpu().numpy() == 0).all() and (k.gradient.flags.cpu().numpy() == 0).all()
    for n in ow:
        ax = tuple(a for a in range(ow[n].ndim) if a != (1 if n == "d_noise" else 0))
        scale = np.maximum(1.0, np.abs(ow[n]).max(axis=ax, keepdims=True))
        assert (np.abs(ow[n] - ok_[n]) / scale).max() <= G.KERNEL_TOL, n


def test_a_single_step_reproduces_the_sensitivity_launches():
    """ticks = 1, seed_x = None, seed_u = e at tick 0: c_0 = e, so every output is that of the three launches on the solved step, bit for bit"""
    import torch
    R = G.reference("full_t1")
    c = controller("full")
    e = R["seed_u"][0]
    r = c.simulate(R["x0"], R["u0"], 1, yref=R["yref"], noise=R["noise"], gradient=dict(seed_u=R["seed_u"], reduce=False, want=ALL))
    s = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    v = c.sensitivityBatch(s.active_lower, s.active_upper, status=s.status, seed_cmd=e)
    p = c.paramSensitivityBatch(s, seed_cmd=e, want=("oweight", "uweight", "duweight"))
    m = c.modelSensitivityBatch(s, seed_cmd=e)
    torch.cuda.synchronize()
    g = r.gradient
    assert torch.equal(r.u[0], s.cmd)
    for got, ref, n in ((g.d_x0, v.d_x0, "x0"), (g.d_u0, v.d_u0, "u0"), (g.d_yref, v.d_yref, "yref"), (g.d_oweight, p.d_oweight, "oweight"),
                        (g.d_uweight, p.d_uweight, "uweight"), (g.d_duweight, p.d_duweight, "duweight"), (g.d_A, m.d_A, "A"), (g.d_B, m.d_B, "B"),
                        (g.d_C, m.d_C, "C"), (g.d_Bd, m.d_Bd, "Bd"), (g.d_Dd, m.d_Dd, "Dd")):
        assert torch.equal(got, ref), n
    assert torch.equal(g.d_noise[0], torch.zeros_like(g.d_noise[0])) and not g.d_plant_A.abs().max().item()


def test_a_flagged_instance_is_nan_and_absent_from_the_sums():
    """the construction of test_infeasible_instances_both_modes: a state outside its step-0 bound, here at tick 0 of instance 3"""
    import torch
    from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc
    c = quadrotor_lmpc(10, device=0)
    x0, u0, yref = quadrotor_batch(8)
    bad = x0.copy(); bad[3, 0] = 1.0
    rg = np.random.default_rng(2)
    sx, su = rg.normal(size=(3, 8, c.nx)), rg.normal(size=(2, 8, c.nu))
    kw = dict(seed_x=sx, seed_u=su, want=ALL)
    good = c.simulate(x0, u0, 2, yref=yref, gradient=dict(reduce=False, **kw)).gradient
    g = c.simulate(bad, u0, 2, yref=yref, gradient=dict(reduce=False, **kw)).gradient
    gs = c.simulate(bad, u0, 2, yref=yref, gradient=dict(reduce=True, **kw)).gradient
    torch.cuda.synchronize()
    flags = g.flags.cpu().numpy()
    others = np.delete(np.arange(8), 3)
    assert flags[3] != 0 and (flags[others] == 0).all() and (good.flags.cpu().numpy() == 0).all()
    og, oo, os_ = outputs(good), outputs(g), outputs(gs)
    for n in oo:
        per = (lambda a: a[:, 3]) if n == "d_noise" else (lambda a: a[3])
        rest = (lambda a: a[:, others]) if n == "d_noise" else (lambda a: a[others])
        assert np.isnan(per(oo[n])).all(), n
        assert rest(oo[n]).tobytes() == rest(og[n]).tobytes(), n                   # nobody else is disturbed
    assert int(gs.n_used.item()) == 7 and np.array_equal(gs.flags.cpu().numpy(), flags)
    for n in G.SUMMED:
        if n in oo:
            ref = oo[n][others].sum(axis=0)
            bound = 8 * 2.0 ** -52 * np.abs(oo[n][others]).sum(axis=0)
            assert np.isfinite(os_[n]).all() and (np.abs(os_[n] - ref) <= bound).all(), n


def test_null_outputs_error_codes_and_the_descriptor():
    import torch
    from libmpc_amd import LMPC, MpcxError, _capi
    lib = _capi.lib()
    assert C.sizeof(_capi.LoopGradDesc) == lib.mpcx_lmpc_loop_grad_desc_size()
    R = G.reference("full_t2")
    c = controller("full")
    full, _ = run("full_t2")
    part, _ = run("full_t2", want=("u0", "B", "duweight"))
    g = part.gradient
    assert all(getattr(g, n) is None for n in ("d_x0", "d_yref", "d_noise", "d_plant_A", "d_oweight", "d_uweight", "d_A", "d_C", "d_Bd", "d_Dd"))
    for n in ("d_u0", "d_B", "d_duweight"):
        assert torch.equal(getattr(g, n), getattr(full.gradient, n)), n
    loop = c.make_loop(R["x0"], R["u0"], R["ticks"], yref=R["yref"])
    stream = torch.cuda.Stream()
    h = C.c_void_p()
    d = _capi.LoopGradDesc()
    sx = torch.zeros((R["ticks"] + 1, R["n"], c.nx), dtype=torch.float64, device="cuda")
    try:
        s = C.c_void_p(stream.cuda_stream)
        assert lib.mpcx_lmpc_loop_grad_create(loop.handle, None, s, C.byref(h)) == _capi.E_INVALID
        assert lib.mpcx_lmpc_loop_grad_create(loop.handle, C.byref(d), s, C.byref(h)) == _capi.E_INVALID and b"seed" in lib.mpcx_last_error()
        d.seed_x = sx.data_ptr()
        assert lib.mpcx_lmpc_loop_grad_create(None, C.byref(d), s, C.byref(h)) == _capi.E_INVALID
        d.reduce = 2
        assert lib.mpcx_lmpc_loop_grad_create(loop.handle, C.byref(d), s, C.byref(h)) == _capi.E_INVALID
        d.reduce = 0
        # an observed loop: a follow-up, and said so -- ahead of any look at the loop's state
        L = np.zeros((c.nx, c.ny))
        obs = c.make_loop(R["x0"], R["u0"], R["ticks"], yref=R["yref"], observer=L)
        try:
            assert lib.mpcx_lmpc_loop_grad_create(obs.handle, C.byref(d), s, C.byref(h)) == _capi.E_INVALID and b"follow-up" in lib.mpcx_last_error()
        finally:
            c.destroy_loop(obs)
        # every output NULL is a valid, if pointless, request
        assert lib.mpcx_lmpc_loop_grad_create(loop.handle, C.byref(d), s, C.byref(h)) == _capi.OK
        c.run_loop(loop)
        assert lib.mpcx_lmpc_loop_grad_run(h, None) == _capi.OK
        torch.cuda.synchronize()
        # a setter since the loop's creation invalidates both
        sp = R["sp"]
        assert c.setObjectiveWeights(sp["OW"], sp["UW"], sp["DUW"])
        assert lib.mpcx_lmpc_loop_grad_run(h, None) == _capi.E_STATE
        h2 = C.c_void_p()
        assert lib.mpcx_lmpc_loop_grad_create(loop.handle, C.byref(d), s, C.byref(h2)) == _capi.E_STATE
        assert lib.mpcx_lmpc_loop_grad_destroy(h) == _capi.OK and lib.mpcx_lmpc_loop_grad_destroy(None) == _capi.OK
    finally:
        c.destroy_loop(loop)
    # a bank's loop
    from libmpc_amd import LMPCHetero
    bank = LMPCHetero([c, c], device=0)
    bl = bank.make_loop(R["x0"][:2], R["u0"][:2], 2)
    try:
        assert lib.mpcx_lmpc_loop_grad_create(bl.handle, C.byref(d), C.c_void_p(stream.cuda_stream), C.byref(h)) == _capi.E_INVALID and b"bank" in lib.mpcx_last_error()
    finally:
        bank.destroy_loop(bl)


@pytest.mark.parametrize("name", ["smallest", "full"])
def test_autograd_against_the_truth(name):
    """lmpc_closed_loop on B = 4: the gradients autograd returns for a loss sum(seed_x * x) + sum(seed_u * u) against the reference's, not torch's
    own differencing; plant and controller model are one tensor here, so their gradients arrive added up"""
    import torch
    from libmpc_amd import lmpc_closed_loop
    R = G.reference(name)
    sp = R["sp"]
    c = controller(G.CASES[name][0])
    nb = 4
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True)
    x0, u0, yref, noise = t(R["x0"][:nb]), t(R["u0"][:nb]), t(R["yref"][:nb]), t(R["noise"][:, :nb])
    ow, uw, dw, A, B, Cm = t(sp["OW"]), t(sp["UW"]), t(sp["DUW"]), t(sp["A"]), t(sp["B"]), t(sp["C"])
    kw = dict(Bd=t(sp["Bd"]), Dd=t(sp["Dd"])) if "Bd" in sp else {}
    x, u = lmpc_closed_loop(c, x0, u0, R["ticks"], yref=yref, noise=noise, OWeight=ow, UWeight=uw, DeltaUWeight=dw, A=A, B=B, C=Cm, **kw)
    sx = torch.as_tensor(R["seed_x"][:, :nb], device="cuda"); su = torch.as_tensor(R["seed_u"][:, :nb], device="cuda")
    ((x * sx).sum() + (u * su).sum()).backward()
    assert all(R["usable"][:nb])
    truth, use = G.stacked(R, np.arange(nb), G.PER_INSTANCE + G.SUMMED)
    tol = lambda v: G.KERNEL_TOL * np.maximum(1.0, np.abs(v).max(axis=tuple(range(1, v.ndim)))).sum()
    for got, n in ((x0, "d_x0"), (u0, "d_u0"), (yref, "d_yref")):
        v = truth[n]
        assert (np.abs(got.grad.cpu().numpy() - v).max(axis=1) <= G.KERNEL_TOL * np.maximum(1.0, np.abs(v).max(axis=1))).all(), n
    assert np.abs(noise.grad.cpu().numpy() - truth["d_noise"]).max() <= G.KERNEL_TOL * max(1.0, np.abs(truth["d_noise"]).max())
    for got, n in ((ow, "d_oweight"), (uw, "d_uweight"), (dw, "d_duweight"), (Cm, "d_C")) + ((("Dd" in kw and kw["Dd"], "d_Dd"),) if kw else ()):
        assert np.abs(got.grad.cpu().numpy() - truth[n].sum(axis=0)).max() <= tol(truth[n]), n
    for got, n, pn in ((A, "d_A", "d_plant_A"), (B, "d_B", "d_plant_B")) + (((kw["Bd"], "d_Bd", "d_plant_Bd"),) if kw else ()):
        both = truth[n] + truth[pn]
        assert np.abs(got.grad.cpu().numpy() - both.sum(axis=0)).max() <= tol(truth[n]) + tol(truth[pn]), n
    assert S.configure(c, sp) is c                                                 # (the controller as the other tests expect it)


def test_one_descent_step_on_the_output_weight_lowers_a_tracking_loss():
    import torch
    from libmpc_amd import LMPC, lmpc_closed_loop
    sp = G.family("full")[0]
    R = G.reference("full")
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    x0, u0, yref = (torch.as_tensor(R[k], device="cuda") for k in ("x0", "u0", "yref"))
    Cm = torch.as_tensor(sp["C"], device="cuda")

    def loss(ow):
        x, u = lmpc_closed_loop(c, x0, u0, 5, yref=yref, OWeight=ow, UWeight=torch.as_tensor(sp["UW"]), DeltaUWeight=torch.as_tensor(sp["DUW"]))
        return ((x[1:] @ Cm.T - yref) ** 2).sum()
    ow = torch.tensor(sp["OW"], dtype=torch.float64, device="cuda", requires_grad=True)
    l0 = loss(ow)
    l0.backward()
    g = ow.grad
    assert torch.isfinite(g).all() and g.abs().max() > 0
    step = 0.05 * float(ow.detach().abs().max() / g.abs().max())
    l1 = loss((ow.detach() - step * g).clamp_min(1e-3))
    print(f"tracking loss {float(l0.detach()):.6f} -> {float(l1.detach()):.6f}")
    assert float(l1.detach()) < float(l0.detach())
