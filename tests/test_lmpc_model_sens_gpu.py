"""Model sensitivities of a solved batch on the GPU, through the C ABI and the Python front-end: the gradients of every family
against the truth of tests/model_sens_ref.py at model_sens_ref.KERNEL_TOL, flags, the reduced form and its determinism, the reference modes of
the solved batch, a perturbed controller, autograd, the host form and the C++ method."""
import copy
import functools
import os

import numpy as np
import pytest

import linear_ref as LR
import model_sens_ref as Mo
import sens_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("d_A", "d_B", "d_C", "d_Bd", "d_Dd")


def _np(o):
    return {n: getattr(o, n).cpu().numpy() for n in OUTS if getattr(o, n) is not None}


@functools.lru_cache(maxsize=None)
def solved(name):
    """the family's controller on the device, its solve and the per-instance gradients for the reference's seeds"""
    import torch
    from libmpc_amd import LMPC
    R = Mo.reference(name)
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    g = c.modelSensitivityBatch(r, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"])
    torch.cuda.synchronize()
    return c, r, g


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _usable(name):
    """instances whose truth exists and whose active set on the device equals the oracle's on the compared rows"""
    R = Mo.reference(name)
    c, r, g = solved(name)
    res, sp = R["res"], R["sp"]
    keep = LR.compared_rows(sp)
    m = int(res["ncon"])
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == (res["active_lower"][:, keep] != 0)).all(axis=1) & (up[:, keep] == (res["active_upper"][:, keep] != 0)).all(axis=1)
    st = r.status.cpu().numpy()
    use = [b for b in range(len(st)) if R["truth"][b] is not None and same[b] and st[b] == 0]
    assert len(st) - len(use) <= Mo.SKIP_CAP * len(st), (name, len(use), len(st))
    return use


def _g(o, b):
    return {k: o[n][b] for k, n in zip(Mo.MODEL, OUTS) if n in o}


@pytest.mark.parametrize("name", Mo.FAMILIES)
def test_gradients_match_the_truth(name):
    R = Mo.reference(name)
    c, r, g = solved(name)
    use = _usable(name)
    o = _np(g)
    flags = g.flags.cpu().numpy()
    assert (flags[use] == 0).all()
    assert o["d_A"].shape == (len(flags), c.nx, c.nx) and o["d_B"].shape == (len(flags), c.nx, c.nu) and o["d_C"].shape == (len(flags), c.ny, c.nx)
    assert ("d_Bd" in o) == (c.ndu > 0) and (c.ndu == 0 or (o["d_Bd"].shape == (len(flags), c.nx, c.ndu) and o["d_Dd"].shape == (len(flags), c.ny, c.ndu)))
    worst = max(Mo.compare(R["truth"][b], _g(o, b)) for b in use)
    count = r.active_count.cpu().numpy()
    print(f"{name}: worst error / bound {worst:.2e} / {Mo.KERNEL_TOL:.2e}, {len(use)} of {len(flags)} instances, active rows {count[use].min()} .. {count[use].max()}")
    assert worst <= Mo.KERNEL_TOL
    if name == "soft":
        assert (count[use] > c.info()["nz"]).any()


def test_flags_nan_and_the_reduced_form():
    import torch
    R = Mo.reference("full")
    c, r, g = solved("full")
    per = _np(g)
    B = per["d_A"].shape[0]
    d = R["tr"].pb.d
    words = c.info()["active_words"]
    # instance 5 not solved; instance 7 with the box row and the step-0 rate row of input 0, which are parallel
    st = r.status.clone(); st[5] = 2
    al = r.active_lower.clone(); au = r.active_upper.clone()
    lo = np.zeros((1, 32 * words), bool); up = np.zeros((1, 32 * words), bool)
    lo[0, d.neq + d.na + c.nx] = True; up[0, d.neq + d.off_du] = True
    al[7] = torch.as_tensor(S.pack_bits(lo, words)[0]); au[7] = torch.as_tensor(S.pack_bits(up, words)[0])
    b2, res2, keep2 = c.make_batch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    c.launch(b2, None, keep2)
    res2.status.copy_(st); res2.active_lower.copy_(al); res2.active_upper.copy_(au)
    g2 = c.modelSensitivityBatch(b2, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"])
    o2 = _np(g2)
    f2 = g2.flags.cpu().numpy()
    assert f2[5] == 1 and f2[7] == 2 and (np.delete(f2, [5, 7]) == g.flags.cpu().numpy()[np.delete(np.arange(B), [5, 7])]).all()
    others = np.delete(np.arange(B), [5, 7])
    for n in OUTS:
        assert np.isnan(o2[n][5]).all() and np.isnan(o2[n][7]).all()
        assert o2[n][others].tobytes() == per[n][others].tobytes()              # nothing else is disturbed
    # the reduced form: the float sum of the per-instance outputs, in a fixed order
    used = f2 == 0
    red = [c.modelSensitivityBatch(b2, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], reduce=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert int(red[0].n_used.item()) == used.sum() and used.sum() < B
    assert torch.equal(red[0].flags, g2.flags)
    o = _np(red[0])
    for n in OUTS:
        ref = o2[n][used].sum(axis=0)
        bound = B * 2.0 ** -52 * np.abs(o2[n][used]).sum(axis=0)
        assert o[n].shape == ref.shape and (np.abs(o[n] - ref) <= bound).all(), n
        assert torch.equal(getattr(red[0], n), getattr(red[1], n)), n                # two launches: the same bits
    # outputs that are not asked for are not needed by the others
    part = c.modelSensitivityBatch(b2, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], want=("B", "Dd"))
    assert part.d_A is None and part.d_C is None and part.d_Bd is None
    assert np.array_equal(part.d_B.cpu().numpy()[others], o2["d_B"][others]) and np.array_equal(part.d_Dd.cpu().numpy()[others], o2["d_Dd"][others])


def _agree(c, R, kw1, kw2):
    import torch
    outs = []
    for kw in (kw1, kw2):
        rr = c.optimizeBatch(R["x0"], R["u0"], want_active=True, want_sequence=True, **kw)
        gg = c.modelSensitivityBatch(rr, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"])
        torch.cuda.synchronize()
        outs.append((rr, gg))
    (r1, g1), (r2, g2) = outs
    same = (torch.equal(r1.active_lower, r2.active_lower) and torch.equal(r1.active_upper, r2.active_upper))
    f1, f2 = g1.flags.cpu().numpy(), g2.flags.cpu().numpy()
    assert same and np.array_equal(f1, f2) and (f1 == 0).sum() >= 0.9 * len(f1)
    ok = f1 == 0
    o1, o2 = _np(g1), _np(g2)
    scale = max(1.0, max(np.abs(o1[n][ok]).max() for n in o1))
    for n in o1:
        assert np.abs(o1[n][ok] - o2[n][ok]).max() <= 2 * Mo.KERNEL_TOL * scale, n
    assert max(np.abs(o1[n][ok]).max() for n in o1) > 1e-3


def test_reference_modes_of_the_solved_batch_agree():
    """the refs family (input and rate references that differ per step): the controller's own references (MPCX_REF_SHARED) against the same
    matrices per instance and step (MPCX_REF_PER_STEP); references constant along the horizon per instance (MPCX_REF_PER_INSTANCE) against
    their per-step tiles.  Each result is within KERNEL_TOL of the truth, so two of them differ by at most twice that"""
    R = Mo.reference("refs")
    c, r, g = solved("refs")
    sp = R["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    B = len(R["x0"])
    rg = np.random.default_rng(5)
    t = lambda m: np.tile(np.asarray(m, float).T[None], (B, 1, 1))             # [n x ph] -> [B, ph, n]
    uc, dc = 0.2 * rg.normal(size=(B, nu)), 0.05 * rg.normal(size=(B, nu))
    _agree(c, R, dict(), dict(yref=t(sp["yref"]), uref=t(sp["uref"]), duref=t(sp["duref"])))
    _agree(c, R, dict(yref=R["yref"], uref=uc, duref=dc),
           dict(yref=np.tile(R["yref"][:, None, :], (1, ph, 1)), uref=np.tile(uc[:, None, :], (1, ph, 1)), duref=np.tile(dc[:, None, :], (1, ph, 1))))


def test_exogenous_input_modes_of_the_solved_batch_agree():
    """the ndu2 family: the controller's own exogenous inputs, which differ per step (MPCX_REF_SHARED), against their per-step tiles; and a
    controller whose exogenous inputs are constant along the horizon against the same constants per instance (MPCX_REF_PER_INSTANCE)"""
    from libmpc_amd import LMPC
    R = Mo.reference("ndu2")
    c, r, g = solved("ndu2")
    sp = R["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    B = len(R["x0"])
    _agree(c, R, dict(yref=R["yref"]), dict(yref=R["yref"], dmeas=np.tile(sp["dmeas"].T[None], (B, 1, 1))))
    sp2 = copy.deepcopy(sp)
    sp2["dmeas"] = np.tile(sp["dmeas"][:, :1], (1, ph))
    c2 = S.configure(LMPC(*sp["dims"], device=0), sp2)
    _agree(c2, R, dict(yref=R["yref"]), dict(yref=R["yref"], dmeas=np.tile(sp2["dmeas"][:, 0][None], (B, 1))))


@pytest.mark.parametrize("name", ["full", "soft"])
def test_a_perturbed_controller_moves_cmd_as_the_gradient_says(name):
    """delta = 1e-4 times a random direction on A, B, C, Bd and Dd, set up again and solved on the GPU: seed . cmd' against
    seed . cmd + <g, delta> within 1e-5 relative, on instances whose active set did not change; the controller is also solved at minus delta,
    and half the difference of the two solves is held to <g, delta> within 1e-2 of its size plus 1e-9, on at least eight instances with
    |<g, delta>| >= 1e-6: the bars and the reasoning of tests/test_lmpc_param_sens_gpu.py"""
    import torch
    from libmpc_amd import LMPC
    R = Mo.reference(name)
    c, r, _ = solved(name)
    sp = R["sp"]
    seed = R["seed_cmd"]
    g = c.modelSensitivityBatch(r, seed_cmd=seed)
    rg = np.random.default_rng(23)
    mats = [m for m in Mo.MODEL if m in sp]
    delta = {m: 1e-4 * rg.normal(size=sp[m].shape) for m in mats}
    res = []
    for sign in (1.0, -1.0):
        sp2 = copy.deepcopy(sp)
        for m in mats:
            sp2[m] = sp[m] + sign * delta[m]
        c2 = S.configure(LMPC(*sp["dims"], device=0), sp2)
        res.append(c2.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True))
    torch.cuda.synchronize()
    r2, r3 = res
    cmd3 = r3.cmd.cpu().numpy()
    same3 = ((r.active_lower == r3.active_lower).all(dim=1) & (r.active_upper == r3.active_upper).all(dim=1) & (r3.status == 0)).cpu().numpy()
    o = _np(g)
    cmd, cmd2 = r.cmd.cpu().numpy(), r2.cmd.cpu().numpy()
    same = (r.active_lower == r2.active_lower).all(dim=1) & (r.active_upper == r2.active_upper).all(dim=1) & (r.status == 0) & (r2.status == 0)
    use = [b for b in np.nonzero(same.cpu().numpy())[0] if g.flags[b].item() == 0]
    assert len(use) >= 0.75 * len(cmd), (name, len(use))
    worst, worst_lin, biting = 0.0, 0.0, 0
    for b in use:
        lin = sum((o[n][b] * delta[m]).sum() for m, n in zip(Mo.MODEL, OUTS) if m in delta)
        pred, act = seed[b] @ cmd[b] + lin, seed[b] @ cmd2[b]
        err = abs(pred - act) / max(abs(act), 1e-12)
        worst = max(worst, err)
        assert err <= 1e-5, (name, b, pred, act, lin)
        if same3[b]:
            half = 0.5 * (seed[b] @ cmd2[b] - seed[b] @ cmd3[b])
            assert abs(half - lin) <= 1e-2 * abs(lin) + 1e-9, (name, b, half, lin)
            if abs(lin) >= 1e-6:
                biting += 1
                worst_lin = max(worst_lin, abs(half - lin) / abs(lin))
    print(f"{name}: perturbed controller, worst relative error {worst:.2e} on {len(use)} instances; central difference against <g, delta>: worst {worst_lin:.2e} relative on {biting} instances with |<g, delta>| >= 1e-6")
    assert biting >= 8


def test_lmpc_cmd_model_fills_the_gradients_of_the_model():
    import torch
    from libmpc_amd import LMPC, lmpc_cmd_model
    R = Mo.reference("full")
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    dev = torch.device("cuda", 0)
    W = [torch.tensor(sp[m], dtype=torch.float64, device=dev, requires_grad=True) for m in Mo.MODEL]
    x0 = torch.tensor(R["x0"], dtype=torch.float64, device=dev, requires_grad=True)
    u0 = torch.tensor(R["u0"], dtype=torch.float64, device=dev)
    yref = torch.tensor(R["yref"], dtype=torch.float64, device=dev)
    seed = torch.tensor(R["seed_cmd"], dtype=torch.float64, device=dev)
    cmd, status = lmpc_cmd_model(c, x0, u0, yref, *W, return_status=True)
    (seed * cmd).sum().backward()
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    assert (r.cmd - cmd.detach()).abs().max().item() <= 1e-12
    red = c.modelSensitivityBatch(r, seed_cmd=R["seed_cmd"], reduce=True)
    vjp = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_cmd=seed)
    torch.cuda.synchronize()
    assert int(red.n_used.item()) == len(R["x0"])
    for w, n in zip(W, OUTS):
        ref = getattr(red, n)                      # (a second solve of the same batch: the same gradient up to the solve's own rounding)
        assert w.grad is not None and w.grad.shape == w.shape and (w.grad - ref).abs().max().item() <= 1e-9 * max(1.0, ref.abs().max().item())
    assert all(w.grad.abs().max().item() > 1e-3 for w in W[:3])
    assert (x0.grad - vjp.d_x0).abs().max().item() <= 1e-9 * max(1.0, vjp.d_x0.abs().max().item()) and u0.grad is None
    # without the disturbance matrices: A, B, C alone, the controller keeps its own Bd, Dd
    W3 = [torch.tensor(sp[m], dtype=torch.float64, device=dev, requires_grad=True) for m in Mo.MODEL[:3]]
    cmd3 = lmpc_cmd_model(c, R["x0"], R["u0"], yref, *W3)
    (seed * cmd3).sum().backward()
    for w, n in zip(W3, OUTS):
        ref = getattr(red, n)
        assert (w.grad - ref).abs().max().item() <= 1e-9 * max(1.0, ref.abs().max().item())


def test_a_changed_controller_is_refused_until_it_is_solved_again():
    from libmpc_amd import LMPC, MpcxError, _capi
    R = Mo.reference("xrows16")
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    c.modelSensitivityBatch(r, seed_cmd=R["seed_cmd"])
    assert c.setStateSpaceModel(sp["A"] * 0.9, sp["B"], sp["C"])
    with pytest.raises(MpcxError) as e:
        c.modelSensitivityBatch(r, seed_cmd=R["seed_cmd"])
    assert e.value.code == _capi.E_STATE
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    assert (c.modelSensitivityBatch(r, seed_cmd=R["seed_cmd"]).flags.cpu().numpy() == 0).any()       # solved again: served, with Xq of the new model
    with pytest.raises(ValueError):
        c.modelSensitivityBatch(c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"]), seed_cmd=R["seed_cmd"])       # no active sets, no sequences


def test_host_form_against_the_batch_call():
    """mpcx_lmpc_model_sensitivity_host over the last mpcx_lmpc_solve_host, per instance and reduced, against the batch call on the same
    instances (shared references here and there); MPCX_E_STATE without sequences"""
    import ctypes as C
    import torch
    from libmpc_amd import LMPC, _capi
    R = Mo.reference("ndu2")
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    lib = _capi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    B = 5
    x0, u0, seed, seeds = (np.ascontiguousarray(R[k][:B]) for k in ("x0", "u0", "seed_cmd", "seed_input"))
    cmd = np.zeros((B, c.nu)); st = np.zeros(B, np.int32)
    assert lib.mpcx_lmpc_solve_host(c._h, B, ptr(x0), ptr(u0), ptr(cmd), None, ptr(st), None, None, None, None, None) == 0
    assert lib.mpcx_lmpc_model_sensitivity_host(c._h, ptr(seed), None, 0, None, None, None, None, None, None, None) == _capi.E_STATE      # no sequences kept
    seq = [np.zeros((B, c.ph + 1, n)) for n in (c.nx, c.ny, c.nu)]
    assert lib.mpcx_lmpc_solve_host(c._h, B, ptr(x0), ptr(u0), ptr(cmd), None, ptr(st), None, None, *(ptr(q) for q in seq)) == 0 and (st == 0).all()
    sizes = (c.nx * c.nx, c.nx * c.nu, c.ny * c.nx, c.nx * c.ndu, c.ny * c.ndu)
    r = c.optimizeBatch(x0, u0, want_active=True, want_sequence=True)
    guard = 7.5e200
    for reduce in (0, 1):
        lead = 1 if reduce else B
        out = [np.full(lead * n + 8, guard) for n in sizes]
        fl = np.full(B, -1, np.int32); nu_ = np.full(1, -1, np.int32)
        assert lib.mpcx_lmpc_solve_host(c._h, B, ptr(x0), ptr(u0), ptr(cmd), None, ptr(st), None, None, *(ptr(q) for q in seq)) == 0
        assert lib.mpcx_lmpc_model_sensitivity_host(c._h, ptr(seed), ptr(seeds), reduce, *(ptr(o) for o in out), ptr(fl), ptr(nu_)) == 0 and (fl == 0).all()
        g = c.modelSensitivityBatch(c.optimizeBatch(x0, u0, want_active=True, want_sequence=True), seed_cmd=seed, seed_input=seeds, reduce=bool(reduce))
        torch.cuda.synchronize()
        ref = [getattr(g, n).transpose(-1, -2).contiguous().cpu().numpy().ravel() for n in OUTS]
        for o, rr in zip(out, ref):
            assert (o[len(rr):] == guard).all() and np.abs(o[:len(rr)] - rr).max() <= 1e-9 * max(1.0, np.abs(rr).max())
        assert max(np.abs(rr).max() for rr in ref) > 1e-4 and (nu_[0] == B if reduce else nu_[0] == -1)


def test_cpp_model_sensitivities_against_differences_of_optimize():
    import subprocess
    from test_lmpc_model_sens import _build_cpp
    env = {k: v for k, v in os.environ.items() if k != "MPCX_DEVICE"}
    out = subprocess.run([_build_cpp(), "solve"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ model-sensitivity checks passed" in out.stdout
