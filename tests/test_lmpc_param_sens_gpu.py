"""Parameter sensitivities of a solved batch on the GPU, through the C ABI and the Python front-end: the gradients of every family
against the truth of tests/param_sens_ref.py at param_sens_ref.KERNEL_TOL, flags, the reduced form and its determinism, the reference modes of
the solved batch, a perturbed controller, autograd and the C++ method."""
import functools
import os

import numpy as np
import pytest

import linear_ref as LR
import param_sens_ref as P
import sens_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("d_oweight", "d_uweight", "d_duweight", "d_lower", "d_upper")


def _np(o):
    return {n: getattr(o, n).cpu().numpy() for n in OUTS}


@functools.lru_cache(maxsize=None)
def solved(name):
    """the family's controller on the device, its solve and the per-instance gradients for the reference's seeds"""
    import torch
    from libmpc_amd import LMPC
    R = P.reference(name)
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    g = c.paramSensitivityBatch(r, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"])
    torch.cuda.synchronize()
    return c, r, g


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _usable(name):
    """instances whose truth exists and whose active set on the device equals the oracle's on the compared rows"""
    R = P.reference(name)
    c, r, g = solved(name)
    res, sp = R["res"], R["sp"]
    keep = LR.compared_rows(sp)
    m = int(res["ncon"])
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == (res["active_lower"][:, keep] != 0)).all(axis=1) & (up[:, keep] == (res["active_upper"][:, keep] != 0)).all(axis=1)
    st = r.status.cpu().numpy()
    use = [b for b in range(len(st)) if R["truth"][b] is not None and same[b] and st[b] == 0]
    assert len(st) - len(use) <= P.SKIP_CAP * len(st), (name, len(use), len(st))
    return use


def _g(o, b):
    return {k: o[n][b] for k, n in zip(P.WEIGHTS + ("lower", "upper"), OUTS)}


@pytest.mark.parametrize("name", P.FAMILIES)
def test_gradients_match_the_truth(name):
    R = P.reference(name)
    c, r, g = solved(name)
    a = P.arrays(c)
    use = _usable(name)
    o = _np(g)
    flags = g.flags.cpu().numpy()
    assert (flags[use] == 0).all()
    assert o["d_oweight"].shape == (len(flags), c.ny, c.ph) and o["d_lower"].shape == (len(flags), c.info()["m_ref"])
    worst = max(P.compare(a, R["truth"][b], _g(o, b), blocked=(name == "blocked")) for b in use)
    count = r.active_count.cpu().numpy()
    print(f"{name}: worst error / bound {worst:.2e} / {P.KERNEL_TOL:.2e}, {len(use)} of {len(flags)} instances, active rows {count[use].min()} .. {count[use].max()}")
    assert worst <= P.KERNEL_TOL
    if name == "soft":
        assert (count[use] > c.info()["nz"]).any()


def test_flags_nan_and_the_reduced_form():
    import torch
    R = P.reference("full")
    c, r, g = solved("full")
    per = _np(g)
    B = per["d_lower"].shape[0]
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
    g2 = c.paramSensitivityBatch(b2, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"])
    o2 = _np(g2)
    f2 = g2.flags.cpu().numpy()
    assert f2[5] == 1 and f2[7] == 2 and (np.delete(f2, [5, 7]) == g.flags.cpu().numpy()[np.delete(np.arange(B), [5, 7])]).all()
    others = np.delete(np.arange(B), [5, 7])
    for n in OUTS:
        assert np.isnan(o2[n][5]).all() and np.isnan(o2[n][7]).all()
        assert o2[n][others].tobytes() == per[n][others].tobytes()              # nothing else is disturbed
    # the reduced form: the float sum of the per-instance outputs, in a fixed order
    used = f2 == 0
    red = [c.paramSensitivityBatch(b2, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], reduce=True) for _ in range(2)]
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
    part = c.paramSensitivityBatch(b2, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], want=("uweight", "upper"))
    assert part.d_oweight is None and part.d_duweight is None and part.d_lower is None
    assert np.array_equal(part.d_uweight.cpu().numpy()[others], o2["d_uweight"][others]) and np.array_equal(part.d_upper.cpu().numpy()[others], o2["d_upper"][others])


def test_reference_modes_of_the_solved_batch_agree():
    """the refs family (input and rate references that differ per step): the controller's own references (MPCX_REF_SHARED) against the same
    matrices per instance and step (MPCX_REF_PER_STEP); references constant along the horizon per instance (MPCX_REF_PER_INSTANCE) against
    their per-step tiles.  Each result is within KERNEL_TOL of the truth, so two of them differ by at most twice that"""
    import torch
    R = P.reference("refs")
    c, r, g = solved("refs")
    sp = R["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    B = len(R["x0"])
    rg = np.random.default_rng(5)
    t = lambda m: np.tile(np.asarray(m, float).T[None], (B, 1, 1))             # [n x ph] -> [B, ph, n]
    uc, dc = 0.2 * rg.normal(size=(B, nu)), 0.05 * rg.normal(size=(B, nu))
    pairs = [(dict(), dict(yref=t(sp["yref"]), uref=t(sp["uref"]), duref=t(sp["duref"]))),
             (dict(yref=R["yref"], uref=uc, duref=dc), dict(yref=np.tile(R["yref"][:, None, :], (1, ph, 1)), uref=np.tile(uc[:, None, :], (1, ph, 1)), duref=np.tile(dc[:, None, :], (1, ph, 1))))]
    for kw1, kw2 in pairs:
        outs = []
        for kw in (kw1, kw2):
            rr = c.optimizeBatch(R["x0"], R["u0"], want_active=True, want_sequence=True, **kw)
            gg = c.paramSensitivityBatch(rr, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"])
            torch.cuda.synchronize()
            outs.append((rr, gg))
        (r1, g1), (r2, g2) = outs
        same = (torch.equal(r1.active_lower, r2.active_lower) and torch.equal(r1.active_upper, r2.active_upper))
        assert same and (g1.flags.cpu().numpy() == 0).all() and (g2.flags.cpu().numpy() == 0).all()
        o1, o2 = _np(g1), _np(g2)
        scale = max(1.0, max(np.abs(o1[n]).max() for n in OUTS))
        for n in OUTS:
            assert np.abs(o1[n] - o2[n]).max() <= 2 * P.KERNEL_TOL * scale, n
        assert max(np.abs(o1[n]).max() for n in OUTS[:3]) > 1e-3


@pytest.mark.parametrize("name", ["full", "soft"])
def test_a_perturbed_controller_moves_cmd_as_the_gradient_says(name):
    """delta = 1e-4 times a random direction on the three weight matrices, set up again and solved on the GPU: seed . cmd' against
    seed . cmd + <g, delta> within 1e-5 relative (the bar of the affine-law check of DESIGN 4.8), on instances whose active set did not change.
    That bar is relative to seed . cmd', of order one, while <g, delta> is of order 1e-5.  So the controller is also solved at minus delta:
    in half the difference of the two solves the second-order term cancels, and it is held to <g, delta> within 1e-2 of its size plus 1e-9
    (the third-order term, 1e-12, and the rounding of two solves on one active set, eps times a condition number of 1e6).  An instance
    whose first move is pinned on its bounds has a zero gradient, and the floor covers it; at least eight instances must have
    |<g, delta>| >= 1e-6, ten times what the floor hides at the 1e-2 bar, so that the relative bar is what decides for them"""
    import torch
    from libmpc_amd import LMPC
    R = P.reference(name)
    c, r, _ = solved(name)
    sp = R["sp"]
    seed = R["seed_cmd"]
    g = c.paramSensitivityBatch(r, seed_cmd=seed)
    rg = np.random.default_rng(23)
    delta = {w: 1e-4 * rg.uniform(0.0, 1.0, size=sp[w].shape) for w in P.WEIGHTS}          # (upwards: a weight stays non-negative)
    c2 = S.configure(LMPC(*sp["dims"], device=0), sp)
    assert c2.setObjectiveWeights(*(sp[w] + delta[w] for w in P.WEIGHTS))
    c2.setup()
    r2 = c2.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True)
    assert c2.setObjectiveWeights(*(sp[w] - delta[w] for w in P.WEIGHTS))
    c2.setup()
    r3 = c2.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True)
    torch.cuda.synchronize()
    cmd3 = r3.cmd.cpu().numpy()
    same3 = ((r.active_lower == r3.active_lower).all(dim=1) & (r.active_upper == r3.active_upper).all(dim=1) & (r3.status == 0)).cpu().numpy()
    o = _np(g)
    cmd, cmd2 = r.cmd.cpu().numpy(), r2.cmd.cpu().numpy()
    same = (r.active_lower == r2.active_lower).all(dim=1) & (r.active_upper == r2.active_upper).all(dim=1) & (r.status == 0) & (r2.status == 0)
    use = [b for b in np.nonzero(same.cpu().numpy())[0] if g.flags[b].item() == 0]
    assert len(use) >= 0.75 * len(cmd), (name, len(use))
    worst, worst_lin, biting = 0.0, 0.0, 0
    for b in use:
        lin = sum((o[n][b] * delta[w]).sum() for w, n in zip(P.WEIGHTS, OUTS))
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


def test_lmpc_cmd_params_fills_the_gradients_of_the_weights():
    import torch
    from libmpc_amd import LMPC, lmpc_cmd_params
    R = P.reference("full")
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    dev = torch.device("cuda", 0)
    W = [torch.tensor(sp[w], dtype=torch.float64, device=dev, requires_grad=True) for w in P.WEIGHTS]
    x0 = torch.tensor(R["x0"], dtype=torch.float64, device=dev, requires_grad=True)
    u0 = torch.tensor(R["u0"], dtype=torch.float64, device=dev)
    yref = torch.tensor(R["yref"], dtype=torch.float64, device=dev)
    seed = torch.tensor(R["seed_cmd"], dtype=torch.float64, device=dev)
    cmd, status = lmpc_cmd_params(c, x0, u0, yref, *W, return_status=True)
    (seed * cmd).sum().backward()
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    assert (r.cmd - cmd.detach()).abs().max().item() <= 1e-12
    red = c.paramSensitivityBatch(r, seed_cmd=R["seed_cmd"], reduce=True)
    vjp = c.sensitivityBatch(r.active_lower, r.active_upper, status=r.status, seed_cmd=seed)
    torch.cuda.synchronize()
    assert int(red.n_used.item()) == len(R["x0"])
    for w, n in zip(W, OUTS):
        ref = getattr(red, n)                      # (a second solve of the same batch: the same gradient up to the solve's own rounding)
        assert w.grad is not None and w.grad.shape == w.shape and (w.grad - ref).abs().max().item() <= 1e-9 * max(1.0, ref.abs().max().item())
        assert w.grad.abs().max().item() > 1e-3
    assert (x0.grad - vjp.d_x0).abs().max().item() <= 1e-9 * max(1.0, vjp.d_x0.abs().max().item()) and u0.grad is None


def test_a_changed_controller_is_refused_until_it_is_solved_again():
    from libmpc_amd import LMPC, MpcxError, _capi
    R = P.reference("rows16")
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    r = c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"], want_active=True, want_sequence=True)
    c.paramSensitivityBatch(r, seed_cmd=R["seed_cmd"])
    assert c.setObjectiveWeights(sp["OW"] * 2, sp["UW"], sp["DUW"])
    with pytest.raises(MpcxError) as e:
        c.paramSensitivityBatch(r, seed_cmd=R["seed_cmd"])
    assert e.value.code == _capi.E_STATE
    with pytest.raises(ValueError):
        c.paramSensitivityBatch(c.optimizeBatch(R["x0"], R["u0"], yref=R["yref"]), seed_cmd=R["seed_cmd"])       # no active sets, no sequences


def test_host_form_after_a_set_up_with_more_rows():
    """mpcx_lmpc_param_sensitivity_host before and after linear rows are added to the controller: m_ref grows between the two calls, the staging
    of the first must not serve the second; each against the batch call on the same instance"""
    import ctypes as C
    import torch
    from libmpc_amd import LMPC, _capi
    R = P.reference("rows16")
    sp = R["sp"]
    c = S.configure(LMPC(*sp["dims"], device=0), sp)
    lib = _capi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    b = int(np.argmin(R["res"]["n_active"]))               # (the smallest working set of the family: its first move is not pinned on bounds)
    x0, u0, seed, seeds = (np.ascontiguousarray(R[k][b:b + 1]) for k in ("x0", "u0", "seed_cmd", "seed_input"))
    sizes = []
    for rows in (0, 5):
        if rows:
            rg = np.random.default_rng(9)
            assert c.setLinearConstraints(rg.normal(size=(rows, c.nx)), rg.normal(size=(rows, c.nu)), np.full(rows, -50.0), np.full(rows, 50.0))
        m = c.info()["m_ref"]
        sizes.append(m)
        cmd = np.zeros((1, c.nu)); st = np.zeros(1, np.int32)
        seq = [np.zeros((1, c.ph + 1, n)) for n in (c.nx, c.ny, c.nu)]
        assert lib.mpcx_lmpc_solve_host(c._h, 1, ptr(x0), ptr(u0), ptr(cmd), None, ptr(st), None, None, *(ptr(q) for q in seq)) == 0 and st[0] == 0
        guard = 7.5e200
        out = [np.full(n + 8, guard) for n in (c.ny * c.ph, c.nu * c.ph, c.nu * c.ph, m, m)]
        fl = np.full(1, -1, np.int32)
        assert lib.mpcx_lmpc_param_sensitivity_host(c._h, ptr(seed), ptr(seeds), 0, *(ptr(o) for o in out), ptr(fl), None) == 0 and fl[0] == 0
        # the batch call on the same instance: shared references here and there
        r = c.optimizeBatch(x0, u0, want_active=True, want_sequence=True)
        g = c.paramSensitivityBatch(r, seed_cmd=seed, seed_input=seeds)
        torch.cuda.synchronize()
        ref = [getattr(g, n)[0].transpose(-1, -2).contiguous().cpu().numpy().ravel() if i < 3 else getattr(g, n)[0].cpu().numpy() for i, n in enumerate(OUTS)]
        for o, rr in zip(out, ref):
            assert (o[len(rr):] == guard).all() and np.abs(o[:len(rr)] - rr).max() <= 1e-9 * max(1.0, np.abs(rr).max())
        assert max(np.abs(rr).max() for rr in ref[:3]) > 1e-4
    assert sizes[1] == sizes[0] + 5 * (c.ph + 1)


def test_cpp_parameter_sensitivities_against_differences_of_optimize():
    import subprocess
    from test_lmpc_param_sens import _build_cpp
    env = {k: v for k, v in os.environ.items() if k != "MPCX_DEVICE"}
    out = subprocess.run([_build_cpp(), "solve"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ parameter-sensitivity checks passed" in out.stdout
