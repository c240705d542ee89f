"""The gradients of a bank's solved batch on weights, bounds and models (mpcx_lmpc_hetero_gradient_batch) on the device: every
family of tests/bank_grad_ref.py solved by the bank and differentiated in one launch, against the truth of each instance's own controller on the
active set the device ended with, against each member's own single-controller kernels, against a perturbed fleet; the per-controller sums, the
flags, the argument errors and lmpc_cmd_fleet.

Measured on an MI355X (this file's printed figures), worst error / max(1, max|truth|) of the parameter | the model outputs, bound 2.24e-11:
see DESIGN.md 4.10b for the table."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import bank_grad_ref as G
import model_sens_ref as Mo
import param_sens_ref as P

pytestmark = pytest.mark.gpu

NAMES = ("oweight", "uweight", "duweight", "lower", "upper", "A", "B", "C", "Bd", "Dd")
KEYS = G.PARAM + G.MODEL                                           # the truth's names, in that order


def controllers(name, specs=None, device=-1):
    from libmpc_amd import LMPC
    return [G.configure(LMPC(*sp["dims"], device=device), sp) for sp in (G.reference(name)["specs"] if specs is None else specs)]


@functools.lru_cache(maxsize=None)
def solved(name):
    """the family's bank on the device, its solve under the shuffled instance -> controller map, and the full gradient launch with the sums"""
    import torch
    from libmpc_amd import LMPCHetero
    R = G.reference(name)
    ctl = controllers(name)
    h = LMPCHetero(ctl, device=0)
    model = torch.as_tensor(R["model"].astype(np.int32)).cuda()
    r = h.optimizeBatch(R["x0"], R["u0"], model=model, yref=R["yref"], want_active=True, want_sequence=True)
    g = h.gradientBatch(r, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], per_controller=True)
    torch.cuda.synchronize()
    return h, ctl, model, r, g


def _np(g, prefix="d_"):
    return {n: (None if getattr(g, prefix + n, None) is None else getattr(g, prefix + n).cpu().numpy()) for n in NAMES}


def _copy(b):
    """a copy of a ctypes descriptor (copy.copy refuses structures that hold pointers)"""
    return type(b).from_buffer_copy(b)


def _row(o, b):
    return {k: o[n][b] for k, n in zip(KEYS, NAMES) if o[n] is not None}


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


@functools.lru_cache(maxsize=None)
def truths(name):
    """per instance the truth on the device's active set (None: left out), and how many of those sets are not the oracle's.  The sets are compared
    on the rows linear_ref.compared_rows names, as every test of the active words does: the others are rows of the reference QP the condensing has
    eliminated (equalities, the moves fixed past the control horizon) or doubles under move blocking, and keep the oracle's bits in the truth"""
    import linear_ref as LR
    R = G.reference(name)
    h, ctl, model, r, g = solved(name)
    m = R["active_lower"].shape[1]
    keep = LR.compared_rows(R["specs"][0])
    ol, ou = R["active_lower"] != 0, R["active_upper"] != 0
    lo, up = np.where(keep, _bits(r.active_lower, m) != 0, ol), np.where(keep, _bits(r.active_upper, m) != 0, ou)
    st = r.status.cpu().numpy()
    out, differ = [], 0
    for b in range(len(st)):
        t = R["truth"][b]
        if t is not None and st[b] == 0 and not (np.array_equal(lo[b], ol[b]) and np.array_equal(up[b], ou[b])):
            differ += 1
            t = R["truths"][R["model"][b]].gradients(R["x0"][b], R["u0"][b], R["yref"][b], lo[b], up[b], R["seed_cmd"][b], R["seed_input"][b])
        out.append(t if st[b] == 0 else None)
    return out, differ


@pytest.mark.parametrize("name", G.FAMILIES)
def test_gradients_match_the_truth(name):
    R = G.reference(name)
    h, ctl, model, r, g = solved(name)
    T, differ = truths(name)
    B = len(T)
    use = [b for b in range(B) if T[b] is not None]
    assert B - len(use) <= G.SKIP_CAP * B, (name, len(use), B)
    flags = g.flags.cpu().numpy()
    assert (flags[use] == 0).all()
    o = _np(g)
    arrs = [G.arrays(c) for c in ctl]
    ep = em = 0.0
    for b in use:
        p, m = G.compare(arrs[R["model"][b]], T[b], _row(o, b), blocked=name == "blocked")
        ep, em = max(ep, p), max(em, m)
    print(f"{name}: worst error of the parameter / the model outputs / bound {ep:.2e} / {em:.2e} / {G.BANK_GRAD_KERNEL_TOL:.2e}, "
          f"{len(use)} of {B} instances, {differ} on a set that is not the oracle's")
    assert max(ep, em) <= G.BANK_GRAD_KERNEL_TOL


@pytest.mark.parametrize("name", G.FAMILIES)
def test_the_bank_gives_what_each_controller_gives(name):
    """for every controller a device LMPC of the same spec differentiates the same optima on the same active words with the single-controller
    kernels (4.9, 4.10): both lie within their tolerance of one truth"""
    import torch
    R = G.reference(name)
    h, ctl, model, r, g = solved(name)
    T, _ = truths(name)
    o = _np(g)
    flags = g.flags.cpu().numpy()
    wp = wm = 0.0
    for k, c in enumerate(controllers(name, device=0)):
        idx = np.nonzero(R["model"] == k)[0]
        it = torch.as_tensor(idx).cuda()
        c.setup()
        own = c.optimizeBatch(R["x0"][idx], R["u0"][idx], yref=R["yref"][idx], want_active=True, want_sequence=True)
        for n in ("active_lower", "active_upper", "status", "seq_state", "seq_output", "seq_input"):       # the bank's optimum, word for word
            getattr(own, n).copy_(getattr(r, n)[it])
        gp = c.paramSensitivityBatch(own, seed_cmd=R["seed_cmd"][idx], seed_input=R["seed_input"][idx])
        gm = c.modelSensitivityBatch(own, seed_cmd=R["seed_cmd"][idx], seed_input=R["seed_input"][idx])
        torch.cuda.synchronize()
        assert np.array_equal(gp.flags.cpu().numpy(), flags[idx]) and np.array_equal(gm.flags.cpu().numpy(), flags[idx])
        op, om = _np(gp), _np(gm)
        for t, b in enumerate(idx):
            if T[b] is None:
                continue
            sp_ = max(1.0, max(np.abs(T[b][q]).max(initial=0.0) for q in G.PARAM))
            sm_ = max(1.0, max(np.abs(T[b][q]).max(initial=0.0) for q in G.MODEL if q in T[b]))
            wp = max(wp, max(np.abs(o[n][b] - op[n][t]).max(initial=0.0) for n in NAMES[:5]) / sp_)
            wm = max(wm, max(np.abs(o[n][b] - om[n][t]).max(initial=0.0) for n in NAMES[5:] if o[n] is not None) / sm_)
    print(f"{name}: bank against its members, parameters {wp:.2e} / {G.BANK_GRAD_KERNEL_TOL + P.KERNEL_TOL:.2e}, model {wm:.2e} / {G.BANK_GRAD_KERNEL_TOL + Mo.KERNEL_TOL:.2e}")
    assert wp <= G.BANK_GRAD_KERNEL_TOL + P.KERNEL_TOL and wm <= G.BANK_GRAD_KERNEL_TOL + Mo.KERNEL_TOL


@pytest.mark.parametrize("name", ["full", "ndu2", "blocked"])
def test_two_launches_give_the_same_bits_and_the_sums_follow_the_grouping(name):
    import torch
    from libmpc_amd import group_by_model
    R = G.reference(name)
    h, ctl, model, r, g = solved(name)
    g2 = h.gradientBatch(r, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], per_controller=True)
    torch.cuda.synchronize()
    assert torch.equal(g.flags, g2.flags) and torch.equal(g.n_used, g2.n_used)
    d1, d2, c1, c2 = _np(g), _np(g2), _np(g, "c_"), _np(g2, "c_")
    flags = g.flags.cpu().numpy()
    order, offsets = group_by_model(R["model"], h.count)
    for n in NAMES:
        if d1[n] is None:
            assert h.ndu == 0 and n in ("Bd", "Dd") and c1[n] is None
            continue
        assert d1[n].tobytes() == d2[n].tobytes() and c1[n].tobytes() == c2[n].tobytes(), n
        ref, used = G.group_sums(d1[n], flags, order, offsets)
        mass, _ = G.group_sums(np.abs(np.nan_to_num(d1[n])), flags, order, offsets)
        assert np.array_equal(g.n_used.cpu().numpy(), used)
        for k in range(h.count):
            assert (np.abs(c1[n][k] - ref[k]) <= max(used[k], 1) * 2.0 ** -52 * mass[k]).all(), (n, k)


def test_an_unsolved_instance_counts_nowhere():
    import torch
    R = G.reference("full")
    h, ctl, model, r, g = solved("full")
    b = 11
    k = int(R["model"][b])
    status = r.status.clone()
    desc = _copy(r._batch)                                      # the solved descriptor with a status of its own: instance b not solved
    status[b] = 2
    desc.status = C.c_void_p(status.data_ptr())
    g2 = h.gradientBatch(desc, model=model, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], per_controller=True)
    torch.cuda.synchronize()
    f1, f2 = g.flags.cpu().numpy(), g2.flags.cpu().numpy()
    assert f1[b] == 0 and f2[b] == 1 and np.array_equal(np.delete(f1, b), np.delete(f2, b))
    n1, n2 = g.n_used.cpu().numpy(), g2.n_used.cpu().numpy()
    assert n2[k] == n1[k] - 1 and np.array_equal(np.delete(n1, k), np.delete(n2, k))
    d1, d2, c1, c2 = _np(g), _np(g2), _np(g, "c_"), _np(g2, "c_")
    for n in NAMES:
        assert np.isnan(d2[n][b]).all() and np.delete(d1[n], b, axis=0).tobytes() == np.delete(d2[n], b, axis=0).tobytes(), n
        assert np.delete(c1[n], k, axis=0).tobytes() == np.delete(c2[n], k, axis=0).tobytes() and np.isfinite(c2[n]).all(), n
        assert (np.abs(c2[n][k] + d1[n][b] - c1[n][k]) <= 8 * 2.0 ** -52 * np.abs(np.nan_to_num(d1[n][R["model"] == k])).sum(axis=0)).all(), n


def test_without_a_map_instance_b_is_controller_b_and_subsets_keep_their_bits():
    import torch
    R = G.reference("nz16")
    h, ctl, model, r, g = solved("nz16")
    pick = np.array([int(np.nonzero(R["model"] == k)[0][0]) for k in range(h.count)])
    ident = torch.arange(h.count, dtype=torch.int32).cuda()
    sc, sq = R["seed_cmd"][pick], R["seed_input"][pick]
    r1 = h.optimizeBatch(R["x0"][pick], R["u0"][pick], yref=R["yref"][pick], want_active=True, want_sequence=True)
    g_none = h.gradientBatch(r1, seed_cmd=sc, seed_input=sq, per_controller=True)
    g_id = h.gradientBatch(r1, model=ident, seed_cmd=sc, seed_input=sq, per_controller=True)
    g_w = h.gradientBatch(r1, seed_cmd=sc, seed_input=sq, want=("oweight", "uweight", "duweight"))
    g_b = h.gradientBatch(r1, seed_cmd=sc, seed_input=sq, want=("lower", "upper"))
    g_m = h.gradientBatch(r1, seed_cmd=sc, seed_input=sq, want=("A", "B", "C"))
    torch.cuda.synchronize()
    assert (g_none.flags.cpu().numpy() == 0).all() and (g_none.n_used.cpu().numpy() == 1).all()
    a, b_, c = _np(g_none), _np(g_id), _np(g_none, "c_")
    for n in NAMES[:8]:
        assert a[n].tobytes() == b_[n].tobytes() and a[n].tobytes() == c[n].tobytes(), n      # one instance per controller: the sum is the row
        part = _np(g_w) if n in NAMES[:3] else (_np(g_b) if n in NAMES[3:5] else _np(g_m))
        assert part[n].tobytes() == a[n].tobytes(), n
    assert g_w.d_A is None and g_w.d_lower is None and g_m.d_oweight is None and g_b.d_C is None


@pytest.mark.parametrize("name", ["full", "soft"])
def test_a_perturbed_fleet_moves_cmd_as_the_gradients_say(name):
    """delta = 1e-4 times a random direction on the three weight matrices and on A, B, C of every controller, the bank rebuilt and solved:
    seed . cmd' against seed . cmd + <g, delta> within 1e-5 relative on the instances whose active set did not change and whose <g, delta> is
    1e-6 or more.  That bar is relative to seed . cmd', of order one, so the fleet is also solved at minus delta: in half the difference of the
    two solves the second-order term cancels, and it is held to <g, delta> within 1e-2 of its size plus 1e-9 -- the bars and the reasoning of
    tests/test_lmpc_param_sens_gpu.py and tests/test_lmpc_model_sens_gpu.py"""
    import torch
    from libmpc_amd import LMPCHetero
    R = G.reference(name)
    h, ctl, model, r, g = solved(name)
    seed = R["seed_cmd"]
    g1 = h.gradientBatch(r, seed_cmd=seed, want=("oweight", "uweight", "duweight", "A", "B", "C"))
    rg = np.random.default_rng(23)
    moved = ("OW", "UW", "DUW", "A", "B", "C")
    outs = ("oweight", "uweight", "duweight", "A", "B", "C")
    # (the weights move upwards: a weight stays non-negative)
    delta = [{q: 1e-4 * (rg.uniform(0.0, 1.0, size=sp[q].shape) if q in P.WEIGHTS else rg.normal(size=sp[q].shape)) for q in moved} for sp in R["specs"]]
    res = []
    for sign in (1.0, -1.0):
        specs = []
        for sp, dl in zip(R["specs"], delta):
            s2 = copy.deepcopy(sp)
            for q in moved:
                s2[q] = sp[q] + sign * dl[q]
            specs.append(s2)
        h2 = LMPCHetero(controllers(name, specs), device=0)
        res.append(h2.optimizeBatch(R["x0"], R["u0"], model=model, yref=R["yref"], want_active=True))
        torch.cuda.synchronize()
    r2, r3 = res
    same = lambda q: ((r.active_lower == q.active_lower).all(dim=1) & (r.active_upper == q.active_upper).all(dim=1) & (r.status == 0) & (q.status == 0)).cpu().numpy()
    same2, same3 = same(r2), same(r3)
    o = _np(g1)
    flags = g1.flags.cpu().numpy()
    cmd, cmd2, cmd3 = r.cmd.cpu().numpy(), r2.cmd.cpu().numpy(), r3.cmd.cpu().numpy()
    worst, worst_lin, checked, biting = 0.0, 0.0, 0, 0
    for b in range(len(cmd)):
        if not same2[b] or flags[b] != 0:
            continue
        dl = delta[R["model"][b]]
        lin = sum((o[n][b] * dl[q]).sum() for q, n in zip(moved, outs))
        if abs(lin) < 1e-6:
            continue
        checked += 1
        pred, act = seed[b] @ cmd[b] + lin, seed[b] @ cmd2[b]
        err = abs(pred - act) / max(abs(act), 1e-12)
        worst = max(worst, err)
        assert err <= 1e-5, (name, b, pred, act, lin)
        if same3[b]:
            half = 0.5 * (seed[b] @ cmd2[b] - seed[b] @ cmd3[b])
            worst_lin = max(worst_lin, abs(half - lin) / abs(lin))
            biting += 1
            assert abs(half - lin) <= 1e-2 * abs(lin) + 1e-9, (name, b, half, lin)
    print(f"{name}: seed . cmd' against the prediction {worst:.2e} relative on {checked} instances; half the difference of two solves against <g, delta> "
          f"{worst_lin:.2e} of its size on {biting}")
    assert checked >= 8 and biting >= 8


def test_argument_errors():
    import torch
    from libmpc_amd import _capi
    R = G.reference("nz16")
    h, ctl, model, r, g = solved("nz16")
    lib = _capi.lib()
    f = lib.mpcx_lmpc_hetero_gradient_batch
    B = len(R["model"])
    seed = torch.ones((B, h.nu), dtype=torch.float64, device="cuda")
    out = torch.full((B * h.nx * h.nx + h.count * h.nx * h.nx,), -7.0, dtype=torch.float64, device="cuda")
    mi = C.c_void_p(model.data_ptr())

    def desc(**kw):
        d = _capi.BankGrad()
        d.solved = C.cast(C.pointer(r._batch), C.c_void_p)
        d.seed_cmd = seed.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert f(h._h, None, mi, None) == _capi.E_INVALID
    assert f(h._h, C.byref(desc(seed_cmd=None)), mi, None) == _capi.E_INVALID and "seed" in lib.mpcx_last_error().decode()
    assert f(h._h, C.byref(desc(solved=None)), mi, None) == _capi.E_INVALID
    assert f(h._h, C.byref(desc(d_A=out.data_ptr())), None, None) == _capi.E_INVALID and "model index" in lib.mpcx_last_error().decode()
    assert f(h._h, C.byref(desc(c_A=out.data_ptr())), mi, None) == _capi.E_INVALID and "per-instance output" in lib.mpcx_last_error().decode()
    assert f(h._h, C.byref(desc(d_A=out.data_ptr(), c_A=out.data_ptr() + 8 * B * h.nx * h.nx)), mi, None) == _capi.E_INVALID and "group_order" in lib.mpcx_last_error().decode()
    for member in ("x0", "u0", "active_lower", "active_upper", "seq_output", "seq_input", "seq_state"):
        b2 = _copy(r._batch)
        setattr(b2, member, None)
        d = desc(d_A=out.data_ptr())
        d.solved = C.cast(C.pointer(b2), C.c_void_p)
        assert f(h._h, C.byref(d), mi, None) == _capi.E_INVALID, member
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                      # a refused call writes nothing
    # without a model output the sequence of states may be missing
    b2 = _copy(r._batch)
    b2.seq_state = None
    g2 = h.gradientBatch(b2, model=model, seed_cmd=R["seed_cmd"], seed_input=R["seed_input"], want=("oweight", "lower"))
    torch.cuda.synchronize()
    assert torch.equal(g2.d_oweight, g.d_oweight) and torch.equal(g2.d_lower, g.d_lower)


def test_autograd_of_a_fleet_gives_the_per_controller_sums():
    import torch
    from libmpc_amd import lmpc_cmd_fleet
    R = G.reference("ndu2")
    specs = R["specs"]
    ctl = controllers("ndu2")
    dev = torch.device("cuda", 0)
    stack = lambda q: torch.tensor(np.stack([sp[q] for sp in specs]), dtype=torch.float64, device=dev, requires_grad=True)
    P_ = {q: stack(q) for q in ("OW", "UW", "DUW", "A", "B", "C", "Bd", "Dd")}
    x0 = torch.tensor(R["x0"], device=dev, requires_grad=True)
    u0, yref = torch.tensor(R["u0"], device=dev), torch.tensor(R["yref"], device=dev)
    model = torch.as_tensor(R["model"].astype(np.int32)).cuda()
    w = torch.tensor(R["seed_cmd"], device=dev)
    cmd, status = lmpc_cmd_fleet(ctl, x0, u0, yref, model, P_["OW"], P_["UW"], P_["DUW"], P_["A"], P_["B"], P_["C"], P_["Bd"], P_["Dd"], return_status=True)
    node = cmd.grad_fn
    (cmd * w).sum().backward()
    torch.cuda.synchronize()
    bank, res = node.bank, node.res
    ref = bank.gradientBatch(res, seed_cmd=w, per_controller=True)
    vjp = bank.sensitivityBatch(res.active_lower, res.active_upper, model=model, status=res.status, seed_cmd=w, want=("x0",))
    torch.cuda.synchronize()
    assert (status == 0).all() and torch.equal(x0.grad, vjp.d_x0)
    for q, n in zip(("OW", "UW", "DUW", "A", "B", "C", "Bd", "Dd"), ("oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")):
        assert torch.equal(P_[q].grad, getattr(ref, "c_" + n)), q
    # the same fleet as the shuffled family solved directly: the same optimum, the same rows
    h, _, _, r, g = solved("ndu2")
    assert torch.equal(res.cmd, r.cmd)
    # a loss on the weights alone never asks for the model part
    ow, uw, dw = (P_[q].detach().clone().requires_grad_(True) for q in ("OW", "UW", "DUW"))
    cmd2 = lmpc_cmd_fleet(ctl, x0.detach(), u0, yref, model, ow, uw, dw)
    node2 = cmd2.grad_fn
    (cmd2 * w).sum().backward()
    torch.cuda.synchronize()
    assert node2.gradient.d_A is None and node2.gradient.c_C is None and node2.gradient.d_lower is None
    for t, n in ((ow, "oweight"), (uw, "uweight"), (dw, "duweight")):
        assert torch.equal(t.grad, getattr(ref, "c_" + n)), n
