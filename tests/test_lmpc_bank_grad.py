"""The gradients of a bank's solved batch on weights, bounds and models, CPU part: the numpy restatement of the kernel's
formulas (tests/bank_grad_ref.rollout_gradients, no Cq / Xq) against the truth of each instance's own controller -- the test that measures
BANK_GRAD_RESTATEMENT_WORST --, against the single-controller restatements where the controllers are equal, the per-controller sums, the
front-end's argument checks and the ABI."""
import ctypes as C
import functools

import numpy as np
import pytest

import bank_grad_ref as G
import model_sens_ref as Mo
import param_sens_ref as P
import sens_ref as S
from libmpc_amd.bank import group_by_model


@functools.lru_cache(maxsize=None)
def hosts(name):
    from libmpc_amd import LMPC
    return [G.configure(LMPC(*sp["dims"], device=-1), sp) for sp in G.reference(name)["specs"]]


@pytest.mark.parametrize("name", G.FAMILIES)
def test_restatement_matches_the_truth(name):
    """measures the constant: the figures of bank_grad_ref's head are this test's printed ones"""
    R = G.reference(name)
    ctl = hosts(name)
    B = len(R["model"])
    oracle, use = G.usable_counts(R)
    print(f"{name}: usable by the oracle alone {oracle} of {B}, with both truths {use}")
    assert B - oracle <= G.SKIP_CAP * B and B - use <= G.SKIP_CAP * B
    assert (oracle, use) == G.USABLE[name]
    wp = wm = 0.0
    for b in range(B):
        if R["truth"][b] is None:
            continue
        g = G.restatement(R, ctl, b)
        assert not g["dependent"]
        ep, em = G.compare(G.arrays(ctl[R["model"][b]]), R["truth"][b], g, blocked=name == "blocked")
        wp, wm = max(wp, ep), max(wm, em)
    print(f"{name}: worst error of the restatement, parameters {wp:.2e}, model {wm:.2e} (committed {G.BANK_GRAD_RESTATEMENT_WORST:.2e})")
    assert max(wp, wm) <= G.BANK_GRAD_RESTATEMENT_WORST


def test_tolerance_is_the_restatements():
    assert G.BANK_GRAD_KERNEL_TOL == max(8.0 * G.BANK_GRAD_RESTATEMENT_WORST, 1e-12) and G.SKIP_CAP == S.SKIP_CAP == 0.10
    assert set(G.FAMILIES) == set(G.SEEDS) == set(G.USABLE) and len(G.FAMILIES) == 15


@pytest.mark.parametrize("name", ["full", "soft", "blocked", "refs", "ndu2"])
def test_equal_controllers_give_the_single_controller_formulas(name):
    """a bank whose K controllers are equal, instance b on controller b: the roll-out form equals the forms with the host-built Cq and Xq"""
    from libmpc_amd import LMPC
    R = Mo.reference(name)
    sp, res = R["sp"], R["res"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    K = 4
    ctl = [S.configure(LMPC(*sp["dims"], device=-1), sp) for _ in range(K)]
    uref, duref, dmeas = G.own_references(sp)
    tol = P.KERNEL_TOL + Mo.KERNEL_TOL
    for b in range(K):
        X, Yo = Mo.rollout(sp, R["x0"][b], res["input"][b])
        yref = np.tile(R["yref"][b][:, None], (1, ph))
        args = (res["active_lower"][b], res["active_upper"][b], R["u0"][b])
        g = G.rollout_gradients(G.arrays(ctl[b]), *args, X, Yo, res["input"][b], yref, uref, duref, dmeas, R["seed_cmd"][b], R["seed_input"][b])
        gp = P.condensed_gradients(P.arrays(ctl[b]), *args, Yo, res["input"][b], yref, uref, duref, R["seed_cmd"][b], R["seed_input"][b])
        gm = Mo.condensed_gradients(Mo.arrays(ctl[b]), *args, X, Yo, res["input"][b], yref, uref, duref, dmeas, R["seed_cmd"][b], R["seed_input"][b])
        assert g["n"] == gp["n"] == gm["n"] and not g["dependent"]
        for ref, keys in ((gp, G.PARAM), (gm, G.MODEL)):
            scale = max(1.0, max(np.abs(ref[k]).max(initial=0.0) for k in keys))
            assert max(np.abs(g[k] - ref[k]).max(initial=0.0) for k in keys) <= tol * scale, (b, keys)


def test_per_controller_sums_follow_the_grouping():
    R = G.reference("nz16")
    ctl = hosts("nz16")
    B, K = len(R["model"]), len(ctl)
    rows = {k: [] for k in G.PARAM + ("A", "B", "C")}
    for b in range(B):
        g = G.restatement(R, ctl, b)
        for k in rows:
            rows[k].append(g[k])
    flags = np.zeros(B, int)
    flags[[3, 17]] = (1, 2)                                        # two instances that do not count
    order, offsets = group_by_model(R["model"], K)
    assert sorted(order) == list(range(B)) and all((np.diff(order[offsets[k]:offsets[k + 1]]) > 0).all() for k in range(K))
    for k, v in rows.items():
        v = np.stack(v)
        sums, used = G.group_sums(v, flags, order, offsets)
        for c in range(K):
            mine = [b for b in range(B) if R["model"][b] == c and flags[b] == 0]         # ascending: the stable grouping's order
            ref = np.zeros(v.shape[1:])
            for b in mine:
                ref = ref + v[b]
            assert used[c] == len(mine) and sums[c].tobytes() == ref.tobytes(), (k, c)
    assert used.sum() == B - 2


def test_a_parallel_pair_is_reported_dependent():
    R = G.reference("full")
    a = G.arrays(hosts("full")[0])
    d = R["truths"][0].param.pb.d
    al = np.zeros(R["active_lower"].shape[1], bool); au = al.copy()
    al[d.neq + d.na + a["nx"]] = True; au[d.neq + d.off_du] = True            # box row and step-0 rate row of input 0
    b = int(np.nonzero(R["model"] == 0)[0][0])
    sp = R["specs"][0]
    g = G.rollout_gradients(a, al, au, R["u0"][b], R["seq_state"][b], R["seq_output"][b], R["input"][b], np.tile(R["yref"][b][:, None], (1, sp["dims"][4])),
                            *G.own_references(sp), R["seed_cmd"][b])
    assert g["dependent"] and g["n"] == 2 and all(np.isnan(g[k]).all() for k in G.PARAM + G.MODEL)


def test_abi_symbols_and_descriptor_size():
    import os
    from libmpc_amd import _capi
    lib = _capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mpcx.h")).read()
    for n in ("mpcx_lmpc_hetero_gradient_batch", "mpcx_lmpc_bank_grad_size"):
        assert n in _capi.EXPORTS and getattr(lib, n) is not None and n + "(" in header
    assert "Banks have no such call" not in header
    assert C.sizeof(_capi.BankGrad) == lib.mpcx_lmpc_bank_grad_size() == 27 * C.sizeof(C.c_void_p)
    names = [f[0] for f in _capi.BankGrad._fields_]
    assert names[:3] == ["solved", "seed_cmd", "seed_input"] and names[3:13] == ["d_" + n for n in ("oweight", "uweight", "duweight", "lower", "upper", "A", "B", "C", "Bd", "Dd")]
    assert names[13:16] == ["flags", "group_order", "group_offsets"] and names[16:26] == ["c" + n[1:] for n in names[3:13]] and names[26] == "n_used"
    f = lib.mpcx_lmpc_hetero_gradient_batch
    d = _capi.BankGrad()
    assert f(None, C.byref(d), None, None) == _capi.E_INVALID and "null bank" in lib.mpcx_last_error().decode()


def _bare_bank():
    """an object that has only the dimensions: the argument checks come before any device call"""
    from libmpc_amd import LMPCHetero
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h, het.count, het.active_words, het.m_ref = 3, 2, 2, 0, 6, -1, None, 4, 2, 40
    return het


def _solved_descriptor(B=4, state=True):
    from libmpc_amd import _capi
    b = _capi.Batch()
    b.batch = B
    for n in ("x0", "u0", "active_lower", "active_upper", "seq_output", "seq_input") + (("seq_state",) if state else ()):
        setattr(b, n, 8)                                            # (never dereferenced: the checks only ask whether it is there)
    return b


def test_front_end_argument_checks():
    import libmpc_amd
    from libmpc_amd import MpcxError, _capi
    het = _bare_bank()
    seed = np.zeros((4, 2))
    with pytest.raises(ValueError, match="result of optimizeBatch"):
        het.make_gradient(object(), seed_cmd=seed)
    with pytest.raises(ValueError, match="seed_cmd or seed_input"):
        het.make_gradient(_solved_descriptor())
    with pytest.raises(ValueError, match="want"):
        het.make_gradient(_solved_descriptor(), seed_cmd=seed, want=("oweight", "Q"))
    with pytest.raises(ValueError, match="want_sequence"):
        het.make_gradient(_solved_descriptor(state=False), seed_cmd=seed)             # a model output without the states
    b = _solved_descriptor()
    b.active_upper = None
    with pytest.raises(ValueError, match="want_active"):
        het.make_gradient(b, seed_cmd=seed, want=("oweight",))
    with pytest.raises(ValueError, match="batch must be the bank"):
        het.make_gradient(_solved_descriptor(B=5), seed_cmd=np.zeros((5, 2)))
    # everything in order: the first device call refuses, as every front-end does without a device; the states may be missing for the weights alone
    for call in (lambda: het.make_gradient(_solved_descriptor(), seed_cmd=seed),
                 lambda: het.gradientBatch(_solved_descriptor(state=False), seed_cmd=seed, want=("oweight", "lower"), per_controller=True)):
        with pytest.raises(MpcxError) as e:
            call()
        assert e.value.code == _capi.E_DEVICE
    # lmpc_cmd_fleet: the parameter tensors come in their groups, K in front
    from libmpc_amd import LMPC
    ctl = [LMPC(3, 2, 0, 2, 6, 6, device=-1) for _ in range(2)]
    x0, u0 = np.zeros((2, 3)), np.zeros((2, 2))
    with pytest.raises(ValueError, match="at least one controller"):
        libmpc_amd.lmpc_cmd_fleet([], x0, u0, None)
    with pytest.raises(ValueError, match="OWeight, UWeight and DeltaUWeight go together"):
        libmpc_amd.lmpc_cmd_fleet(ctl, x0, u0, None, OWeight=np.ones((2, 2, 6)))
    with pytest.raises(ValueError, match="A, B and C go together"):
        libmpc_amd.lmpc_cmd_fleet(ctl, x0, u0, None, A=np.ones((2, 3, 3)), B=np.ones((2, 3, 2)))
    with pytest.raises(ValueError, match="Bd and Dd go together"):
        libmpc_amd.lmpc_cmd_fleet(ctl, x0, u0, None, Bd=np.ones((2, 3, 1)))
    with pytest.raises(ValueError, match=r"\[K, rows, columns\]"):
        libmpc_amd.lmpc_cmd_fleet(ctl, x0, u0, None, A=np.ones((3, 3, 3)), B=np.ones((3, 3, 2)), C=np.ones((3, 2, 3)))
