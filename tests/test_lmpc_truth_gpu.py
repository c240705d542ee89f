"""The LMPC solve kernels against a certified truth of the reference QP (tests/qp_truth.py): every family of tests/golden/qp_truth_*.npz on
every form of the solve its controller admits, ragged batches, the forced ADMM fallback, warm starts from right, empty and wrong sets, a
heterogeneous bank and the single-instance front end.

Held on ALL instances -- those the oracle never polished included, which the oracle-based tests compare at 5e-2 --: cmd, cost and the three
sequences at qp_truth.kernel_tol(family) = max(8 x the float64 restatement's worst error, 1e-12) (measured on the CPU by
tests/test_qp_truth.py, never on a GPU), status 0 and is_feasible.  On the instances whose optimal working set is unique: the active bits on
the compared rows bit for bit, and active_count where no row at all is degenerate.  The truths come from the fixture files alone: no oracle
solve, no mpmath here.

Figures of the first GPU run are in DESIGN.md 2."""
import numpy as np
import pytest

import qp_truth as Q
import sens_ref as SF
from helpers import SHAPES_MAXIT

pytestmark = pytest.mark.gpu

# (name, debug_force_generic, debug_use_fused): the forms of test_lmpc_shapes_gpu.py
PATHS = [("default", False, None), ("two-kernel", False, 0), ("generic", True, None), ("fused", False, 1), ("group", False, 2)]
# forms a family's controller must admit (as test_lmpc_shapes_gpu.py asserts them): a set-up change that loses one fails here instead of skipping it
MUST_TAKE = {"classes": ("fused", "group"), "large": ("fused", "group"), "v2": ("group",)}
FAMILIES = tuple(f for f in Q.families() if f != "bank")


def _controller(sp, generic=False, fused=None, warm=False, rounds=None):
    from libmpc_amd import LMPC, LParameters
    from libmpc_amd._capi import check
    c = Q.configure(LMPC(*sp["dims"], device=0), sp)
    if warm:
        c.setOptimizerParameters(LParameters(maximum_iteration=SHAPES_MAXIT, enable_warm_start=1))
    c.debug_force_generic(generic)
    c.debug_use_fused(fused)
    if rounds is not None:
        check(c._lib.mpcx_lmpc_debug_set_rounds(c._h, rounds, 10))
    return c


def _can_take(c, pname):
    flags = c.debug_get("flags")
    return not ((pname == "fused" and int(flags[2]) != 1) or (pname == "group" and int(flags[1]) != 1))


def _solve(c, x0, u0, yref, **kw):
    import torch
    r = c.optimizeBatch(x0, u0, yref=yref, want_active=True, want_sequence=True, **kw)
    torch.cuda.synchronize()
    return r


def _bits(words, m):
    w = np.ascontiguousarray(words.cpu().numpy()).astype(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def _check(r, family, label, idx=None, keep=None):
    """a BatchResult against the fixture rows `idx` (default: all); prints and returns worst error / bound"""
    g = Q.load(family)
    idx = np.arange(len(g["cost"])) if idx is None else np.asarray(idx)
    tol = Q.kernel_tol(family)
    got = dict(cmd=r.cmd.cpu().numpy(), cost=r.cost.cpu().numpy(), input=r.seq_input.cpu().numpy(), state=r.seq_state.cpu().numpy(),
               output=r.seq_output.cpu().numpy())
    st = r.status.cpu().numpy(); feas = r.is_feasible.cpu().numpy(); ac = r.active_count.cpu().numpy()
    assert (st == 0).all(), (label, np.nonzero(st != 0)[0][:8], st[st != 0][:8])
    assert (feas != 0).all(), label
    err = np.zeros(len(idx)); cerr = np.zeros(len(idx))
    for i, b in enumerate(idx):
        err[i], cerr[i] = Q.errors({k: v[i] for k, v in got.items()},
                                   dict(cmd=g["cmd"][b], cost=g["cost"][b], input=g["seq_input"][b], state=g["seq_state"][b], output=g["seq_output"][b]))
    pol = g["polished"][idx]
    worst = max(err.max(), cerr.max())
    print("%s %s: worst error / bound %.2e / %.2e (sequences %.2e, cost %.2e; on the %d instances the oracle never polished %.2e), working sets %d .. %d"
          % (family, label, worst, tol, err.max(), cerr.max(), int((~pol).sum()), max(err[~pol].max(initial=0.0), cerr[~pol].max(initial=0.0)),
             ac.min(), ac.max()))
    assert np.isfinite(err).all() and np.isfinite(cerr).all(), label
    assert err.max() <= tol, (family, label, "sequences", float(err.max()), int(idx[np.argmax(err)]), tol)
    assert cerr.max() <= tol, (family, label, "cost", float(cerr.max()), int(idx[np.argmax(cerr)]), tol)
    # the working set, where it is unique
    m = int(g["ncon"])
    keep = np.ones(m, bool) if keep is None else keep
    lo, up = _bits(r.active_lower, m), _bits(r.active_upper, m)
    same = (lo[:, keep] == g["active_lower"][idx][:, keep]).all(axis=1) & (up[:, keep] == g["active_upper"][idx][:, keep]).all(axis=1)
    unique = ~g["degenerate"][idx]
    assert same[unique].all(), (family, label, "active bits", idx[np.nonzero(unique & ~same)[0]][:8])
    plain = ~g["degenerate_all"][idx]
    assert np.array_equal(ac[plain], g["n_active"][idx][plain]), (family, label, "active_count", idx[plain][np.nonzero(ac[plain] != g["n_active"][idx][plain])[0]][:8])
    return worst


# ---------------------------------------------------------------------------------------------
# 1. every family on every form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_every_family_on_every_form(family):
    w, x0, u0, yref = Q.inputs_of(family)
    sp = w["sp"]
    keep = Q.compared_rows(sp)
    taken = []
    for pname, generic, fused in PATHS:
        c = _controller(sp, generic, fused)
        assert c.info()["m_ref"] == int(Q.load(family)["ncon"])
        if not _can_take(c, pname):
            assert pname not in MUST_TAKE.get(family, ()), (family, pname, c.debug_get("flags"))
            continue
        taken.append(pname)
        _check(_solve(c, x0, u0, yref), family, pname, keep=keep)
    print("%s: forms taken %s" % (family, taken))
    assert {"default", "two-kernel", "generic"} <= set(taken)
    if family in ("v2", "v4", "ldg"):
        from helpers import SHAPES_VARIANTS
        c = _controller(sp)
        assert c.info()["kernel_variant"] == SHAPES_VARIANTS[family][1] and int(c.debug_get("flags")[0]) == SHAPES_VARIANTS[family][2]


# ---------------------------------------------------------------------------------------------
# 2. ragged batches: partial workgroups with instances of every bucket
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 17])
def test_ragged_batches_of_the_large_family(B):
    w, x0, u0, yref = Q.inputs_of("large")
    n = Q.load("large")["n_active"][:B]
    if B > 1:
        assert (n <= 16).any() and ((n > 16) & (n <= 28)).any() and (n > 28).any(), n
    for pname, generic, fused in PATHS:
        c = _controller(w["sp"], generic, fused)
        assert _can_take(c, pname)
        _check(_solve(c, x0[:B], u0[:B], yref[:B]), "large", "%s B=%d" % (pname, B), idx=np.arange(B))


# ---------------------------------------------------------------------------------------------
# 3. the ADMM -> guess -> re-polish path, forced by a round cap of 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["classes", "large"])
def test_forced_fallback_reaches_the_truth(family):
    w, x0, u0, yref = Q.inputs_of(family)
    c = _controller(w["sp"], fused=0, rounds=1)
    r = _solve(c, x0, u0, yref)
    it = r.iterations.cpu().numpy()
    print("%s: %d of %d instances took ADMM iterations (max %d)" % (family, int((it > 0).sum()), len(it), int(it.max())))
    assert (it > 0).mean() > 0.5, (it > 0).mean()
    _check(r, family, "forced fallback")


# ---------------------------------------------------------------------------------------------
# 4. warm starts: a wrong seed may cost rounds, never digits
# ---------------------------------------------------------------------------------------------
def _warm_seeds(g, words):
    own = (SF.pack_bits(g["active_lower"], words), SF.pack_bits(g["active_upper"], words))
    return {"the truth's sets": own, "empty sets": tuple(np.zeros_like(a) for a in own), "another instance's sets": tuple(np.roll(a, 1, axis=0) for a in own)}


@pytest.mark.parametrize("family", ["large", "full"])
def test_warm_starts_from_right_empty_and_wrong_sets(family):
    import torch
    w, x0, u0, yref = Q.inputs_of(family)
    g = Q.load(family)
    sp = w["sp"]
    c = _controller(sp, warm=True)
    seeds = _warm_seeds(g, c.info()["active_words"])
    rounds = {}
    for label, (wl, wu) in seeds.items():
        for shift in (False, True):
            warm = (torch.from_numpy(np.ascontiguousarray(wl)).cuda(), torch.from_numpy(np.ascontiguousarray(wu)).cuda())
            r = _solve(c, x0, u0, yref, warm=warm, warm_shift=shift)
            _check(r, family, "warm from %s, warm_shift=%s" % (label, shift), keep=Q.compared_rows(sp))
            rounds[(label, shift)] = int(r.polish_rounds.sum().item())
    print("%s: polish rounds in all %s" % (family, rounds))


def test_warm_starts_under_the_forced_fallback():
    """the same seeds with a round cap of 1: the lean kernel gives up after its one round and the fallback kernel reads the warm start itself,
    then writes the results.  Held as the cold forced fallback is, the share of instances that took ADMM iterations included: no seed is exempt from
    it.  With the truth's own sets and warm_shift off the lean kernel finishes in its one round the 23 instances whose optimum holds at most 16 rows;
    the other 41 of 64 reach the fallback (63 or 64 of 64 with the five other seeds)."""
    import torch
    w, x0, u0, yref = Q.inputs_of("large")
    c = _controller(w["sp"], fused=0, warm=True, rounds=1)
    for label, (wl, wu) in _warm_seeds(Q.load("large"), c.info()["active_words"]).items():
        for shift in (False, True):
            warm = (torch.from_numpy(np.ascontiguousarray(wl)).cuda(), torch.from_numpy(np.ascontiguousarray(wu)).cuda())
            r = _solve(c, x0, u0, yref, warm=warm, warm_shift=shift)
            it = r.iterations.cpu().numpy()
            print("large, warm from %s, warm_shift=%s: %d of %d instances took ADMM iterations (max %d)" % (label, shift, int((it > 0).sum()), len(it), int(it.max())))
            assert (it > 0).mean() > 0.5, (label, shift, (it > 0).mean())
            _check(r, "large", "forced fallback, warm from %s, warm_shift=%s" % (label, shift))


# ---------------------------------------------------------------------------------------------
# 5. a heterogeneous bank through lmpc_solve_hetero
# ---------------------------------------------------------------------------------------------
def test_bank_of_perturbed_controllers():
    import torch
    from libmpc_amd import LMPC
    from libmpc_amd.bank import LMPCHetero
    w, x0, u0, yref = Q.inputs_of("bank")
    g = Q.load("bank")
    assert np.array_equal(g["model"], w["model"]) and len(w["sps"]) == Q.BANK_MODELS and len(x0) == Q.BANK_BATCH
    het = LMPCHetero([Q.configure(LMPC(*s["dims"], device=-1), s) for s in w["sps"]], device=0)
    r = het.optimizeBatch(x0, u0, model=w["model"], want_active=True, want_sequence=True)
    torch.cuda.synchronize()
    _check(r, "bank", "lmpc_solve_hetero")


# ---------------------------------------------------------------------------------------------
# 6. the single-instance front end
# ---------------------------------------------------------------------------------------------
def test_optimize_and_get_optimal_sequence():
    from libmpc_amd import LMPC
    w, x0, u0, yref = Q.inputs_of("full")
    g = Q.load("full")
    sp = w["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    tol = Q.kernel_tol("full")
    c = Q.configure(LMPC(*sp["dims"], device=0), sp)
    picks = [int(np.argmax(g["n_active"])), int(np.argmin(g["n_active"])), 0, len(x0) - 1]
    for b in picks:
        assert c.setReferences(np.tile(yref[b][:, None], (1, ph)), sp["uref"], sp["duref"])
        res = c.optimize(x0[b], u0[b])
        seq = c.getOptimalSequence()
        assert res.status == 0 and res.is_feasible
        e, ce = Q.errors(dict(cmd=res.cmd, cost=res.cost, input=seq.input, state=seq.state, output=seq.output),
                         dict(cmd=g["cmd"][b], cost=g["cost"][b], input=g["seq_input"][b], state=g["seq_state"][b], output=g["seq_output"][b]))
        print("full optimize instance %d (%d rows): worst error / bound %.2e / %.2e" % (b, g["n_active"][b], max(e, ce), tol))
        assert e <= tol and ce <= tol, (b, e, ce)
