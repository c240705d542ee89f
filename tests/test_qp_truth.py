"""The truth the solve kernels are held to (tests/qp_truth.py, tests/golden/qp_truth_*.npz), checked on the CPU: a sample of every fixture is
certified again from nothing (no oracle seed), the populations the GPU tests rely on are there, the degenerate share is under its cap, the
oracle's polished points agree with the truth, and the bound of the GPU tests -- the float64 restatement of the kernels' formula against the
truth -- is measured and pinned.  No GPU; the product enters only as a host-only handle whose set-up arrays the restatement reads."""
import os

import numpy as np
import pytest

import qp_truth as Q
import sens_ref as SF

SAMPLE = 4


def _builders(w):
    return [SF.builder(s) for s in w["sps"]] if "sps" in w else [SF.builder(w["sp"])]


def _specs(w):
    return w["sps"] if "sps" in w else [w["sp"]]


def _sample(g):
    """SAMPLE instances: the largest working set, a degenerate one and one the oracle did not polish where there are any, then the first ones"""
    order = [int(np.argmax(g["n_active"]))] + [int(b) for b in np.nonzero(g["degenerate_all"])[0][:1]] + [int(b) for b in np.nonzero(~g["polished"])[0][:1]]
    order += list(range(len(g["cost"])))
    out = []
    for b in order:
        if b not in out:
            out.append(b)
    return out[:SAMPLE]


def test_fixture_files_are_there_and_small():
    for file in Q.FILES:
        assert os.path.getsize(Q.path(file)) <= Q.MAX_FIXTURE_BYTES, file
    assert {f for members in Q.FILES.values() for f, _, _ in members} == set(Q.families())
    assert "v1_zero_weight" not in Q.families()


@pytest.mark.parametrize("name", Q.families())
def test_family(name):
    w, x0, u0, yref = Q.inputs_of(name)
    g = Q.load(name)
    B = len(g["cost"])
    assert np.array_equal(g["x0"], x0) and np.array_equal(g["u0"], u0) and np.array_equal(g["yref"], yref)       # the fixture is the workload
    specs, builders = _specs(w), _builders(w)
    nx, nu, ndu, ny, ph, ch = specs[0]["dims"]
    assert int(g["ncon"]) == builders[0].d.ncon and g["active_lower"].shape == (B, builders[0].d.ncon)
    assert np.isfinite(g["cmd"]).all() and np.isfinite(g["cost"]).all()                                               # every instance certified
    assert np.array_equal(g["n_active"], (g["active_lower"] | g["active_upper"]).sum(axis=1))
    assert not g["active_lower"][:, :int(g["neq"])].any() and not g["active_upper"][:, :int(g["neq"])].any()
    assert np.array_equal(g["cmd"], g["seq_input"][:, 0])

    # ---- a sample certified again from nothing: same point to the last bit or two, same sets wherever they are unique
    for b in _sample(g):
        k = int(g["model"][b])
        t = Q.truth_of(builders[k], specs[k], x0[b], u0[b], yref[b])
        assert t is not None and t["residual"] <= Q.RES_TOL, (name, b)
        scale = max(1.0, np.abs(g["cmd"][b]).max())
        assert np.abs(t["cmd"] - g["cmd"][b]).max() <= 1e-15 * scale, (name, b)
        assert abs(t["cost"] - g["cost"][b]) <= 1e-15 * max(1.0, abs(g["cost"][b])), (name, b)
        for key in ("input", "state", "output"):
            assert np.abs(t[key] - g["seq_" + key][b]).max() <= 1e-15 * max(1.0, np.abs(g["seq_" + key][b]).max()), (name, b, key)
        assert t["degenerate"] == g["degenerate"][b] and t["degenerate_all"] == g["degenerate_all"][b], (name, b)
        if not g["degenerate_all"][b]:
            assert np.array_equal(t["active_lower"], g["active_lower"][b]) and np.array_equal(t["active_upper"], g["active_upper"][b]), (name, b)
            assert t["margin"] >= Q.MARGIN_MIN and np.isclose(t["margin"], g["margin"][b], rtol=1e-6)
        elif not g["degenerate"][b]:
            keep = Q.compared_rows(specs[k])
            assert np.array_equal(t["active_lower"][keep], g["active_lower"][b][keep]), (name, b)
            assert np.array_equal(t["active_upper"][keep], g["active_upper"][b][keep]), (name, b)

    # ---- the populations the GPU tests rely on
    n = g["n_active"]
    if name == "classes":
        from test_lmpc_round_classes import ROUND_CLASSES
        counts = [int(((n >= lo) & (n <= hi)).sum()) for lo, hi in ROUND_CLASSES]
        assert min(counts) >= 3 and (n > 16).sum() >= 8 and B <= 64, (counts, B)
        assert ((n >= 15) & (n <= 16)).any() and (n > 16).any()                              # both sides of the lean kernels' hand-over
    if name in ("large", "bank"):
        buckets = (int((n <= 16).sum()), int(((n > 16) & (n <= 28)).sum()), int((n > 28).sum()))
        assert min(buckets) >= (8 if name == "large" else 4) and B == (64 if name == "large" else 32), buckets
    if name in ("v2", "v4", "ldg") or name in Q.edge_families():
        assert B >= 8
    if name == "smallest":
        assert (n == 0).all()
    if name in ("full", "soft", "linear", "terminal"):
        assert (n > 16).any() and (n <= 16).any()
    if name == "blocked":
        assert g["dependent"].any()                 # linearly dependent working rows are part of the family: cmd, cost and sequences are held there too

    # ---- degenerate instances: decided from the truth alone, at most SKIP_CAP of the family
    assert g["degenerate"].mean() <= Q.SKIP_CAP, (name, g["degenerate"].mean())
    assert np.array_equal(g["degenerate"] | g["dependent"] | (g["margin"] < Q.MARGIN_MIN), g["degenerate_all"])
    if ch >= ph - 1:
        assert np.array_equal(g["degenerate"], g["degenerate_all"])

    # ---- the oracle where it polished: its point is the truth's
    pol = g["polished"]
    oerr = np.abs(g["oracle_cmd"] - g["cmd"]).max(axis=1) / np.maximum(1.0, np.abs(g["cmd"]).max(axis=1))
    worst_oracle = float(oerr[pol].max(initial=0.0))
    assert worst_oracle <= max(8.0 * Q.ORACLE_WORST[name], 1e-12), (name, worst_oracle)
    if name in ("classes", "ch_lt_ph"):
        o = Q.oracle_solve(name)                      # the whole draw: if it holds unpolished instances, so does the fixture
        assert np.array_equal(o["polished"][g["pick"]] == 1, pol) and np.array_equal(o["cmd"][g["pick"]], g["oracle_cmd"])
        assert (~pol).any() or (o["polished"] == 1).all()
    if name in ("classes", "large", "soft", "blocked", "ch_lt_ph"):
        assert (~pol).any(), name                     # the instances today's suite compares at 5e-2

    # ---- the bound: the kernels' formula in float64 against the truth
    from libmpc_amd import LMPC
    arrays = [Q.arrays(Q.configure(LMPC(*s["dims"], device=-1), s), s) for s in specs]
    worst, worst_cost = 0.0, 0.0
    for b in range(B):
        k = int(g["model"][b])
        r = Q.restate_condensed(arrays[k], x0[b], u0[b], yref[b], None, (g["active_lower"][b], g["active_upper"][b]))
        e, ce = Q.errors(r, dict(cmd=g["cmd"][b], cost=g["cost"][b], input=g["seq_input"][b], state=g["seq_state"][b], output=g["seq_output"][b]))
        worst, worst_cost = max(worst, e), max(worst_cost, ce)
    measured = max(worst, worst_cost)
    print("%-9s %2d instances, working sets %d .. %d, degenerate %.1f %% (any row %.1f %%), oracle polished %d: agreement %.2e; restatement worst %.2e (cost %.2e) "
          "-> kernel bound %.2e" % (name, B, n.min(), n.max(), 100 * g["degenerate"].mean(), 100 * g["degenerate_all"].mean(), pol.sum(), worst_oracle,
                                    worst, worst_cost, Q.kernel_tol(name)))
    assert measured <= Q.RESTATEMENT_WORST[name] <= 2.0 * measured, (name, measured, Q.RESTATEMENT_WORST[name])
    assert Q.RESTATEMENT_WORST[name] <= 1e-9          # (a family past this would be reported with its condition numbers in DESIGN.md 2 and keep its own bound)


def test_soft_family_the_one_point_that_differs_is_one_the_oracle_did_not_polish():
    """on the soft family every point the oracle polished is the certified optimum to 4.4e-11; the one that is off (5.3e-4 of |cmd|,
    4.5e-5 of max(1, |cmd|)) is the instance whose polish failed -- flag -1, which counts as "polished" only for a reader who tests the flag's
    truth value instead of == 1, as every test of the suite does"""
    g = Q.load("soft")
    oerr = np.abs(g["oracle_cmd"] - g["cmd"]).max(axis=1) / np.maximum(1.0, np.abs(g["cmd"]).max(axis=1))
    off = np.nonzero(oerr > 1e-9)[0]
    assert len(off) == 1 and not g["polished"][off[0]] and 1e-6 < oerr[off[0]] < 1e-3
    w, x0, u0, yref = Q.inputs_of("soft")
    b = int(off[0])
    pb = SF.builder(w["sp"])
    o = SF.solve_one(pb, w["sp"], x0[b], u0[b], yref[b])
    assert o["polished"] == -1 and o["polished_raw"] == -1 and bool(o["polished"])
    assert np.array_equal(o["cmd"], g["oracle_cmd"][b])
    assert o["cost"] - g["cost"][b] > 1e-4            # an ADMM iterate, 1.7e-3 above the optimum's cost: no KKT point
    assert 4e-4 < np.abs(o["cmd"] - g["cmd"][b]).max() / np.abs(g["cmd"][b]).max() < 6e-4          # the 5e-4 of the first comparison, relative to |cmd|


def test_regenerating_reproduces_the_committed_arrays():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_qp_golden", os.path.join(Q.GOLDEN, "make_qp_golden.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    for fam in ("nu1", "blocked"):
        again = mod.solve_family(fam)
        g = Q.load(fam)
        m = int(g["ncon"])
        for k, v in again.items():
            if k in ("active_lower", "active_upper"):
                v = np.unpackbits(v, axis=1, bitorder="little")[:, :m]
            assert np.array_equal(np.asarray(v), g[k]), (fam, k)
