"""Writes tests/golden/qp_truth_<file>.npz: the certified optima (tests/qp_truth.py) of every workload of tests/test_lmpc_truth_gpu.py.

CPU only, deterministic: the oracle supplies the first working set of each instance and nothing else; every stored figure is the mpmath
point rounded to float64.  Run from the repository root:  python tests/golden/make_qp_golden.py [file ...]   (about two minutes for all)

Per family <f>, arrays <f>__<key>: the inputs x0, u0, yref [B, ny], dmeas [ndu, ph] (the controller's); the truths cmd, cost, seq_input,
seq_state, seq_output; active_lower / active_upper as bits packed little-endian in the reference's row numbering; n_active, margin,
margin_compared, dependent, degenerate (bits not unique on the compared rows), degenerate_all (on any row); polished and oracle_cmd (the
oracle's flag and command); pick (index into the workload's batch); model (the bank's controller per instance); ncon, neq."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import qp_truth as Q          # noqa: E402
import sens_ref as SF         # noqa: E402


def pick_classes(n_active, polished):
    """CLASSES_PER_CLASS of each size class of the round and CLASSES_PAST_16 beyond the lean kernels' 16 rows: those the oracle did not polish,
    then the first of each in batch order"""
    from test_lmpc_round_classes import ROUND_CLASSES
    order = np.argsort(polished == 1, kind="stable")
    n = n_active[order]
    pick = []
    for lo, hi in ROUND_CLASSES:
        pick += list(order[(n >= lo) & (n <= hi)][:Q.CLASSES_PER_CLASS])
    pick += list(order[n > 16][:Q.CLASSES_PAST_16])
    return np.array(sorted(pick), int)


def solve_family(name):
    w = Q.workload(name)
    o = Q.oracle_solve(name)
    B = len(w["x0"])
    builders = [SF.builder(s) for s in w["sps"]] if name == "bank" else [SF.builder(w["sp"])]
    model = w["model"] if name == "bank" else np.zeros(B, int)
    specs = w["sps"] if name == "bank" else [w["sp"]]
    truths = []
    for b in range(B):
        t = Q.truth_of(builders[model[b]], specs[model[b]], w["x0"][b], w["u0"][b], w["yref"][b], o["active_lower"][b], o["active_upper"][b])
        assert t is not None, (name, b)
        truths.append(t)
    pick = np.arange(B)
    if name == "classes":
        pick = pick_classes(np.array([t["n_active"] for t in truths]), o["polished"])
    if name == "ch_lt_ph":
        deg = np.array([t["degenerate"] or t["degenerate_all"] for t in truths])
        unpol = o["polished"] != 1                     # instances the oracle did not polish first, so that the fixture holds some
        order = np.argsort(~unpol, kind="stable")
        pick = np.sort(np.concatenate([order[~deg[order]][:Q.BLOCKED_PLAIN], order[deg[order]][:Q.BLOCKED_DEGENERATE]]))
    nx, nu, ndu, ny, ph, ch = w["sp"]["dims"]
    d = builders[0].d
    out = dict(x0=w["x0"][pick], u0=w["u0"][pick], yref=w["yref"][pick], dmeas=w["sp"].get("dmeas", np.zeros((ndu, ph))),
               ncon=np.int64(d.ncon), neq=np.int64(d.neq), pick=pick, model=model[pick],
               polished=(o["polished"][pick] == 1), oracle_cmd=o["cmd"][pick])
    T = [truths[b] for b in pick]
    out["cmd"] = np.stack([t["cmd"] for t in T]); out["cost"] = np.array([t["cost"] for t in T])
    for k in ("input", "state", "output"):
        out["seq_" + k] = np.stack([t[k] for t in T])
    for k in ("active_lower", "active_upper"):
        out[k] = np.packbits(np.stack([t[k] for t in T]), axis=1, bitorder="little")
    out["n_active"] = np.array([t["n_active"] for t in T], np.int32)
    for k in ("margin", "margin_compared"):
        out[k] = np.array([t[k] for t in T])
    for k in ("dependent", "degenerate", "degenerate_all"):
        out[k] = np.array([t[k] for t in T], bool)
    return out


def main(files):
    solved = {}
    for file in files:
        arrays = {}
        for fam, first, last in Q.FILES[file]:
            if fam not in solved:
                solved[fam] = solve_family(fam)
            for k, v in solved[fam].items():
                arrays[fam + "__" + k] = v[first:last] if k in Q.PER_INSTANCE else v
            s = solved[fam]
            print("%-10s %3d instances, working sets %d .. %d, oracle polished %d, degenerate %d (any row %d)" % (
                fam, len(s["cost"]), s["n_active"].min(), s["n_active"].max(), s["polished"].sum(), s["degenerate"].sum(), s["degenerate_all"].sum()))
        np.savez_compressed(Q.path(file), **arrays)
        size = os.path.getsize(Q.path(file))
        print("%s: %d bytes" % (os.path.basename(Q.path(file)), size))
        assert size <= Q.MAX_FIXTURE_BYTES, (file, size)


if __name__ == "__main__":
    main(sys.argv[1:] or list(Q.FILES))
