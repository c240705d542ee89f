"""Writes tests/golden/soft_oracle.npz: the slack-augmented reference QP (tests/soft_ref.py) solved for the cases of
tests/test_lmpc_soft_gpu.py whose yardstick solves take seconds each, inputs and recorded results under a prefix per case:

    large_   the double integrator with ph = 40, ch = 2 (three decision variables) and 41 soft velocity rows, soft_ref.large_case()
    full0_   soft_ref.full_feature_soft() on rate_ref.full_feature_batch(24)
    full1_   the same controller one tick later, from the recorded commands of full0_ (the warm-start test's second tick)

A CPU test solves the first instance of large_ again and compares (tests/test_lmpc_soft.py).

    python tests/golden/make_soft_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import rate_ref as RR  # noqa: E402
import soft_ref as SR  # noqa: E402

KEEP = ("cmd", "cost", "status", "solver_status", "polished", "iters", "is_feasible", "n_active", "n_soft_active")


def pack(out, prefix, ref, **inputs):
    for k in KEEP:
        out[prefix + k] = ref[k]
    out[prefix + "active_lower"] = np.packbits(ref["active_lower"], axis=1, bitorder="little")
    out[prefix + "active_upper"] = np.packbits(ref["active_upper"], axis=1, bitorder="little")
    out[prefix + "neq"] = ref["neq"]; out[prefix + "ncon"] = ref["ncon"]
    for k, v in inputs.items():
        out[prefix + k] = v
    print("%s polished %d of %d, active soft rows up to %d, iterations up to %d" % (prefix, (ref["polished"] == 1).sum(), len(ref["cmd"]), ref["n_soft_active"].max(), ref["iters"].max()))


if __name__ == "__main__":
    out = {}
    sp, x0, u0 = SR.large_case()
    pack(out, "large_", SR.solve_batch(sp, x0, u0), x0=x0, u0=u0, rho=SR.LARGE_RHO)
    sp = SR.full_feature_soft()
    x0, u0, yref, dmeas = RR.full_feature_batch(24)
    ref = SR.solve_batch(sp, x0, u0, yref, dmeas)
    pack(out, "full0_", ref, x0=x0, u0=u0)
    x1 = x0 @ sp["A"].T + ref["cmd"] @ sp["B"].T + dmeas[:, :, 0] @ sp["Bd"].T
    pack(out, "full1_", SR.solve_batch(sp, x1, ref["cmd"], yref, dmeas), x0=x1, u0=ref["cmd"])
    np.savez_compressed(os.path.join(HERE, "soft_oracle.npz"), **out)
