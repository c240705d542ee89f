"""Writes tests/golden/terminal_oracle.npz: the reference QP with the terminal block (tests/terminal_ref.py) solved for the cases of
tests/test_lmpc_terminal_gpu.py whose yardstick solves take seconds, inputs and recorded results under a prefix per case:

    fullc_   terminal_ref.full_feature_terminal() on its batch of 24, a constant output reference per instance, the controller's own disturbance
    fulls_   the same controller with a per-step output reference and a disturbance per instance
    fulls1_  ... one tick later, from the recorded commands of fulls_ (the warm-start test's second tick)

A CPU test solves the first instances of fullc_ again and compares (tests/test_lmpc_terminal.py).

    python tests/golden/make_terminal_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import terminal_ref as TR  # noqa: E402

KEEP = ("cmd", "cost", "status", "solver_status", "polished", "iters", "is_feasible")


def pack(out, prefix, ref, **inputs):
    for k in KEEP:
        out[prefix + k] = ref[k]
    out[prefix + "active_lower"] = np.packbits(ref["active_lower"], axis=1, bitorder="little")
    out[prefix + "active_upper"] = np.packbits(ref["active_upper"], axis=1, bitorder="little")
    out[prefix + "neq"] = ref["neq"]; out[prefix + "ncon"] = ref["ncon"]
    for k, v in inputs.items():
        out[prefix + k] = v
    print("%s polished %d of %d, iterations up to %d" % (prefix, (ref["polished"] == 1).sum(), len(ref["cmd"]), ref["iters"].max()))
    assert (ref["polished"] == 1).mean() >= 0.75, prefix


if __name__ == "__main__":
    out = {}
    sp = TR.full_feature_terminal()
    x0, u0, yconst, ystep, dmeas = TR.full_feature_batch(24)
    pack(out, "fullc_", TR.solve_batch(sp, x0, u0, yref=yconst), x0=x0, u0=u0)
    ref = TR.solve_batch(sp, x0, u0, yref=ystep, dmeas=dmeas)
    pack(out, "fulls_", ref, x0=x0, u0=u0)
    x1 = x0 @ sp["A"].T + ref["cmd"] @ sp["B"].T + dmeas[:, :, 0] @ sp["Bd"].T
    pack(out, "fulls1_", TR.solve_batch(sp, x1, ref["cmd"], yref=ystep, dmeas=dmeas), x0=x1, u0=ref["cmd"])
    np.savez_compressed(os.path.join(HERE, "terminal_oracle.npz"), **out)
