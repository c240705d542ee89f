"""Writes tests/golden/rate_bounds_oracle.npz: the reference QP with finite delta-u rows (tests/rate_ref.py) solved for the one case of
tests/test_lmpc_rate_bounds_gpu.py whose oracle solves take a second each -- (nx, nu, ndu, ny, ph, ch) = (2, 4, 0, 1, 40, 40), 160 rate
rows.  Inputs and recorded results; the controller and its inputs are rate_ref.large_case(), and a CPU test solves the first instance
again and compares (tests/test_lmpc_rate_bounds.py).

    python tests/golden/make_rate_bounds_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import rate_ref as RR  # noqa: E402

if __name__ == "__main__":
    sp, x0, u0, yref = RR.large_case()
    ref = RR.solve_batch(sp, x0, u0, yref)
    keep = {k: ref[k] for k in ("cmd", "cost", "status", "solver_status", "polished", "iters", "is_feasible", "n_active", "n_rate_active")}
    keep["active_lower"] = np.packbits(ref["active_lower"], axis=1, bitorder="little")
    keep["active_upper"] = np.packbits(ref["active_upper"], axis=1, bitorder="little")
    np.savez_compressed(os.path.join(HERE, "rate_bounds_oracle.npz"), x0=x0, u0=u0, yref=yref, neq=ref["neq"], ncon=ref["ncon"], **keep)
    print("polished %d of %d, active rate rows %s" % ((ref["polished"] == 1).sum(), len(x0), ref["n_rate_active"]))
