"""Writes tests/golden/offset_free_gain_truth.npz: the 60-digit solutions (make_dare_golden.truth) of the estimator Riccati equation of two
models augmented with their integrating disturbance model, Aa = [[A, Bd], [0, I]], Ca = [C, Dd], Q = blkdiag(Qw, Qd) -- what
libmpc_amd.utils.disturbance_gains solves -- rounded to float64.  `random`: random_lmpc_spec(3) (nx = 3, ndu = 1, ny = 2); `quadrotor`: the
quadrotor with Bd = B, Dd = 0 (nx = 12, ndu = 4, ny = 12).  Per model A, Bd, C, Dd, Qw, Qd, Rv, P [n x n] and L [n x ny], n = nx + ndu.

    python tests/golden/make_offset_free_golden.py          (needs mpmath)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, "offset_free_gain_truth.npz")


def models():
    from helpers import random_lmpc_spec
    from oracle.lmpc_numpy import quadrotor_model
    sp = random_lmpc_spec(3)
    A, B, C = quadrotor_model()
    return {"random": (sp["A"], sp["Bd"], sp["C"], sp["Dd"]), "quadrotor": (A, B.copy(), C, np.zeros((12, 4)))}


def main():
    from make_dare_golden import truth
    out = {}
    for name, (A, Bd, C, Dd) in models().items():
        nx, ndu, ny = A.shape[0], Bd.shape[1], C.shape[0]
        Qw, Qd, Rv = 0.01 * np.eye(nx), 0.05 * np.eye(ndu), 0.04 * np.eye(ny)
        Aa = np.block([[A, Bd], [np.zeros((ndu, nx)), np.eye(ndu)]]); Ca = np.hstack([C, Dd])
        Q = np.block([[Qw, np.zeros((nx, ndu))], [np.zeros((ndu, nx)), Qd]])
        P, K = truth(Aa.T, Ca.T, Q, Rv)               # the control form of the dual: K = L'
        for key, M in (("A", A), ("Bd", Bd), ("C", C), ("Dd", Dd), ("Qw", Qw), ("Qd", Qd), ("Rv", Rv), ("P", P), ("L", K.T)):
            out[name + "." + key] = np.ascontiguousarray(M)
    np.savez(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
