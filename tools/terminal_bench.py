"""What the terminal cost costs where its code runs, on the GPU box: lmpc_assemble_generic on the quadrotor (N = 20) with and
without a terminal weight (mpcx_lmpc_debug_time_kernels, HIP events over 100 launches), and lmpc_condense_models on a bank of quadrotor
variants with and without one (the bank's "flags": the condensing kernel's ms).  No pass mark; profiles/terminal_cost.txt keeps the figures.

    python tools/terminal_bench.py [batch] [controllers]
"""
import ctypes as C
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
from libmpc_amd import LMPCHetero
from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc, quadrotor_variant

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 256
ph = 20
F = np.random.default_rng(1).normal(size=(12, 12))
P = F @ F.T / 12.0
x0, u0, yref = quadrotor_batch(B)
s = torch.cuda.current_stream(0)
for rep in range(2):
    for term in (False, True):
        c = quadrotor_lmpc(ph, device=0)
        if term:
            assert c.setTerminalCost(P)
        c.debug_force_generic(True)
        c.debug_use_fused(0)
        b, r, keep = c.make_batch(x0, u0, yref=yref)
        for _ in range(20):
            c.launch(b, s)
        torch.cuda.synchronize()
        ms3 = (C.c_float * 3)()
        c._lib.mpcx_lmpc_debug_time_kernels(c._h, C.byref(b), C.c_void_p(s.cuda_stream), 100, ms3)
        print("lmpc_assemble_generic, quadrotor N = %d, batch %d, %s terminal cost: %.4f ms (lmpc_solve %.4f, fallback %.4f), LDS per wave %d doubles, solved %.3f"
              % (ph, B, "with a" if term else "no", ms3[0], ms3[1], ms3[2], int(c.debug_get("dims")[10]), (r.status == 0).float().mean().item()), flush=True)
for horizon in (20, 50):
    for rep in range(2):
        for term in (False, True):
            ctrls = [quadrotor_variant(k, horizon, device=-1) for k in range(K if horizon == 20 else K // 8)]
            if term:
                for c in ctrls:
                    assert c.setTerminalCost(P)
            bank = LMPCHetero(ctrls, device=0)
            fl = bank.debug_get(0, "flags")
            assert fl[1] == 1.0
            print("lmpc_condense_models%s, %d quadrotor variants N = %d, %s terminal cost: %.3f ms (the bank's whole set-up %.1f ms)"
                  % ("<BIG>" if horizon == 50 else "", len(ctrls), horizon, "with a" if term else "no", fl[2], fl[3]), flush=True)
            del bank
