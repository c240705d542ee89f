"""Times the bank's gradient kernels (mpcx_lmpc_hetero_gradient_batch) on the benchmark's heterogeneous workload: 4096
quadrotor variants at N = 20, one instance each, the optimum and the active sets that batch's solve ends with, one seed on cmd per instance.
HIP events around `--repeats` back-to-back launches after `--warmup` untimed ones, the median of `--rounds` such rounds, of: the weights alone,
the weights and the bounds, every output, every output with the per-controller sums (the reduce kernel included); beside them the bank's one-seed
VJP launch (4.8b), the bank's solve with sequences, and the single-controller launches of 4.9 and 4.10 (per instance) of the quadrotor controller at
the same shape on its own solve of the same batch.  One JSON line.

    python tools/bank_grad_bench.py [--batch 4096] [--ph 20] [--repeats 50] [--rounds 7]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from libmpc_amd import LMPCHetero  # noqa: E402
from libmpc_amd.bank import MODEL_OUTPUTS, PARAM_OUTPUTS  # noqa: E402
from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc, quadrotor_variant  # noqa: E402
from tools.sens_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ph", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    het = LMPCHetero([quadrotor_variant(k, a.ph, device=-1) for k in range(a.batch)], device=0)
    x0, u0, yref = quadrotor_batch(a.batch)
    desc, res, keep, mi = het.make_batch(x0, u0, yref=yref, want_active=True, want_sequence=True)
    het.launch(desc, mi)
    torch.cuda.synchronize()
    count = res.active_count.cpu().numpy().astype(np.float64)
    seed = torch.ones((a.batch, het.nu), dtype=torch.float64, device="cuda")
    out = {"workload": f"quadrotor N={a.ph}, every instance its own controller", "batch": a.batch, "device": torch.cuda.get_device_name(0),
           "active_rows_mean": float(count.mean()), "active_rows_max": int(count.max()),
           "solve_with_sequences_ms": het.time_launches(desc, mi, a.repeats)}
    full = het.gradientBatch(desc, seed_cmd=seed, per_controller=True)
    torch.cuda.synchronize()
    flags = full.flags.cpu().numpy()
    out["flags"] = {str(k): int((flags == k).sum()) for k in range(4)}
    out["n_used_sum"] = int(full.n_used.sum().item())
    # one descriptor per form, launched over and over: the timed loop is the C call alone, as mpcx_lmpc_hetero_time_solve_batch's is
    forms = (("weights", dict(want=PARAM_OUTPUTS[:3])), ("weights_bounds", dict(want=PARAM_OUTPUTS)), ("full", dict()),
             ("full_per_controller", dict(per_controller=True)))
    for name, kw in forms:
        d, _, keep2, _ = het.make_gradient(desc, None, seed_cmd=seed, **kw)
        med, lo, hi = timed(lambda: het.launch_gradient(d), a.warmup, a.repeats, a.rounds)
        out[name + "_ms"] = {"median": med, "min": lo, "max": hi}
    d, _, keep2, _ = het.make_sensitivity(res.active_lower, res.active_upper, None, res.status, seed_cmd=seed)
    med, lo, hi = timed(lambda: het.launch_sensitivity(d), a.warmup, a.repeats, a.rounds)
    out["bank_vjp_ms"] = {"median": med, "min": lo, "max": hi}
    # the single-controller kernels at the same shape: the quadrotor controller's own solve of the same batch
    c = quadrotor_lmpc(a.ph, device=0)
    d1, r1, k1 = c.make_batch(x0, u0, yref=yref, want_active=True, want_sequence=True)
    c.launch(d1)
    torch.cuda.synchronize()
    dp, _, k2 = c.make_param_sensitivity(d1, seed_cmd=seed)
    med, lo, hi = timed(lambda: c.launch_param_sensitivity(dp), a.warmup, a.repeats, a.rounds)
    out["single_controller_param_ms"] = {"median": med, "min": lo, "max": hi}
    dm, _, k3 = c.make_model_sensitivity(d1, seed_cmd=seed, want=MODEL_OUTPUTS)
    med, lo, hi = timed(lambda: c.launch_model_sensitivity(dm), a.warmup, a.repeats, a.rounds)
    out["single_controller_model_ms"] = {"median": med, "min": lo, "max": hi}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
