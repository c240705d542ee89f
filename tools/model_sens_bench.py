"""Times the model-sensitivity kernel (mpcx_lmpc_model_sensitivity_batch) on the benchmark workload: the quadrotor controller at
N = 20, a batch of 4096, the active sets the benchmark batch's solve ends with.  The per-instance form and the reduced form (its second, small
kernel included), next to the one-seed VJP launch of mpcx_lmpc_sensitivity_batch, the per-instance launch of mpcx_lmpc_param_sensitivity_batch
 and the solve's own time from mpcx_lmpc_time_solve_batch, all in the same run.  HIP events around `--repeats` back-to-back launches after
`--warmup` untimed ones, the median of `--rounds` such rounds.  One JSON line.

    python tools/model_sens_bench.py [--batch 4096] [--ph 20] [--repeats 50] [--rounds 7]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc  # noqa: E402
from tools.sens_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ph", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--once", action="store_true", help="one launch of each form and no timing (for a kernel trace)")
    a = ap.parse_args()
    c = quadrotor_lmpc(a.ph, device=0)
    x0, u0, yref = quadrotor_batch(a.batch)
    desc, res, keep = c.make_batch(x0, u0, yref, want_active=True, want_sequence=True)
    c.launch(desc, keep=keep)
    torch.cuda.synchronize()
    count = res.active_count.cpu().numpy()
    seed = torch.ones((a.batch, c.nu), dtype=torch.float64, device="cuda")
    first = c.modelSensitivityBatch(desc, seed_cmd=seed)
    torch.cuda.synchronize()
    flags = first.flags.cpu().numpy()
    info = c.info()
    out = {"workload": f"quadrotor N={a.ph}", "batch": a.batch, "device": torch.cuda.get_device_name(0),
           "active_rows_mean": float(count.mean()), "active_rows_max": int(count.max()), "nz": info["nz"], "model_entries": c.nx * (c.nx + c.nu + c.ndu) + c.ny * (c.nx + c.ndu),
           "flags": {str(k): int((flags == k).sum()) for k in range(4)}}
    forms = []
    d, _, k1 = c.make_sensitivity(res.active_lower, res.active_upper, res.status, seed_cmd=seed)
    forms.append(("vjp", lambda: c.launch_sensitivity(d)))
    dp, _, k2 = c.make_param_sensitivity(desc, seed_cmd=seed)
    forms.append(("param_per_instance", lambda: c.launch_param_sensitivity(dp)))
    dm, _, k3 = c.make_model_sensitivity(desc, seed_cmd=seed)
    forms.append(("model_per_instance", lambda: c.launch_model_sensitivity(dm)))
    dr, red, k4 = c.make_model_sensitivity(desc, seed_cmd=seed, reduce=True)
    forms.append(("model_reduced", lambda: c.launch_model_sensitivity(dr)))
    if a.once:
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        out["n_used"] = int(red.n_used.item())
        print(json.dumps(out))
        return
    out["solve_ms"] = c.time_launches(desc, a.repeats)
    # one descriptor per form, launched over and over: the timed loop is the C call alone, as mpcx_lmpc_time_solve_batch's is
    for name, fn in forms:
        med, lo, hi = timed(fn, a.warmup, a.repeats, a.rounds)
        out[name + "_ms"] = {"median": med, "min": lo, "max": hi}
    out["n_used"] = int(red.n_used.item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
