"""Times the sensitivity kernel (mpcx_lmpc_sensitivity_batch) on the benchmark workload: the quadrotor controller at N = 20, a batch
of 4096, the active sets the benchmark batch's solve ends with.  Jacobian mode (nu seeds per instance) and one-seed VJP mode, HIP events around
`--repeats` back-to-back launches after `--warmup` untimed ones, the median of `--rounds` such rounds; the solve's own time from
mpcx_lmpc_time_solve_batch beside them.  One JSON line.

    python tools/sens_bench.py [--batch 4096] [--ph 20] [--repeats 50] [--rounds 7]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc  # noqa: E402


def timed(fn, warmup, repeats, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / repeats)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ph", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    c = quadrotor_lmpc(a.ph, device=0)
    x0, u0, yref = quadrotor_batch(a.batch)
    desc, res, keep = c.make_batch(x0, u0, yref, want_active=True)
    c.launch(desc, keep=keep)
    torch.cuda.synchronize()
    count = res.active_count.cpu().numpy()
    solve_ms = c.time_launches(desc, a.repeats)
    al, au, st = res.active_lower, res.active_upper, res.status
    seed = torch.ones((a.batch, c.nu), dtype=torch.float64, device="cuda")
    jac = c.sensitivityBatch(al, au, status=st)
    torch.cuda.synchronize()
    flags = jac.flags.cpu().numpy()
    out = {"workload": f"quadrotor N={a.ph}", "batch": a.batch, "device": torch.cuda.get_device_name(0),
           "active_rows_mean": float(count.mean()), "active_rows_max": int(count.max()),
           "flags": {str(k): int((flags == k).sum()) for k in range(4)},
           "solve_ms": solve_ms}
    # one descriptor per mode, launched over and over: the timed loop is the C call alone, as mpcx_lmpc_time_solve_batch's is
    for name, kw in (("jacobian", {}), ("vjp", {"seed_cmd": seed})):
        d, _, keep = c.make_sensitivity(al, au, st, **kw)
        med, lo, hi = timed(lambda: c.launch_sensitivity(d), a.warmup, a.repeats, a.rounds)
        out[name + "_ms"] = {"median": med, "min": lo, "max": hi}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
