"""Times the bank's sensitivity kernel (mpcx_lmpc_hetero_sensitivity_batch) on the benchmark's heterogeneous workload: 4096
quadrotor variants at N = 20, one instance each, the active sets that batch's solve ends with.  Jacobian mode (nu seeds per instance) and
one-seed VJP mode, HIP events around `--repeats` back-to-back launches after `--warmup` untimed ones, the median of `--rounds` such rounds.
Beside them the bank's own solve step (mpcx_lmpc_hetero_time_solve_batch) and the single-controller sensitivity launch (4.8) of the quadrotor
controller at the same shape on the same active words, and the bytes an instance must read -- (nu + |A|) columns of its controller's Y over the
nz rows of the decision vector, the gathered S, its model -- against the bandwidth that makes.  One JSON line.

    python tools/bank_sens_bench.py [--batch 4096] [--ph 20] [--repeats 50] [--rounds 7]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from libmpc_amd import LMPCHetero  # noqa: E402
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
    desc, res, keep, mi = het.make_batch(x0, u0, yref=yref, want_active=True)
    het.launch(desc, mi)
    torch.cuda.synchronize()
    count = res.active_count.cpu().numpy().astype(np.float64)
    solve_ms = het.time_launches(desc, mi, a.repeats)
    al, au, st = res.active_lower, res.active_upper, res.status
    seed = torch.ones((a.batch, het.nu), dtype=torch.float64, device="cuda")
    jac = het.sensitivityBatch(al, au, status=st)
    torch.cuda.synchronize()
    flags = jac.flags.cpu().numpy()
    nx, nu, ny = het.nx, het.nu, het.ny
    nz = nu * a.ph                       # (the benchmark's controllers block no moves)
    per_instance = 8.0 * ((nu + count) * nz + count * (count + 1) / 2 + nx * nx + nx * nu + ny * nx)
    out = {"workload": f"quadrotor N={a.ph}, every instance its own controller", "batch": a.batch, "device": torch.cuda.get_device_name(0),
           "active_rows_mean": float(count.mean()), "active_rows_max": int(count.max()),
           "flags": {str(k): int((flags == k).sum()) for k in range(4)},
           "solve_ms": solve_ms, "bytes_per_launch": float(per_instance.sum())}
    # one descriptor per mode, launched over and over: the timed loop is the C call alone, as mpcx_lmpc_hetero_time_solve_batch's is
    for name, kw in (("jacobian", {}), ("vjp", {"seed_cmd": seed})):
        d, _, keep, _ = het.make_sensitivity(al, au, None, st, **kw)
        med, lo, hi = timed(lambda: het.launch_sensitivity(d), a.warmup, a.repeats, a.rounds)
        out[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        out[name + "_GBps"] = out["bytes_per_launch"] / (med * 1e-3) / 1e9
    # the single-controller kernel at the same shape, on the same active words
    c = quadrotor_lmpc(a.ph, device=0)
    one = c.sensitivityBatch(al, au, status=st)
    torch.cuda.synchronize()
    f1 = one.flags.cpu().numpy()
    out["single_controller_flags"] = {str(k): int((f1 == k).sum()) for k in range(4)}
    for name, kw in (("jacobian", {}), ("vjp", {"seed_cmd": seed})):
        d, _, keep = c.make_sensitivity(al, au, st, **kw)
        med, lo, hi = timed(lambda: c.launch_sensitivity(d), a.warmup, a.repeats, a.rounds)
        out["single_controller_" + name + "_ms"] = {"median": med, "min": lo, "max": hi}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
