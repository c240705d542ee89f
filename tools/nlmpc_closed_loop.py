"""Receding-horizon NLMPC loop on the device: B UGV controllers, each tick = one batched solve + one
plant step (the closed loop of examples/ugv_ex.cpp for a batch), cold starts against the shifted warm start of
NLOptimizer::run (NLOptimizer.hpp:460-510) with the carried curvature estimate.  Two legs, run alternately: the loop driven from
the host (optimizeBatch and NLMPC.plant_step per tick) and the device loop (NLMPC.make_loop / run_loop: a tick is a graph replay);
each line gives both legs' ms per tick (median, min, max), mean iterations and the fraction that did not fail.  A last line is the
host-driven loop with the shifted start alone (no carried curvature), which the device loop has no counterpart of.
Usage: python tools/nlmpc_closed_loop.py [batch] [ticks] [repeats]

With a fourth argument `observed` the two legs are the device loop with output feedback (ekf=: the positions are measured, an extended Kalman
filter in the advance step) beside the plain device loop of the same build, cold and warm.  The measurement noise is small
(standard deviation 1e-6 unless a fifth argument gives another) so that the estimate stays where the truth is and the solves take the
iterations they take without a filter: the figure then times the filter's kernel and not extra SQP iterations (DESIGN 4.3c names the pitfall;
the UGV's solves react to an estimate that is 2e-6 off: profiles/nlmpc_observed_loop.txt); with 0 there is no measurement noise, the estimate is
the truth bit for bit and the two legs differ by the filter's kernel alone.  The iteration counts of both legs are printed.
Usage: python tools/nlmpc_closed_loop.py [batch] [ticks] [repeats] observed [meas_noise_sd]"""
import json
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from tools.nlmpc_bench import make  # noqa: E402


def run(c, x0, u0, ticks, warm, curvature=False):
    """the host-driven loop: one batched solve and one plant-step kernel per tick"""
    B = x0.shape[0]
    x = x0.clone(); u = u0.clone()
    z = None
    its = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        r = c.optimizeBatch(x, u, z_warm=z if warm else None, warm_curvature=curvature)
        u = r["cmd"]
        x = c.plant_step(x, u)
        z = r["z"]
        its += r["iterations"].float().mean()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = float((r["status"] != 3).float().mean())
    return dict(warm=warm, keep_curvature=curvature, batch=B, ticks=ticks, solves_per_s=B * ticks / dt, ms_per_tick=dt / ticks * 1e3,
                mean_iterations=float(its) / ticks, not_failed=ok)


def run_device(c, loop):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = c.run_loop(loop)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B, ticks = res.u.shape[1], loop.ticks
    return dict(device_loop=True, batch=B, ticks=ticks, solves_per_s=B * ticks / dt, ms_per_tick=dt / ticks * 1e3,
                mean_iterations=float(res.iterations.float().mean()), not_failed=float((res.status[-1] != 3).float().mean()))


def median_spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def observed_leg(c, x0, u0, ticks, repeats, sd=1e-6):
    """the observed device loop beside the unobserved one, run alternately"""
    import numpy as np
    from libmpc_amd.nlmpc import NLEkf
    B = x0.shape[0]
    g = torch.Generator(device="cpu"); g.manual_seed(11)
    v = (sd * torch.randn((ticks, B, 2), generator=g, dtype=torch.float64)).cuda()
    var = max(sd * sd, 1e-12)               # (sd = 0: no measurement noise at all -- the estimate is the truth bit for bit, the solves are the same solves)
    ekf = NLEkf(Q=1e-2 * var * np.eye(4), R=var * np.eye(2), P0=var * np.eye(4), C=np.eye(4)[:2])
    for w in (False, True):
        plain = c.make_loop(x0, u0, ticks, warm=w)
        obs = c.make_loop(x0, u0, ticks, warm=w, ekf=ekf, meas_noise=v)
        run_device(c, plain); run_device(c, obs)                  # warm-up of both legs
        a, b = [], []
        for _ in range(repeats):
            a.append(run_device(c, plain)); b.append(run_device(c, obs))
        am, alo, ahi = median_spread([r["ms_per_tick"] for r in a])
        bm, blo, bhi = median_spread([r["ms_per_tick"] for r in b])
        err = float((obs.result.xhat - obs.result.x).abs().max())
        print(json.dumps(dict(leg="observed", warm=w, batch=B, ticks=ticks, repeats=repeats, meas_noise_sd=sd,
                              unobserved_ms_per_tick=dict(median=am, min=alo, max=ahi), observed_ms_per_tick=dict(median=bm, min=blo, max=bhi),
                              unobserved_mean_iterations=a[-1]["mean_iterations"], observed_mean_iterations=b[-1]["mean_iterations"],
                              unobserved_not_failed=a[-1]["not_failed"], observed_not_failed=b[-1]["not_failed"],
                              max_estimate_error=err, updates_skipped=int(obs.result.ekf_flags.sum()))), flush=True)
        c.destroy_loop(plain); c.destroy_loop(obs)


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    c, x0, u0 = make("ugv", B)
    x0 = x0.cuda(); u0 = u0.cuda()
    if len(sys.argv) > 4 and sys.argv[4] == "observed":
        observed_leg(c, x0, u0, ticks, repeats, float(sys.argv[5]) if len(sys.argv) > 5 else 1e-6)
        sys.exit(0)
    for w in (False, True):
        loop = c.make_loop(x0, u0, ticks, warm=w)
        run_device(c, loop); run(c, x0, u0, ticks, w, w)          # warm-up of both legs
        host, dev = [], []
        for _ in range(repeats):                                  # alternating, so that whatever else the machine does hits both alike
            host.append(run(c, x0, u0, ticks, w, w)); dev.append(run_device(c, loop))
        hm, hlo, hhi = median_spread([r["ms_per_tick"] for r in host])
        dm, dlo, dhi = median_spread([r["ms_per_tick"] for r in dev])
        print(json.dumps(dict(warm=w, keep_curvature=w, batch=B, ticks=ticks, repeats=repeats,
                              host_ms_per_tick=dict(median=hm, min=hlo, max=hhi), device_ms_per_tick=dict(median=dm, min=dlo, max=dhi),
                              host_mean_iterations=host[-1]["mean_iterations"], device_mean_iterations=dev[-1]["mean_iterations"],
                              host_not_failed=host[-1]["not_failed"], device_not_failed=dev[-1]["not_failed"])), flush=True)
        c.destroy_loop(loop)
    print(json.dumps(run(c, x0, u0, ticks, True, False)), flush=True)
