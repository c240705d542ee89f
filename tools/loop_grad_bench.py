"""What the backward pass of the closed loop costs: the quadrotor loop (ph = 20, batch 4096, 50 ticks), the backward time per tick
beside the forward tick of the same loop for {x0 / u0 only, + weights, + model}, and the host-driven alternative beside it -- `ticks` x lmpc_cmd
under torch autograd, which keeps `ticks` autograd nodes alive and comes back to the host between ticks.

    python tools/loop_grad_bench.py [--batch 4096] [--ticks 50] [--ph 20] [--repeats 5] [--host-ticks 50]

Prints one line per leg (median and range over the repeats, milliseconds per tick) and one JSON line with everything."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--ph", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-ticks", type=int, default=50)
    a = ap.parse_args()
    import torch
    from libmpc_amd import lmpc_cmd
    from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc

    c = quadrotor_lmpc(a.ph, device=0)
    x0, u0, yref = quadrotor_batch(a.batch)
    B, T = a.batch, a.ticks
    rg = np.random.default_rng(0)
    sx, su = rg.normal(size=(T + 1, B, c.nx)), rg.normal(size=(T, B, c.nu))
    loop = c.make_loop(x0, u0, T, yref=yref)
    stream = torch.cuda.current_stream(0)

    def timed(fn):
        ms = []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            ms.append(e0.elapsed_time(e1) / T)
        ms = ms[1:]                              # the first run warms up
        return dict(median=float(np.median(ms)), lo=float(min(ms)), hi=float(max(ms)))

    out = dict(batch=B, ticks=T, ph=a.ph, repeats=a.repeats)
    out["forward"] = timed(lambda: c.run_loop(loop))
    legs = (("x0_u0", ("x0", "u0")), ("plus_weights", ("x0", "u0", "oweight", "uweight", "duweight")),
            ("plus_model", ("x0", "u0", "oweight", "uweight", "duweight", "A", "B", "C", "Bd", "Dd")))
    for name, want in legs:
        g = c.make_loop_gradient(loop, sx, su, reduce=True, want=want)
        c.run_loop(loop); torch.cuda.synchronize()
        out["backward_" + name] = timed(lambda: c.run_loop_gradient(g))
        out["flagged_" + name] = int((g.flags != 0).sum())
        c.destroy_loop_gradient(g)
    c.destroy_loop(loop)

    # the host-driven alternative: the same loop as `ticks` differentiable solves and a torch plant step, forward and backward (wall clock: the
    # host is part of what it costs)
    A, Bm = (torch.as_tensor(m, device="cuda") for m in (c._A, c._B))
    HT = min(a.host_ticks, T)
    tsx, tsu = torch.as_tensor(sx, device="cuda"), torch.as_tensor(su, device="cuda")

    def host_loop():
        x = torch.as_tensor(x0, device="cuda").requires_grad_(True)
        u = torch.as_tensor(u0, device="cuda").requires_grad_(True)
        yr = torch.as_tensor(yref, device="cuda")
        loss = (tsx[0] * x).sum()
        xs, us = x, u
        for k in range(HT):
            us = lmpc_cmd(c, xs, us, yr)
            xs = xs @ A.T + us @ Bm.T
            loss = loss + (tsx[k + 1] * xs).sum() + (tsu[k] * us).sum()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        loss.backward()
        torch.cuda.synchronize()
        return t1
    fw, bw = [], []
    for _ in range(min(a.repeats, 3) + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        t1 = host_loop()
        t2 = time.perf_counter()
        fw.append((t1 - t0) * 1e3 / HT); bw.append((t2 - t1) * 1e3 / HT)
    out["host_forward"] = dict(median=float(np.median(fw[1:])), lo=float(min(fw[1:])), hi=float(max(fw[1:])), ticks=HT)
    out["host_backward"] = dict(median=float(np.median(bw[1:])), lo=float(min(bw[1:])), hi=float(max(bw[1:])), ticks=HT)
    for k, v in out.items():
        if isinstance(v, dict):
            print(f"{k:24s} {v['median']:.4f} ms / tick ({v['lo']:.4f} ... {v['hi']:.4f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
