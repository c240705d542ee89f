"""Receding-horizon loop on the device: B quadrotor controllers, each tick = one batched solve +
one plant step x+ = A x + B u (the closed loop of examples/quadrotor_ex.cpp run for a batch), with and without the
warm start that carries the working set from tick to tick.  Three legs: the loop driven from the host (optimizeBatch and two
torch matmuls per tick) and the device loop (LMPC.make_loop / run_loop: the plant step is a kernel, a tick is a graph replay),
run alternately; each line gives both legs' ms per tick (median, min, max), polish rounds and solved fraction.
The bank leg (lines with "bank": true) is the same comparison for B different controllers (quadrotor_variant(k), the lmpc-hetero workload of
bench.py): the host-driven loop is LMPCHetero.optimizeBatch plus a batched torch bmm plant step per tick, the device loop is
LMPCHetero.make_loop / run_loop, every instance stepped by its own controller's model.
The observed leg (lines with "observed": true; not part of "all") is the device loop with output feedback beside the device loop without, the same
build and the same inputs, run alternately: the observer's gain is LMPC.kalman_gain(0.01 I, 0.04 I), the sensor noise has standard deviation 0.2.
The offset_free leg (lines with "offset_free": true; not part of "all") is the offset-free loop beside the observed loop, the same build and the
same inputs, run alternately: the quadrotor with an input-disturbance model (Bd = B, Dd = 0), a constant load of 0.1 per rotor and sensor noise of
standard deviation 0.01.  The observed loop is told the load as its per-instance dmeas (so both loops' solves take the same kernels) and estimates
with LMPC.kalman_gain(0.01 I, 0.04 I); the offset-free loop is told nothing and estimates with LMPC.disturbance_gain(0.01 I, 0.01 I, 0.04 I).
The target leg (lines with "target": true; not part of "all") is the offset-free loop beside the offset-free loop with steady-state targets, the
same build and the same inputs, run alternately: the quadrotor with the four outputs a target can reach (workloads.quadrotor_target_lmpc: x, y, z,
yaw; Bd = B, Dd = 0; the example's input weight 0.1), the same load and sensor noise, both estimating with LMPC.disturbance_gain(0.01 I, 0.01 I,
0.04 I); the second computes us from LMPC.target_map() at every tick.  Both loops' solves read a per-instance uref (zeros for the first).  A
third loop has the pass-through map [0 | 0 | I]: its us is ubar = 0, so its solves are the first loop's bit for bit and what its tick costs more
is what the begin, pack and advance kernels cost more -- the second loop's solves see other input references and take other rounds.  The final
errors are max |y - yref| of the last tick over the outputs, as the median and the maximum over the instances (the maximum is an unsolved one's).
Usage: python tools/closed_loop.py [batch] [ticks] [repeats] [single|bank|observed|offset_free|target|all]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from libmpc_amd.workloads import quadrotor_batch, quadrotor_lmpc, quadrotor_matrices  # noqa: E402


def run(B, ticks, warm):
    c = quadrotor_lmpc(20, device=0)
    x0, u0, yref = quadrotor_batch(B)
    Ad, Bd, _ = quadrotor_matrices()
    A = torch.as_tensor(Ad).cuda().T.contiguous(); Bm = torch.as_tensor(Bd).cuda().T.contiguous()
    x = torch.as_tensor(x0).cuda(); u = torch.as_tensor(u0).cuda(); yr = torch.as_tensor(yref).cuda()
    prev = None
    rounds = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(ticks):
        r = c.optimizeBatch(x, u, yref=yr, want_active=warm, warm=prev if warm else None, warm_shift=True)
        x = x @ A + r.cmd @ Bm
        u = r.cmd
        prev = r
        rounds += r.polish_rounds.float().mean()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(warm=warm, batch=B, ticks=ticks, solves_per_s=B * ticks / dt, ms_per_tick=dt / ticks * 1e3,
                mean_rounds=float(rounds) / ticks, solved=float((r.status == 0).float().mean()))


def make_device(B, ticks, warm):
    """the device loop of the same run, ready to be timed: (controller, loop)"""
    c = quadrotor_lmpc(20, device=0)
    x0, u0, yref = quadrotor_batch(B)
    return c, c.make_loop(x0, u0, ticks, yref=yref, warm=warm)


def make_observed(B, ticks, warm):
    """the device loop of the same run with a Kalman predictor between plant and controller: (controller, loop)"""
    c = quadrotor_lmpc(20, device=0)
    x0, u0, yref = quadrotor_batch(B)
    L = c.kalman_gain(0.01 * np.eye(c.nx), 0.04 * np.eye(c.ny))
    v = 0.2 * np.random.default_rng(1).normal(size=(ticks, B, c.ny))
    return c, c.make_loop(x0, u0, ticks, yref=yref, warm=warm, observer=L, meas_noise=v)


def make_disturbed(B, ticks, warm, offset_free):
    """the observed loop that is told the load, or the offset-free loop that estimates it: (controller, loop)"""
    c = quadrotor_lmpc(20, device=0)
    _, Bq, _ = quadrotor_matrices()
    assert c.setDisturbances(Bq, np.zeros((c.ny, c.ndu)))
    x0, u0, yref = quadrotor_batch(B)
    load = np.full((B, c.ndu), 0.1)
    v = 0.01 * np.random.default_rng(1).normal(size=(ticks, B, c.ny))
    if offset_free:
        L = c.disturbance_gain(0.01 * np.eye(c.nx), 0.01 * np.eye(c.ndu), 0.04 * np.eye(c.ny))
        return c, c.make_loop(x0, u0, ticks, yref=yref, warm=warm, disturbance_observer=L, dmeas=load, meas_noise=v)
    L = c.kalman_gain(0.01 * np.eye(c.nx), 0.04 * np.eye(c.ny))
    return c, c.make_loop(x0, u0, ticks, yref=yref, warm=warm, observer=L, dmeas=load, meas_noise=v)


def make_targeted(B, ticks, warm, targets):
    """the offset-free loop of the four-output quadrotor, without or with steady-state targets: (controller, loop)"""
    from libmpc_amd.workloads import quadrotor_target_lmpc
    c = quadrotor_target_lmpc(20, device=0)
    x0, u0, yref = quadrotor_batch(B)
    yref = np.ascontiguousarray(yref[:, [3, 4, 5, 2]])
    load = np.full((B, c.ndu), 0.1)
    v = 0.01 * np.random.default_rng(1).normal(size=(ticks, B, c.ny))
    L = c.disturbance_gain(0.01 * np.eye(c.nx), 0.01 * np.eye(c.ndu), 0.04 * np.eye(c.ny))
    kw = dict(yref=yref, uref=np.zeros((B, c.nu)), warm=warm, disturbance_observer=L, dmeas=load, meas_noise=v)
    T = None if not targets else c.target_map() if targets == "map" else np.concatenate([np.zeros((c.nu, c.ny + c.ndu)), np.eye(c.nu)], axis=1)
    return c, c.make_loop(x0, u0, ticks, target=T, **kw)


def run_device(c, loop):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = c.run_loop(loop)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B, ticks = res.u.shape[1], loop.ticks
    return dict(device_loop=True, batch=B, ticks=ticks, solves_per_s=B * ticks / dt, ms_per_tick=dt / ticks * 1e3,
                mean_rounds=float(res.polish_rounds.float().mean()), solved=float((res.status[-1] == 0).float().mean()))


def make_bank(B, ph=20):
    """B quadrotor variants behind one bank, their inputs on the device and their plants as bmm operands"""
    from libmpc_amd import LMPCHetero
    from libmpc_amd.workloads import quadrotor_variant
    ctrls = [quadrotor_variant(k, ph, device=-1) for k in range(B)]
    het = LMPCHetero(ctrls, device=0)
    x0, u0, yref = quadrotor_batch(B)
    dev = dict(x=torch.as_tensor(x0).cuda(), u=torch.as_tensor(u0).cuda(), yr=torch.as_tensor(yref).cuda(),
               At=torch.as_tensor(np.stack([c._A.T for c in ctrls])).cuda().contiguous(),
               Bt=torch.as_tensor(np.stack([c._B.T for c in ctrls])).cuda().contiguous())
    return het, (x0, u0, yref), dev


def run_bank(het, dev, ticks, warm):
    """the host-driven loop of a bank: one batched solve and x <- A_b x + B_b u as two bmm per tick"""
    x, u, yr = dev["x"], dev["u"], dev["yr"]
    prev = None
    rounds = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(ticks):
        r = het.optimizeBatch(x, u, yref=yr, want_active=warm, warm=prev if warm else None, warm_shift=True)
        x = (torch.bmm(x.unsqueeze(1), dev["At"]) + torch.bmm(r.cmd.unsqueeze(1), dev["Bt"])).squeeze(1)
        u = r.cmd
        prev = r
        rounds += r.polish_rounds.float().mean()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B = x.shape[0]
    return dict(warm=warm, batch=B, ticks=ticks, solves_per_s=B * ticks / dt, ms_per_tick=dt / ticks * 1e3,
                mean_rounds=float(rounds) / ticks, solved=float((r.status == 0).float().mean()))


def median_spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    legs = sys.argv[4] if len(sys.argv) > 4 else "all"
    if legs in ("single", "all"):
        run(B, 5, True)
    for w in (False, True) if legs in ("single", "all") else ():
        c, loop = make_device(B, ticks, w)
        run_device(c, loop)                                   # warm-up of both legs (the host leg builds its controller anew each time)
        run(B, ticks, w)
        host, dev = [], []
        for _ in range(repeats):                              # alternating, so that whatever else the machine does hits both alike
            host.append(run(B, ticks, w)); dev.append(run_device(c, loop))
        hm, hlo, hhi = median_spread([r["ms_per_tick"] for r in host])
        dm, dlo, dhi = median_spread([r["ms_per_tick"] for r in dev])
        print(json.dumps(dict(warm=w, batch=B, ticks=ticks, repeats=repeats,
                              host_ms_per_tick=dict(median=hm, min=hlo, max=hhi), device_ms_per_tick=dict(median=dm, min=dlo, max=dhi),
                              host_mean_rounds=host[-1]["mean_rounds"], device_mean_rounds=dev[-1]["mean_rounds"],
                              host_solved=host[-1]["solved"], device_solved=dev[-1]["solved"])))
        c.destroy_loop(loop)
    for w in (False, True) if legs == "observed" else ():
        c, loop = make_device(B, ticks, w)
        co, loopo = make_observed(B, ticks, w)
        run_device(c, loop); run_device(co, loopo)            # warm-up of both legs
        plain, obs = [], []
        for _ in range(repeats):                              # alternating, as above
            plain.append(run_device(c, loop)); obs.append(run_device(co, loopo))
        pm, plo, phi = median_spread([r["ms_per_tick"] for r in plain])
        om, olo, ohi = median_spread([r["ms_per_tick"] for r in obs])
        print(json.dumps(dict(observed=True, warm=w, batch=B, ticks=ticks, repeats=repeats,
                              unobserved_ms_per_tick=dict(median=pm, min=plo, max=phi), observed_ms_per_tick=dict(median=om, min=olo, max=ohi),
                              unobserved_mean_rounds=plain[-1]["mean_rounds"], observed_mean_rounds=obs[-1]["mean_rounds"],
                              unobserved_solved=plain[-1]["solved"], observed_solved=obs[-1]["solved"])))
        c.destroy_loop(loop); co.destroy_loop(loopo)
    for w in (False, True) if legs == "offset_free" else ():
        co, loopo = make_disturbed(B, ticks, w, False)
        cf, loopf = make_disturbed(B, ticks, w, True)
        run_device(co, loopo); run_device(cf, loopf)          # warm-up of both legs
        obs, off = [], []
        for _ in range(repeats):                              # alternating, as above
            obs.append(run_device(co, loopo)); off.append(run_device(cf, loopf))
        om, olo, ohi = median_spread([r["ms_per_tick"] for r in obs])
        fm, flo, fhi = median_spread([r["ms_per_tick"] for r in off])
        print(json.dumps(dict(offset_free=True, warm=w, batch=B, ticks=ticks, repeats=repeats,
                              observed_ms_per_tick=dict(median=om, min=olo, max=ohi), offset_free_ms_per_tick=dict(median=fm, min=flo, max=fhi),
                              observed_mean_rounds=obs[-1]["mean_rounds"], offset_free_mean_rounds=off[-1]["mean_rounds"],
                              observed_solved=obs[-1]["solved"], offset_free_solved=off[-1]["solved"])))
        co.destroy_loop(loopo); cf.destroy_loop(loopf)
    for w in (False, True) if legs == "target" else ():
        cf, loopf = make_targeted(B, ticks, w, None)
        ct, loopt = make_targeted(B, ticks, w, "map")
        cp, loopp = make_targeted(B, ticks, w, "pass")
        run_device(cf, loopf); run_device(ct, loopt); run_device(cp, loopp)          # warm-up of the three legs
        off, tgt, thru = [], [], []
        for _ in range(repeats):                              # alternating, as above
            off.append(run_device(cf, loopf)); tgt.append(run_device(ct, loopt)); thru.append(run_device(cp, loopp))
        fm, flo, fhi = median_spread([r["ms_per_tick"] for r in off])
        tm, tlo, thi = median_spread([r["ms_per_tick"] for r in tgt])
        pm, plo, phi = median_spread([r["ms_per_tick"] for r in thru])
        assert torch.equal(loopp.result.u, loopf.result.u)
        yr = torch.as_tensor(quadrotor_batch(B)[2][:, [3, 4, 5, 2]]).cuda()
        err = lambda loop: (loop.result.y[-1] - yr).abs().max(dim=1).values
        print(json.dumps(dict(target=True, warm=w, batch=B, ticks=ticks, repeats=repeats,
                              offset_free_ms_per_tick=dict(median=fm, min=flo, max=fhi), target_ms_per_tick=dict(median=tm, min=tlo, max=thi),
                              pass_through_ms_per_tick=dict(median=pm, min=plo, max=phi),
                              offset_free_mean_rounds=off[-1]["mean_rounds"], target_mean_rounds=tgt[-1]["mean_rounds"],
                              offset_free_solved=off[-1]["solved"], target_solved=tgt[-1]["solved"],
                              offset_free_final_error=dict(median=float(err(loopf).median()), max=float(err(loopf).max())),
                              target_final_error=dict(median=float(err(loopt).median()), max=float(err(loopt).max())))))
        cf.destroy_loop(loopf); ct.destroy_loop(loopt); cp.destroy_loop(loopp)
    if legs in ("bank", "all"):
        het, (x0, u0, yref), dev = make_bank(B)
        run_bank(het, dev, 5, True)
        for w in (False, True):
            loop = het.make_loop(x0, u0, ticks, yref=yref, warm=w)
            run_device(het, loop)                             # warm-up of both legs
            run_bank(het, dev, ticks, w)
            host, devl = [], []
            for _ in range(repeats):                          # alternating, as above
                host.append(run_bank(het, dev, ticks, w)); devl.append(run_device(het, loop))
            hm, hlo, hhi = median_spread([r["ms_per_tick"] for r in host])
            dm, dlo, dhi = median_spread([r["ms_per_tick"] for r in devl])
            print(json.dumps(dict(bank=True, warm=w, batch=B, ticks=ticks, repeats=repeats,
                                  host_ms_per_tick=dict(median=hm, min=hlo, max=hhi), device_ms_per_tick=dict(median=dm, min=dlo, max=dhi),
                                  host_mean_rounds=host[-1]["mean_rounds"], device_mean_rounds=devl[-1]["mean_rounds"],
                                  host_solved=host[-1]["solved"], device_solved=devl[-1]["solved"])))
            het.destroy_loop(loop)
