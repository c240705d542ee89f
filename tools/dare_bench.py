"""Kalman gains for a fleet: the batched device call (mpcx_dare_batch, libmpc_amd.utils.kalman_gains) beside the only way there was before it, a loop
of mpcx_lmpc_kalman_gain over host-only handles (LMPC.kalman_gain), on two inputs:
  quadrotor   the (A, C) of quadrotor_variant(k, 10) for k < batch (nx = ny = 12), Qw = 0.01 I, Rv = 0.04 I
  random32    random A (n = 32, spectral radius 0.95) and C (m = 8), the same covariances
  sweep       device times only, both product forms, random inputs of n = 2 .. 32 with m = min(n, 4): what the threshold between the forms rests on
One JSON line per input (per n in the sweep).  device_ms: the C call alone on inputs that are on the device, timed with device events over `calls` calls back to
back, median / min / max of `repeats` windows, for the product form of the size class and for each form forced (lanes over the entries, the f64
matrix pipe), the three run alternately.  front_end_ms: utils.kalman_gains from numpy inputs to a synchronised result (upload included), host
clock.  host_loop_ms: the loop of LMPC.kalman_gain over `host_count` handles (their creation not included), host clock, scaled to the batch
where host_count < batch (host_loop_scaled says so).  agreement: the worst relative difference, max norm, between the device gain and the host
routine's over the controllers of the host loop.
Usage: python tools/dare_bench.py [batch] [host_count] [repeats] [calls] [quadrotor|random32|all|sweep] [sizes of the sweep, comma-separated]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libmpc_amd import LMPC, _capi  # noqa: E402
from libmpc_amd.utils import kalman_gains  # noqa: E402
from libmpc_amd.workloads import quadrotor_variant  # noqa: E402


def quadrotor_inputs(batch):
    ctrls = [quadrotor_variant(k, 10, device=-1) for k in range(batch)]
    return np.stack([c._A for c in ctrls]), np.stack([c._C for c in ctrls]), ctrls


def random_inputs(batch, host_count, n=32, m=8):
    rng = np.random.default_rng(n)
    A = rng.normal(size=(batch, n, n))
    A *= (0.95 / np.abs(np.linalg.eigvals(A)).max(axis=1))[:, None, None]
    Cm = rng.normal(size=(batch, m, n))
    ctrls = []
    for k in range(host_count):
        c = LMPC(n, 1, 0, m, 2, 2, device=-1)
        assert c.setStateSpaceModel(A[k], np.zeros((n, 1)), Cm[k])
        ctrls.append(c)
    return A, Cm, ctrls


def median_spread(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def device_times(A, Cm, Qw, Rv, repeats, calls):
    lib = _capi.lib()
    bn, n, m = A.shape[0], A.shape[1], Cm.shape[1]
    cm = lambda a: torch.as_tensor(np.ascontiguousarray(np.swapaxes(a, -1, -2))).cuda()
    Ad, Cd, Qd, Rd = cm(A), cm(Cm), cm(Qw), cm(Rv)
    X = torch.empty((bn, n, n), dtype=torch.float64, device="cuda"); G = torch.empty((bn, m, n), dtype=torch.float64, device="cuda")
    flags = torch.empty(bn, dtype=torch.int32, device="cuda"); its = torch.empty(bn, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()

    def call():
        _capi.check(lib.mpcx_dare_batch(0, _capi.DARE_ESTIMATOR, n, m, bn, Ad.data_ptr(), Cd.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), 0, 0,
                                        X.data_ptr(), G.data_ptr(), flags.data_ptr(), its.data_ptr(), s.cuda_stream))
    forms = {"size_class": 0, "lanes": 1, "mfma": 2}
    times = {k: [] for k in forms}
    gains = {}
    for name, f in forms.items():                       # warm-up of every form
        lib.mpcx_dare_debug_product(f)
        call(); call()
        torch.cuda.synchronize()
        gains[name] = G.transpose(1, 2).cpu().numpy().copy()
    for _ in range(repeats):                            # alternating, so that whatever else the machine does hits all alike
        for name, f in forms.items():
            lib.mpcx_dare_debug_product(f)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(calls):
                call()
            e1.record(s)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls)
    lib.mpcx_dare_debug_product(0)
    assert int((flags != 0).sum()) == 0
    scale = np.abs(gains["lanes"]).max(axis=(1, 2))
    forms_differ = float((np.abs(gains["lanes"] - gains["mfma"]).max(axis=(1, 2)) / scale).max())
    return {k: median_spread(v) for k, v in times.items()}, gains["size_class"], dict(min=int(its.min()), max=int(its.max())), forms_differ


def run(name, batch, host_count, repeats, calls):
    A, Cm, ctrls = quadrotor_inputs(batch) if name == "quadrotor" else random_inputs(batch, host_count)
    host_count = min(host_count, len(ctrls))
    n, m = A.shape[1], Cm.shape[1]
    Qw, Rv = 0.01 * np.eye(n), 0.04 * np.eye(m)
    dev_ms, L, doublings, forms_differ = device_times(A, Cm, Qw, Rv, repeats, calls)
    front = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Lf, _, fl = kalman_gains(A, Cm, Qw, Rv)
        torch.cuda.synchronize()
        front.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(Lf.cpu().numpy(), L)
    t0 = time.perf_counter()
    host = [c.kalman_gain(Qw, Rv, want_P=True) for c in ctrls[:host_count]]
    host_ms = (time.perf_counter() - t0) * 1e3
    agree = max(float(np.abs(L[k] - h[0]).max() / np.abs(h[0]).max()) for k, h in enumerate(host))
    its = [h[2] for h in host]
    print(json.dumps(dict(input=name, batch=batch, n=n, m=m, repeats=repeats, calls=calls, device_ms=dev_ms, doublings=doublings,
                          product_forms_relative_difference=forms_differ, front_end_ms=median_spread(front[1:]),
                          host_count=host_count, host_loop_ms=host_ms * batch / host_count, host_loop_scaled=host_count < batch,
                          host_iterations=dict(min=min(its), max=max(its)), agreement=agree,
                          host_over_device=host_ms * batch / host_count / dev_ms["size_class"]["median"])), flush=True)


def sweep(batch, repeats, calls, sizes=(2, 4, 6, 8, 10, 12, 16, 17, 24, 32)):
    for n in sizes:
        A, Cm, _ = random_inputs(batch, 0, n, min(n, 4))
        dev_ms, _, doublings, forms_differ = device_times(A, Cm, 0.01 * np.eye(n), 0.04 * np.eye(min(n, 4)), repeats, calls)
        print(json.dumps(dict(input="sweep", batch=batch, n=n, m=min(n, 4), repeats=repeats, calls=calls, device_ms=dev_ms, doublings=doublings,
                              product_forms_relative_difference=forms_differ)), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "dare_bench.py needs an MI355X"
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    host_count = int(sys.argv[2]) if len(sys.argv) > 2 else batch
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    which = sys.argv[5] if len(sys.argv) > 5 else "all"
    for name in ("quadrotor", "random32"):
        if which in (name, "all"):
            run(name, batch, host_count, repeats, calls)
    if which == "sweep":
        sweep(batch, repeats, calls, *([tuple(int(v) for v in sys.argv[6].split(","))] if len(sys.argv) > 6 else []))
