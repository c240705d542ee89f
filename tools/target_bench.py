"""Steady-state target maps for a fleet: the batched device call (mpcx_target_map_batch, libmpc_amd.utils.target_maps) beside the host's way, a
loop of numpy.linalg.solve on each instance's KKT system, on two inputs:
  quadrotor   `batch` variants of the four-output quadrotor (workloads.quadrotor_target_model with B and Bd scaled per instance): nx = 12,
              nu = ndu = ny = 4, a KKT system of order 32 with 12 right-hand sides
  limit       `limit_batch` random models of the largest shape the kernel takes, (nx, nu, ndu, ny) = (58, 8, 4, 8): order 132, 20 right-hand
              sides, 160 512 bytes of LDS per wavefront -- one wavefront per compute unit
One JSON line per input.  device_ms: the C call alone on inputs that are on the device, timed with device events over `calls` calls back to back,
median / min / max of `repeats` windows.  front_end_ms: utils.target_maps from numpy inputs to a synchronised result (the rank check on the
host and the upload included), host clock; front_end_unchecked_ms: the same with check_rank=False.  host_loop_ms: numpy.linalg.solve over `host_count` instances, assembling each K included, host
clock, scaled to the batch where host_count < batch (host_loop_scaled says so).  agreement: the worst relative difference, max norm, between the
device's map_u and numpy's over the instances of the host loop.
Usage: python tools/target_bench.py [batch] [limit_batch] [host_count] [repeats] [calls] [quadrotor|limit|all]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libmpc_amd import _capi  # noqa: E402
from libmpc_amd.utils import target_maps  # noqa: E402
from libmpc_amd.workloads import quadrotor_target_model  # noqa: E402


def quadrotor_inputs(batch):
    A, B, _, C, Dd = quadrotor_target_model()
    s = np.random.default_rng(4).uniform(0.85, 1.15, size=(batch, 1, 1))
    rep = lambda M: np.broadcast_to(M, (batch,) + M.shape).copy()
    return rep(A), s * B[None], s * B[None], rep(C), rep(Dd)


def limit_inputs(batch, dims=(58, 8, 4, 8)):
    nx, nu, ndu, ny = dims
    rng = np.random.default_rng(nx)
    A = rng.normal(size=(batch, nx, nx))
    A *= (0.9 / np.abs(np.linalg.eigvals(A)).max(axis=1))[:, None, None]
    return A, rng.normal(size=(batch, nx, nu)), rng.normal(size=(batch, nx, ndu)), rng.normal(size=(batch, ny, nx)), rng.normal(size=(batch, ny, ndu))


def kkt(A, B, Bd, C, Dd):
    nx, nu = B.shape
    ndu, ny = Bd.shape[1], C.shape[0]
    nz, nk = nx + nu, 2 * nx + nu + ny
    K = np.zeros((nk, nk)); R = np.zeros((nk, ny + ndu + nu))
    K[nz:nz + nx, :nx] = np.eye(nx) - A; K[nz:nz + nx, nx:nz] = -B; K[nz + nx:, :nx] = C
    K[:nz, nz:] = K[nz:, :nz].T
    K[nx:nz, nx:nz] = np.eye(nu)
    R[nz + nx:, :ny] = np.eye(ny); R[nz:nz + nx, ny:ny + ndu] = Bd; R[nz + nx:, ny:ny + ndu] = -Dd; R[nx:nz, ny + ndu:] = np.eye(nu)
    return K, R


def median_spread(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def device_times(mats, repeats, calls):
    lib = _capi.lib()
    A, B, Bd, C, Dd = mats
    bn, nx, nu, ndu, ny = A.shape[0], A.shape[1], B.shape[2], Bd.shape[2], C.shape[1]
    cm = lambda a: torch.as_tensor(np.ascontiguousarray(np.swapaxes(a, -1, -2))).cuda()
    dev = [cm(M) for M in mats]
    Tu = torch.empty((bn, ny + ndu + nu, nu), dtype=torch.float64, device="cuda")
    flags = torch.empty(bn, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()

    def call():
        _capi.check(lib.mpcx_target_map_batch(0, nx, nu, ndu, ny, bn, *(d.data_ptr() for d in dev), Tu.data_ptr(), None, flags.data_ptr(), s.cuda_stream))
    call(); call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(calls):
            call()
        e1.record(s)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / calls)
    assert int((flags != 0).sum()) == 0
    return median_spread(times), Tu.transpose(1, 2).cpu().numpy().copy()


def run(name, batch, host_count, repeats, calls):
    mats = quadrotor_inputs(batch) if name == "quadrotor" else limit_inputs(batch)
    host_count = min(host_count, batch)
    nx, nu, ndu, ny = mats[0].shape[1], mats[1].shape[2], mats[2].shape[2], mats[3].shape[1]
    dev_ms, T = device_times(mats, repeats, calls)
    front, bare = [], []
    for _ in range(repeats + 1):
        for times, check in ((front, True), (bare, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Tf, fl = target_maps(*mats, check_rank=check)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(Tf.cpu().numpy(), T)
    t0 = time.perf_counter()
    host = []
    for k in range(host_count):
        K, R = kkt(*(M[k] for M in mats))
        host.append(np.linalg.solve(K, R)[nx:nx + nu])
    host_ms = (time.perf_counter() - t0) * 1e3
    agree = max(float(np.abs(T[k] - h).max() / np.abs(h).max()) for k, h in enumerate(host))
    print(json.dumps(dict(input=name, batch=batch, nx=nx, nu=nu, ndu=ndu, ny=ny, order=2 * nx + nu + ny, repeats=repeats, calls=calls, device_ms=dev_ms,
                          front_end_ms=median_spread(front[1:]), front_end_unchecked_ms=median_spread(bare[1:]), host_count=host_count, host_loop_ms=host_ms * batch / host_count,
                          host_loop_scaled=host_count < batch, agreement=agree, host_over_device=host_ms * batch / host_count / dev_ms["median"])),
          flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "target_bench.py needs an MI355X"
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    limit_batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    host_count = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    calls = int(sys.argv[5]) if len(sys.argv) > 5 else 20
    which = sys.argv[6] if len(sys.argv) > 6 else "all"
    if which in ("quadrotor", "all"):
        run("quadrotor", batch, host_count, repeats, calls)
    if which in ("limit", "all"):
        run("limit", limit_batch, host_count, repeats, calls)
