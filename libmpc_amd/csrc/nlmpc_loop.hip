// The closed loop around the batched NLMPC solve for the built-in systems (mpcx_nlmpc_loop_*, mpcx_nlmpc_plant_step_batch): the __global__
// wrappers of the bodies in mpcx/nlmpc_loop.hpp and their launchers.
//
//   nlmpc_loop_begin        x <- x0, u <- u0, row 0 of traj_x, tick counter <- 0
//   nlmpc_loop_advance<M>   tick k = the counter: the plant step, u <- cmd, the tick's row of every trajectory, counter <- k + 1
//   nlmpc_plant_step<M>     the plant step alone
//   nlmpc_ekf_begin         an observed loop's begin: the truth <- x0, the estimate <- xhat0 (or x0), P <- P0, the flags <- 0
//   nlmpc_ekf_advance<M>    an observed loop's tick: plant step, measurement and extended Kalman filter (mpcx/nlmpc_ekf.hpp), 2 NX + 2 lanes
//                           per instance, the filter's matrices in LDS
//   nlmpc_ekf_step<M>       the filter step alone
//
// Shape as lmpc_loop.hip: one wavefront per block, lane <-> instance of a tile of 64 instances.  The tick number is device state [tick, blocks
// through]: the kernel's arguments are the same at every tick, so a captured graph of one tick replays unchanged; the counter moves when the last
// block is through, and a replay with the counter at `ticks` returns before its first store.  Every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include "mpcx/nlmpc_ekf.hpp"
#include "mpcx/nlmpc_loop.hpp"
#include "nlmpc_zoo.hpp"

namespace mpcx {

namespace {

constexpr int kTile = engine::kLoopTile;

__global__ __launch_bounds__(kTile) void nlmpc_loop_begin_kernel(const NlmpcLoopDev L, const int nx, const int nu)
{
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kTile;
    const int nvalid = min(kTile, L.batch - b0);
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {
        const double v = engine::loop_gin(L.x0)[xo + idx];
        engine::loop_gout(L.x)[xo + idx] = v;
        engine::loop_gout(L.traj_x)[xo + idx] = v;
    }
    for (int idx = tid; idx < nvalid * nu; idx += kTile) engine::loop_gout(L.u)[uo + idx] = engine::loop_gin(L.u0)[uo + idx];
    if (blockIdx.x == 0 && tid == 0) { engine::loop_gout(L.state)[0] = 0; engine::loop_gout(L.state)[1] = 0; }
}

template <class Mdl>
__global__ __launch_bounds__(kTile) void nlmpc_loop_advance_kernel(const NlmpcDev M, const NlmpcLoopDev L)
{
    const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(L.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k >= L.ticks) return;                     // a replay past the run's end: nothing is written
    engine::loop_advance_tile<Mdl>(M, L, k);
    // the counter moves when the last block is through: a block that starts late still reads tick k
    __threadfence();
    if (threadIdx.x == 0) {
        const int done = atomicAdd(L.state + 1, 1);
        if (done == (int)gridDim.x - 1) {
            __hip_atomic_store(L.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(L.state, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <class Mdl>
__global__ __launch_bounds__(kTile) void nlmpc_plant_step_kernel(const NlmpcDev M, const int batch, const double *x, const double *u, const double *params,
                                                                 const int nparams, const double *noise, const int substeps, double *x_next)
{
    engine::loop_plant_tile<Mdl>(M, batch, x, u, params, nparams, noise, substeps, x_next);
}

__global__ __launch_bounds__(kTile) void nlmpc_ekf_begin_kernel(const NlmpcLoopDev L, const NlmpcEkfDev E, const int nx, const int nu)
{
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kTile;
    const int nvalid = min(kTile, L.batch - b0);
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu, po = xo * nx;
    const double *xh0 = E.xhat0 ? E.xhat0 : L.x0, *P0 = E.cb + (size_t)E.ny * nx + (size_t)nx * nx + (size_t)E.ny * E.ny;
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {
        const double v = engine::loop_gin(L.x0)[xo + idx], vh = engine::loop_gin(xh0)[xo + idx];
        engine::loop_gout(E.xt)[xo + idx] = v;
        engine::loop_gout(L.traj_x)[xo + idx] = v;
        engine::loop_gout(L.x)[xo + idx] = vh;
        engine::loop_gout(E.traj_xhat)[xo + idx] = vh;
    }
    for (int idx = tid; idx < nvalid * nu; idx += kTile) engine::loop_gout(L.u)[uo + idx] = engine::loop_gin(L.u0)[uo + idx];
    for (int idx = tid; idx < nvalid * nx * nx; idx += kTile) {
        const double v = engine::loop_gin(P0)[idx % (nx * nx)];
        engine::loop_gout(E.P)[po + idx] = v;
        if (E.traj_P) engine::loop_gout(E.traj_P)[po + idx] = v;
    }
    if (tid < nvalid) engine::loop_gout(E.flags)[b0 + tid] = 0;
    if (blockIdx.x == 0 && tid == 0) { engine::loop_gout(L.state)[0] = 0; engine::loop_gout(L.state)[1] = 0; }
}

template <class Mdl>
__global__ __launch_bounds__(kTile) void nlmpc_ekf_advance_kernel(const NlmpcDev M, const NlmpcLoopDev L, const NlmpcEkfDev E)
{
    __shared__ double lds[engine::EkfLay<Mdl::NX>::DOUBLES];
    const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(L.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k >= L.ticks) return;                     // a replay past the run's end: nothing is written
    engine::ekf_advance_tile<Mdl>(M, L, E, k, lds);
    __threadfence();
    if (threadIdx.x == 0) {
        const int done = atomicAdd(L.state + 1, 1);
        if (done == (int)gridDim.x - 1) {
            __hip_atomic_store(L.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(L.state, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <class Mdl>
__global__ __launch_bounds__(kTile) void nlmpc_ekf_step_kernel(const NlmpcDev M, const int batch, const double *xhat, const double *P, const double *u,
                                                               const double *y, const double *params, const int nparams, const double *cb, const int ny,
                                                               const int substeps, double *xhat_next, double *P_next, int *flags)
{
    __shared__ double lds[engine::EkfLay<Mdl::NX>::DOUBLES];
    engine::ekf_step_tile<Mdl>(M, batch, xhat, P, u, y, params, nparams, cb, ny, substeps, xhat_next, P_next, flags, lds);
}

inline int tiles(int batch) { return (batch + kTile - 1) / kTile; }
template <class Mdl> inline int ekf_blocks(int batch) { constexpr int ipw = engine::EkfLay<Mdl::NX>::IPW; return (batch + ipw - 1) / ipw; }

}  // namespace

int nlmpc_loop_begin(const NlmpcDev *m, const NlmpcLoopDev *L, void *stream)
{
    hipLaunchKernelGGL(nlmpc_loop_begin_kernel, dim3(tiles(L->batch)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *L, m->nx, m->nu);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int nlmpc_loop_advance(const NlmpcDev *m, const NlmpcLoopDev *L, void *stream)
{
    return dispatch_model(m->model_id, [&](auto mdl) {
        hipLaunchKernelGGL(nlmpc_loop_advance_kernel<decltype(mdl)>, dim3(tiles(L->batch)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *m, *L);
        return hipGetLastError() == hipSuccess ? 0 : -3;
    });
}

int nlmpc_plant_step(const NlmpcDev *m, int batch, const double *x, const double *u, const double *params, int nparams, const double *noise,
                     int substeps, double *x_next, void *stream)
{
    return dispatch_model(m->model_id, [&](auto mdl) {
        hipLaunchKernelGGL(nlmpc_plant_step_kernel<decltype(mdl)>, dim3(tiles(batch)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *m, batch, x, u,
                           params, nparams, noise, substeps, x_next);
        return hipGetLastError() == hipSuccess ? 0 : -3;
    });
}

int nlmpc_ekf_begin(const NlmpcDev *m, const NlmpcLoopDev *L, const NlmpcEkfDev *E, void *stream)
{
    hipLaunchKernelGGL(nlmpc_ekf_begin_kernel, dim3(tiles(L->batch)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *L, *E, m->nx, m->nu);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int nlmpc_ekf_advance(const NlmpcDev *m, const NlmpcLoopDev *L, const NlmpcEkfDev *E, void *stream)
{
    return dispatch_model(m->model_id, [&](auto mdl) {
        using Mdl = decltype(mdl);
        hipLaunchKernelGGL(nlmpc_ekf_advance_kernel<Mdl>, dim3(ekf_blocks<Mdl>(L->batch)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *m, *L, *E);
        return hipGetLastError() == hipSuccess ? 0 : -3;
    });
}

int nlmpc_ekf_step(const NlmpcDev *m, int batch, const double *xhat, const double *P, const double *u, const double *y, const double *params, int nparams,
                   const double *cb, int ny, int substeps, double *xhat_next, double *P_next, int *flags, void *stream)
{
    return dispatch_model(m->model_id, [&](auto mdl) {
        using Mdl = decltype(mdl);
        hipLaunchKernelGGL(nlmpc_ekf_step_kernel<Mdl>, dim3(ekf_blocks<Mdl>(batch)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *m, batch, xhat, P, u, y,
                           params, nparams, cb, ny, substeps, xhat_next, P_next, flags);
        return hipGetLastError() == hipSuccess ? 0 : -3;
    });
}

}  // namespace mpcx
