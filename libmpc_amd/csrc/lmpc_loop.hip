// The closed loop around the batched LMPC solve (mpcx_lmpc_loop_*, include/mpcx.h): what runs between two solves of a receding-horizon
// run, on the device, so that a tick is "solve, advance" with no host work in between.
//
//   lmpc_loop_begin    x <- x0, u <- u0, row 0 of traj_x, the preview windows of tick 0, tick counter <- 0
//   lmpc_loop_advance  tick k = the counter: x <- A_p x + B_p cmd + Bd_p d_k + w_k, u <- cmd, the tick's row of every trajectory, the
//                      active sets handed to the next solve's warm start, the preview windows of tick k + 1, counter <- k + 1
//
// Shape: one wavefront per block, lane <-> instance of a tile of 64 instances.  The instance-major arrays ([B x n], a tile of them is one
// contiguous run) go through LDS both ways -- global accesses walk the run element by element across the lanes, the lane then reads its own
// instance's row from LDS at an odd stride.  The plant [A_p | B_p | Bd_p] is the same for every lane: it is read through the constant
// address space, i.e. by scalar loads into SGPRs, and feeds the FMAs as a scalar operand.  No register arrays (the dimensions are run-time
// values), hence no scratch.  The tick number is device state: the kernel's arguments are the same at every tick, so a captured graph of one
// tick replays unchanged; a replay with the counter at `ticks` returns before its first store.
#include <hip/hip_runtime.h>

#include "lmpc_device.hpp"

namespace mpcx {

namespace {

constexpr int kTile = 64;                         // instances per block = lanes of its one wavefront

#define LOOP_GAS __attribute__((address_space(1)))
#define LOOP_CAS __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ const T LOOP_GAS *gin(const T *p) { return (const T LOOP_GAS *)p; }
template <typename T> __device__ __forceinline__ T LOOP_GAS *gout(T *p) { return (T LOOP_GAS *)p; }

// the window of ph rows starting at row `row0` of every preview array, for the tile's instances: per instance one contiguous run of
// ph * n doubles in the source ([B x (ticks + ph) x n]) and in the staging buffer the solve reads as a per-step reference ([B x ph x n])
__device__ __forceinline__ void gather_windows(const LmpcLoopDev &L, const int b0, const int nvalid, const int row0, const int tid)
{
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!L.pv_src[a]) continue;
        const int n = L.pv_n[a], run = L.ph * n;
        const size_t src_bs = (size_t)(L.ticks + L.ph) * n;
        const double LOOP_GAS *src = gin(L.pv_src[a]) + (size_t)row0 * n;
        double LOOP_GAS *dst = gout(L.pv_dst[a]);
        for (int idx = tid; idx < nvalid * run; idx += kTile) {
            const int r = idx / run, c = idx - r * run;
            dst[(size_t)b0 * run + idx] = src[(size_t)(b0 + r) * src_bs + c];
        }
    }
}

__global__ __launch_bounds__(kTile) void lmpc_loop_begin_kernel(const LmpcLoopDev L)
{
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kTile;
    const int nvalid = min(kTile, L.batch - b0);
    const size_t xo = (size_t)b0 * L.nx, uo = (size_t)b0 * L.nu;
    for (int idx = tid; idx < nvalid * L.nx; idx += kTile) {
        const double v = gin(L.x0)[xo + idx];
        gout(L.x)[xo + idx] = v;
        gout(L.traj_x)[xo + idx] = v;
    }
    for (int idx = tid; idx < nvalid * L.nu; idx += kTile) gout(L.u)[uo + idx] = gin(L.u0)[uo + idx];
    gather_windows(L, b0, nvalid, 0, tid);
    if (blockIdx.x == 0 && tid == 0) { gout(L.state)[0] = 0; gout(L.state)[1] = 0; }
}

__global__ __launch_bounds__(kTile) void lmpc_loop_advance_kernel(const LmpcLoopDev L)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(L.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k >= L.ticks) return;                     // a replay past the run's end: nothing is written
    const int nx = L.nx, nu = L.nu, ndu = L.ndu, B = L.batch;
    const int sx = L.sx, su = L.su, sd = L.sd;
    const int b0 = blockIdx.x * kTile;
    const int nvalid = min(kTile, B - b0);
    double *xin = lds, *cin = xin + kTile * sx, *din = cin + kTile * su, *xout = din + kTile * sd;
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;

    // in: the tile's states, commands and exogenous-input samples, one contiguous run each
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {
        const int r = idx / nx, c = idx - r * nx;
        xin[r * sx + c] = gin(L.x)[xo + idx];
    }
    double LOOP_GAS *tu = gout(L.traj_u) + (size_t)k * B * nu;
    for (int idx = tid; idx < nvalid * nu; idx += kTile) {
        const int r = idx / nu, c = idx - r * nu;
        const double v = gin(L.cmd)[uo + idx];
        cin[r * su + c] = v;
        gout(L.u)[uo + idx] = v;                  // lastU of the next tick: the command as it is
        tu[uo + idx] = v;
    }
    if (ndu > 0) {                                // d_k: column 0 of this tick's exogenous input, wherever its layout keeps it
        const double LOOP_GAS *dk = gin(L.dmeas) + (size_t)k * L.d_tick;
        for (int idx = tid; idx < nvalid * ndu; idx += kTile) {
            const int r = idx / ndu, c = idx - r * ndu;
            din[r * sd + c] = dk[(size_t)(b0 + r) * L.d_bs + c];
        }
    }
    __syncthreads();

    // the plant step of the lane's instance, row by row of [A_p | B_p | Bd_p] (row-major, the rows of the three side by side per matrix)
    if (tid < nvalid) {
        const double LOOP_CAS *Ap = (const double LOOP_CAS *)L.plant;
        const double LOOP_CAS *Bp = Ap + nx * nx, *Dp = Bp + nx * nu;
        const double *xr = xin + tid * sx, *ur = cin + tid * su, *dr = din + tid * sd;
        for (int i = 0; i < nx; ++i) {
            double acc = 0.0;
#pragma unroll 8
            for (int j = 0; j < nx; ++j) acc = fma(Ap[i * nx + j], xr[j], acc);
#pragma unroll 4
            for (int j = 0; j < nu; ++j) acc = fma(Bp[i * nu + j], ur[j], acc);
#pragma unroll 2
            for (int j = 0; j < ndu; ++j) acc = fma(Dp[i * ndu + j], dr[j], acc);
            xout[tid * sx + i] = acc;
        }
    }
    __syncthreads();

    // out: the new state (plus the process disturbance the controller knows nothing about) to the loop's x and to row k + 1 of traj_x
    {
        double LOOP_GAS *tx = gout(L.traj_x) + (size_t)(k + 1) * B * nx;
        const double LOOP_GAS *w = L.noise ? gin(L.noise) + (size_t)k * B * nx : nullptr;
        for (int idx = tid; idx < nvalid * nx; idx += kTile) {
            const int r = idx / nx, c = idx - r * nx;
            double v = xout[r * sx + c];
            if (w) v += w[xo + idx];
            gout(L.x)[xo + idx] = v;
            tx[xo + idx] = v;
        }
    }
    // the tick's row of the per-instance logs
    if (tid < nvalid) {
        const int b = b0 + tid;
        const size_t at = (size_t)k * B + b;
        if (L.traj_cost) gout(L.traj_cost)[at] = gin(L.cost)[b];
        if (L.traj_status) gout(L.traj_status)[at] = gin(L.status)[b];
        if (L.traj_solver_status) gout(L.traj_solver_status)[at] = gin(L.solver_status)[b];
        if (L.traj_iterations) gout(L.traj_iterations)[at] = gin(L.iterations)[b];
        if (L.traj_polish_rounds) gout(L.traj_polish_rounds)[at] = gin(L.polish_rounds)[b];
        if (L.traj_active_count) gout(L.traj_active_count)[at] = gin(L.active_count)[b];
    }
    // this tick's active sets become the next solve's first working sets
    if (L.warm_lower) {
        const size_t ao = (size_t)b0 * L.aw;
        for (int idx = tid; idx < nvalid * L.aw; idx += kTile) {
            gout(L.warm_lower)[ao + idx] = gin(L.active_lower)[ao + idx];
            gout(L.warm_upper)[ao + idx] = gin(L.active_upper)[ao + idx];
        }
    }
    if (k + 1 < L.ticks) gather_windows(L, b0, nvalid, k + 1, tid);

    // the counter moves when the last block is through: a block that starts late still reads tick k
    __threadfence();
    if (tid == 0) {
        const int done = atomicAdd(L.state + 1, 1);
        if (done == (int)gridDim.x - 1) {
            __hip_atomic_store(L.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(L.state, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

inline int odd(int n) { return n | 1; }

}  // namespace

void lmpc_loop_plan_lds(LmpcLoopDev &L)
{
    L.sx = odd(L.nx); L.su = odd(L.nu); L.sd = L.ndu > 0 ? odd(L.ndu) : 0;
}

size_t lmpc_loop_lds_bytes(const LmpcLoopDev &L) { return (size_t)kTile * (2 * L.sx + L.su + L.sd) * sizeof(double); }

int lmpc_loop_prepare(const LmpcLoopDev &L)
{
    const size_t bytes = lmpc_loop_lds_bytes(L);
    if (bytes > lmpc_lds_limit()) return -2;
    if (bytes > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(lmpc_loop_advance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return -3;
    return 0;
}

int lmpc_loop_begin(const LmpcLoopDev &L, void *stream)
{
    const int blocks = (L.batch + kTile - 1) / kTile;
    hipLaunchKernelGGL(lmpc_loop_begin_kernel, dim3(blocks), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_advance(const LmpcLoopDev &L, void *stream)
{
    const int blocks = (L.batch + kTile - 1) / kTile;
    hipLaunchKernelGGL(lmpc_loop_advance_kernel, dim3(blocks), dim3(kTile), lmpc_loop_lds_bytes(L), reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mpcx
