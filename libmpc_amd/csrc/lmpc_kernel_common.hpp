// Helpers shared by the LMPC kernel translation units (lmpc_kernels.hip, lmpc_fast.hip): address-space casts, wave-level
// primitives, the batched mat-vec.  Everything lives in an anonymous namespace: each unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <type_traits>

#include "lmpc_device.hpp"

namespace mpcx {

namespace {

#ifndef MPCX_WAVES_PER_BLOCK
#define MPCX_WAVES_PER_BLOCK 2
#endif
constexpr int kWavesPerBlock = MPCX_WAVES_PER_BLOCK;
// a working set with all signs right grows by the rows violated by at least this fraction of the largest violation: adding
// every violated row at once over-constrains, the surplus rows are shed one round later and the slowest instances ping-pong
// (max rounds 18-22 over six batches of 4096 with 0, 12-14 with 0.3; 0.1 and 0.5 are worse than either)
#ifndef MPCX_ADD_THETA
#define MPCX_ADD_THETA 0.3
#endif
// lean solve (solve_fast): thresholds of the first working set and of the rows that enter later, as fractions of the largest violation
// (round 6 tried 0.5: tools/activeset_sim.py over five batches of 4096 at N = 20 and one each at N = 10 / 50 has the mean number of rounds fall by 2 % at every
// horizon -- 3.512 -> 3.440, 3.548 -> 3.464, 3.579 -> 3.504; N = 50: 3.557 -> 3.485 -- and the GPU reports those counts; side by side on one box the benchmark
// batch is 1 % SLOWER with it (0.0459 vs 0.0463 ms: its time is its slowest instance's, whose later working sets are larger), 32768 instances 0.8 % faster,
// config 4's shard within the noise: kept at 0.3)
#ifndef MPCX_INIT_THETA
#define MPCX_INIT_THETA 0.3
#endif
#ifndef MPCX_FAST_ADD_THETA
#define MPCX_FAST_ADD_THETA 0.2
#endif

// Pointers that come out of the model struct are generic pointers to the compiler, which
// would emit flat_load (tied to both vmcnt and lgkmcnt, serialising against LDS traffic).
// Everything they point to lives in HBM: say so.
#define MPCX_GAS __attribute__((address_space(1)))
typedef const double MPCX_GAS *gdp;
typedef const int MPCX_GAS *gip;
typedef double MPCX_GAS *gdw;
template <typename T> __device__ __forceinline__ const T MPCX_GAS *gl(const T *p) { return (const T MPCX_GAS *)p; }
template <typename T> __device__ __forceinline__ T MPCX_GAS *glw(T *p) { return (T MPCX_GAS *)p; }
typedef double d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d2 ld2(gdp p) { return *reinterpret_cast<const d2 MPCX_GAS *>(p); }
__device__ __forceinline__ void st2(gdw p, double a, double b)
{
    d2 v; v.x = a; v.y = b;
    *reinterpret_cast<d2 MPCX_GAS *>(p) = v;
}

// One lane files instance b in the failure queue (lmpc_device.hpp): one atomic, one store, clamped to the list's capacity
__device__ __forceinline__ void fallback_append(int *fq, const int cap, const int b)
{
    const int at = atomicAdd(fq + kFqCount, 1);
    if (at >= 0 && at < cap) glw(fq)[kFqList + at] = b;
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }
// broadcast lane l's value (l wave-uniform): two v_readlane_b32, no LDS round trip
__device__ __forceinline__ double readlane_d(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
// (the lean kernels' elimination has a form that takes lane K's value inside the FMA instead, fmac_row_bcast in lmpc_fast.hip: MPCX_FAST_DPP_CLASSES)
constexpr int kRegCap = 16;      // working sets up to this size are factored in registers
// 1/d for a positive, well-scaled pivot: hardware estimate + two Newton steps (full precision, a third of the latency of the
// IEEE division sequence, which sits on the dependent chain of every elimination step)
__device__ __forceinline__ double pivot_rcp(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// acc += M[:, 0..ncols) * xs.  M column-major, leading dimension ld, R (even) valid rows.
template <int CP, int U = (CP == 1 ? 8 : (CP == 2 ? 4 : 2))>
__device__ __forceinline__ void matvec_acc(gdp M, int ld, int R, int ncols, const double *xs,
                                           double (&acc)[2 * CP], int lane)
{
    int off[CP];
    double t[2 * CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        const int e = 128 * c + 2 * lane;
        off[c] = e < R ? e : 0;
        t[2 * c] = 0; t[2 * c + 1] = 0;
    }
    // explicit software pipelining: issue a batch of column fetches, then consume them
    int j = 0;
    for (; j + U <= ncols; j += U) {
        d2 m[U][CP];
        double xj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            gdp col = M + (size_t)(j + u) * ld;
#pragma unroll
            for (int c = 0; c < CP; ++c) m[u][c] = ld2(col + off[c]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) xj[u] = xs[j + u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                t[2 * c] = fma(m[u][c].x, xj[u], t[2 * c]);
                t[2 * c + 1] = fma(m[u][c].y, xj[u], t[2 * c + 1]);
            }
        }
    }
    for (; j < ncols; ++j) {
        const double xj = xs[j];
        gdp col = M + (size_t)j * ld;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const d2 m = ld2(col + off[c]);
            t[2 * c] = fma(m.x, xj, t[2 * c]);
            t[2 * c + 1] = fma(m.y, xj, t[2 * c + 1]);
        }
    }
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (128 * c + 2 * lane < R) { acc[2 * c] += t[2 * c]; acc[2 * c + 1] += t[2 * c + 1]; }
}

template <int CP>
__device__ __forceinline__ void stage_store(double *xs, const double (&v)[2 * CP], int n, int lane)
{
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        const int e = 128 * c + 2 * lane;
        if (e < n) *reinterpret_cast<double2 *>(xs + e) = make_double2(v[2 * c], v[2 * c + 1]);
    }
}

__device__ __forceinline__ double ref_at(gdp p, long bs, long ks, int b, int k, int a)
{
    return p[(size_t)b * bs + (size_t)k * ks + a];
}

__device__ __forceinline__ bool violates(double v, double lo, double hi, double ea, double er)
{
    // same slack OSQP's primal tolerance would grant a fixed row
    return (v < lo - (ea + er * fabs(lo))) || (v > hi + (ea + er * fabs(hi)));
}

#define GP(field) gl(M.field)

typedef double v4d __attribute__((ext_vector_type(4)));

}  // namespace

}  // namespace mpcx
