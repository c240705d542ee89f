// The backward pass of the plain closed loop (mpcx_lmpc_loop_grad_*, include/mpcx.h): what runs between two vector-Jacobian
// launches of the adjoint recursion, on the device, so that a backward tick is "re-solve, VJP launches, adjoint" with no host work in between.
//
//   lmpc_loop_grad_begin    lambda <- seed_x[ticks] (or 0), mu <- 0, every accumulator and flag <- 0, the inputs of the re-solve of tick ticks - 1
//                           and c_{ticks-1}, tick counter <- ticks - 1
//   lmpc_loop_grad_adjoint  tick k = the counter, lambda = lambda_{k+1}, (gx, gu, gy, g_theta) the VJP of tick k's solve seeded with c_k:
//                             d_noise[k] <- lambda;  d_plant += lambda [x_k; cmd_k; d_k]';  d_yref += gy;  d_theta += g_theta;  flag |= the tick's
//                             lambda <- (A_p' lambda + seed_x[k]) + gx;  mu <- gu
//                             x <- traj_x[k-1], u <- traj_u[k-2] (u0 at tick 0), the preview windows of row k - 1,
//                             c <- (B_p' lambda + seed_u[k-1]) + mu;  counter <- k - 1
//   lmpc_loop_grad_finish   d_x0 <- lambda_0, d_u0 <- mu_0; NaN in every per-instance output of an instance whose flag is not 0
//   lmpc_loop_grad_sum      reduce = 1: the per-instance accumulators of the instances whose flag is 0 added up, a workgroup per 64 instances in
//                           instance order into its row of the partials, then the ordered reduce of lmpc_sens_common.hpp over the rows
//
// Shapes follow lmpc_loop.hip.  One wavefront per block.  The uniform form (one plant for the batch): lane <-> instance of a tile of 64, the plant
// [A_p | B_p | Bd_p] row-major through the constant address space, i.e. scalar operands.  The per-instance form (plant_batch): lane <-> (instance,
// row) over the packed plant block, ipw = 64 / nx instances per wavefront; the rows of c (nu of them) are taken by the same nx lanes and can
// outnumber them: that loop strides by lpi.
//
// The products are transposed: row j of A_p' lambda is column j of A_p.  In the packed block a term is a column -- term j of instance q is the run of
// nx doubles at ((t terms + j) ipw + q) nx -- so the lane of (q, j) sums its column directly from global memory, element by element of a contiguous
// run, with lambda from LDS.  No partial sums cross lanes and the plant never goes through LDS; the only barriers are those between a tile's staging
// and its use.  In the uniform form the lane walks the same column at stride nx (or nu) through scalar loads.
//
// Order of every sum, both forms: acc = 0, fma by ascending row, then + seed, then + gx (lambda) or + mu (c).  The two forms agree bit for bit on
// equal plants: everything but the two products is the same flat loop over the tile's contiguous runs in both.  Accumulators are plain += in tick
// order (the outer product one fma per entry), so two runs give the same bits.  No register arrays sized by run-time dimensions, hence no scratch;
// vector stores only.  The tick number is device state: the kernel's arguments are the same at every tick, so one captured tick replays unchanged;
// a replay with the counter below 0 returns before its first store.
#include <hip/hip_runtime.h>

#include "lmpc_device.hpp"
#include "lmpc_sens_common.hpp"

namespace mpcx {

namespace {

constexpr int kTile = 64;                         // lanes of a block's one wavefront; instances of a tile in the uniform form

#define LOOP_CAS __attribute__((address_space(4)))

// an instance's LDS row: [lambda_{k+1} | x_k | cmd_k | d_k | lambda_k | mu_k]; cmd's slot is reused for the sums of c once the outer product is through
struct Row { int lam, x, cmd, d, ln, mu; };
__device__ __forceinline__ Row row_of(const LmpcLoopGradDev &G)
{
    Row r;
    r.lam = 0; r.x = G.nx; r.cmd = 2 * G.nx; r.d = r.cmd + G.nu; r.ln = r.d + G.ndu; r.mu = r.ln + G.nx;
    return r;
}

// the window of ph rows starting at row `row0` of every preview array, for the tile's instances (lmpc_loop.hip's gather_windows)
__device__ __forceinline__ void grad_windows(const LmpcLoopGradDev &G, const int b0, const int nvalid, const int row0, const int tid)
{
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!G.pv_src[a]) continue;
        const int n = G.pv_n[a], run = G.ph * n;
        const size_t src_bs = (size_t)(G.ticks + G.ph) * n;
        const double MPCX_GAS *src = gl(G.pv_src[a]) + (size_t)row0 * n;
        double MPCX_GAS *dst = glw(G.pv_dst[a]);
        for (int idx = tid; idx < nvalid * run; idx += kTile) {
            const int r = idx / run, c = idx - r * run;
            dst[(size_t)b0 * run + idx] = src[(size_t)(b0 + r) * src_bs + c];
        }
    }
}

// column j of the matrix whose columns are the terms first .. of the plant, times the vector v (LDS), summed from 0 by ascending row.
// kPlants: the packed block, the column a contiguous run; else the row-major matrix M [nx x ncols] by scalar loads
template <bool kPlants>
__device__ __forceinline__ double column_sum(const LmpcLoopGradDev &G, const double MPCX_GAS *Pq, const int first, const double LOOP_CAS *M, const int ncols,
                                             const int j, const double *v)
{
    const int nx = G.nx;
    double acc = 0.0;
    if constexpr (kPlants) {
        const double MPCX_GAS *col = Pq + (size_t)(first + j) * G.ipw * nx;
        int i = 0;
#pragma unroll 1
        for (; i + 4 <= nx; i += 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fma(col[i + e], v[i + e], acc);
        }
#pragma unroll 1
        for (; i < nx; ++i) acc = fma(col[i], v[i], acc);
    } else {
#pragma unroll 4
        for (int i = 0; i < nx; ++i) acc = fma(M[i * ncols + j], v[i], acc);
    }
    return acc;
}

// the product rows of the block's tile: out[j] = sum_i M[i, j] v[i] for the nrows columns j of the plant's terms first .., of every instance of
// the tile; v at offset vin of the instance's LDS row, the sums to offset vout
template <bool kPlants>
__device__ __forceinline__ void transposed_product(const LmpcLoopGradDev &G, double *lds, const int nvalid, const int first, const int nrows,
                                                   const int vin, const int vout)
{
    const int tid = threadIdx.x, nx = G.nx, sg = G.sg;
    if constexpr (kPlants) {
        const int lpi = min(nx, kTile), q = tid / lpi;
        if (q < nvalid) {
            const size_t per_tile = (size_t)(nx + G.nu + G.ndu) * G.ipw * nx;
            const double MPCX_GAS *Pq = gl(G.pk) + (size_t)blockIdx.x * per_tile + (size_t)q * nx;
            double *row = lds + q * sg;
            for (int j = tid - q * lpi; j < nrows; j += lpi) row[vout + j] = column_sum<true>(G, Pq, first, nullptr, 0, j, row + vin);
        }
    } else {
        if (tid < nvalid) {
            const double LOOP_CAS *M = (const double LOOP_CAS *)G.plant + (first == 0 ? 0 : nx * nx);
            double *row = lds + tid * sg;
            for (int j = 0; j < nrows; ++j) row[vout + j] = column_sum<false>(G, nullptr, first, M, nrows, j, row + vin);
        }
    }
}

// What a tick leaves for the next replay, the tick kn >= 0 that replay differentiates: its solve's inputs x <- traj_x[kn], u <- traj_u[kn - 1] (the
// caller's u0 at tick 0), the preview windows of row kn, and c_kn = (B_p' lambda + seed_u[kn]) + mu with lambda, mu of tick kn + 1 at the row's ln
// and mu.  Ends behind a barrier.
template <bool kPlants>
__device__ __forceinline__ void stage_next(const LmpcLoopGradDev &G, double *lds, const int b0, const int nvalid, const int kn)
{
    const int tid = threadIdx.x, nx = G.nx, nu = G.nu, sg = G.sg, B = G.batch;
    const Row R = row_of(G);
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;
    transposed_product<kPlants>(G, lds, nvalid, nx, nu, R.ln, R.cmd);
    {
        const double MPCX_GAS *tx = gl(G.traj_x) + (size_t)kn * B * nx;
        for (int idx = tid; idx < nvalid * nx; idx += kTile) glw(G.x)[xo + idx] = tx[xo + idx];
        const double MPCX_GAS *tu = kn > 0 ? gl(G.traj_u) + (size_t)(kn - 1) * B * nu : gl(G.u0);
        for (int idx = tid; idx < nvalid * nu; idx += kTile) glw(G.u)[uo + idx] = tu[uo + idx];
    }
    grad_windows(G, b0, nvalid, kn, tid);
    __syncthreads();
    const double MPCX_GAS *su = G.seed_u ? gl(G.seed_u) + (size_t)kn * B * nu : nullptr;
    for (int idx = tid; idx < nvalid * nu; idx += kTile) {
        const int r = idx / nu, c = idx - r * nu;
        double v = lds[r * sg + R.cmd + c];
        if (su) v += su[uo + idx];
        v += lds[r * sg + R.mu + c];
        glw(G.c)[uo + idx] = v;
    }
}

// the ticket that moves the counter when the last block is through (lmpc_loop.hip's finish_tick)
__device__ __forceinline__ void move_counter(const LmpcLoopGradDev &G, const int to)
{
    __threadfence();
    if (threadIdx.x == 0) {
        const int done = atomicAdd(G.state + 1, 1);
        if (done == (int)gridDim.x - 1) {
            __hip_atomic_store(G.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(G.state, to, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool kPlants>
__device__ __forceinline__ void begin_run(const LmpcLoopGradDev &G, double *lds)
{
    const int tid = threadIdx.x, nx = G.nx, nu = G.nu, sg = G.sg, B = G.batch;
    const int nt = kPlants ? G.ipw : kTile;
    const int b0 = blockIdx.x * nt, nvalid = min(nt, B - b0);
    const Row R = row_of(G);
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;
    const double MPCX_GAS *sx = G.seed_x ? gl(G.seed_x) + (size_t)G.ticks * B * nx : nullptr;
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {
        const int r = idx / nx, c = idx - r * nx;
        const double v = sx ? sx[xo + idx] : 0.0;
        lds[r * sg + R.ln + c] = v;
        glw(G.lam)[xo + idx] = v;
    }
    for (int idx = tid; idx < nvalid * nu; idx += kTile) {
        const int r = idx / nu, c = idx - r * nu;
        lds[r * sg + R.mu + c] = 0.0;
        glw(G.mu)[uo + idx] = 0.0;
    }
    // the accumulators of the tile's instances, each one contiguous run
    if (G.a_yref) for (int idx = tid; idx < nvalid * G.ny; idx += kTile) glw(G.a_yref)[(size_t)b0 * G.ny + idx] = 0.0;
    if (G.a_plant) {
        const int plen = nx * (nx + nu + G.ndu);
        for (int idx = tid; idx < nvalid * plen; idx += kTile) glw(G.a_plant)[(size_t)b0 * plen + idx] = 0.0;
    }
#pragma unroll 1
    for (int s = 0; s < kLoopGradSlots; ++s) {
        if (!G.acc[s]) continue;
        const int len = G.len[s];
        for (int idx = tid; idx < nvalid * len; idx += kTile) glw(G.acc[s])[(size_t)b0 * len + idx] = 0.0;
    }
    if (tid < nvalid) glw(G.flags)[b0 + tid] = 0;
    __syncthreads();
    stage_next<kPlants>(G, lds, b0, nvalid, G.ticks - 1);
    if (blockIdx.x == 0 && tid == 0) { glw(G.state)[0] = G.ticks - 1; glw(G.state)[1] = 0; }
}

template <bool kPlants>
__device__ __forceinline__ void adjoint_tick(const LmpcLoopGradDev &G, double *lds)
{
    const int tid = threadIdx.x, nx = G.nx, nu = G.nu, ndu = G.ndu, sg = G.sg, B = G.batch;
    const int nt = kPlants ? G.ipw : kTile;
    const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(G.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k < 0 || k >= G.ticks) return;
    const int b0 = blockIdx.x * nt, nvalid = min(nt, B - b0);
    const Row R = row_of(G);
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;

    // in: lambda_{k+1} (which is d_noise[k]), x_k, cmd_k, d_k and mu_k = gu of the tile's instances, one contiguous run each
    {
        const double MPCX_GAS *tx = gl(G.traj_x) + (size_t)k * B * nx;
        double MPCX_GAS *dn = G.d_noise ? glw(G.d_noise) + (size_t)k * B * nx : nullptr;
        for (int idx = tid; idx < nvalid * nx; idx += kTile) {
            const int r = idx / nx, c = idx - r * nx;
            const double l = gl(G.lam)[xo + idx];
            lds[r * sg + R.lam + c] = l;
            lds[r * sg + R.x + c] = tx[xo + idx];
            if (dn) dn[xo + idx] = l;
        }
        const double MPCX_GAS *tu = gl(G.traj_u) + (size_t)k * B * nu;
        for (int idx = tid; idx < nvalid * nu; idx += kTile) {
            const int r = idx / nu, c = idx - r * nu;
            const double g = gl(G.gu)[uo + idx];
            lds[r * sg + R.cmd + c] = tu[uo + idx];
            lds[r * sg + R.mu + c] = g;
            glw(G.mu)[uo + idx] = g;
        }
        if (ndu > 0) {
            const double MPCX_GAS *dk = gl(G.dmeas) + (size_t)k * G.d_tick;
            for (int idx = tid; idx < nvalid * ndu; idx += kTile) {
                const int r = idx / ndu, c = idx - r * ndu;
                lds[r * sg + R.d + c] = dk[(size_t)(b0 + r) * G.d_bs + c];
            }
        }
    }
    __syncthreads();

    // d_plant += lambda [x_k; cmd_k; d_k]': entry (term j, row i) of an instance at j nx + i, plant_batch's layout; [x | cmd | d] lie side by side
    if (G.a_plant) {
        const int plen = nx * (nx + nu + ndu);
        double MPCX_GAS *ap = glw(G.a_plant) + (size_t)b0 * plen;
        for (int idx = tid; idx < nvalid * plen; idx += kTile) {
            const int r = idx / plen, e = idx - r * plen, j = e / nx, i = e - j * nx;
            ap[idx] = fma(lds[r * sg + R.lam + i], lds[r * sg + R.x + j], ap[idx]);
        }
    }
    // the tick's per-instance vector-Jacobian products into their accumulators, the tick's flags into the instance's
    if (G.a_yref) {
        const size_t yo = (size_t)b0 * G.ny;
        for (int idx = tid; idx < nvalid * G.ny; idx += kTile) glw(G.a_yref)[yo + idx] += gl(G.gy)[yo + idx];
    }
#pragma unroll 1
    for (int s = 0; s < kLoopGradSlots; ++s) {
        if (!G.acc[s]) continue;
        const int len = G.len[s];
        const size_t o = (size_t)b0 * len;
        for (int idx = tid; idx < nvalid * len; idx += kTile) glw(G.acc[s])[o + idx] += gl(G.tick_out[s])[o + idx];
    }
    if (tid < nvalid) {
        int32_t f = gl(G.flags)[b0 + tid];
        for (int t = 0; t < G.ntf; ++t) f |= gl(G.tflags)[(size_t)t * B + b0 + tid];
        glw(G.flags)[b0 + tid] = f;
    }

    // lambda_k = (A_p' lambda_{k+1} + seed_x[k]) + gx
    transposed_product<kPlants>(G, lds, nvalid, 0, nx, R.lam, R.ln);
    __syncthreads();                              // (the outer product's reads of cmd's slot are behind this one as well)
    {
        const double MPCX_GAS *sx = G.seed_x ? gl(G.seed_x) + (size_t)k * B * nx : nullptr;
        for (int idx = tid; idx < nvalid * nx; idx += kTile) {
            const int r = idx / nx, c = idx - r * nx;
            double v = lds[r * sg + R.ln + c];
            if (sx) v += sx[xo + idx];
            v += gl(G.gx)[xo + idx];
            lds[r * sg + R.ln + c] = v;
            glw(G.lam)[xo + idx] = v;
        }
    }
    __syncthreads();
    if (k > 0) stage_next<kPlants>(G, lds, b0, nvalid, k - 1);
    move_counter(G, k - 1);
}

__global__ __launch_bounds__(kTile) void lmpc_loop_grad_begin_kernel(const LmpcLoopGradDev G)
{
    extern __shared__ double lds[];
    begin_run<false>(G, lds);
}

__global__ __launch_bounds__(kTile) void lmpc_loop_grad_begin_plants_kernel(const LmpcLoopGradDev G)
{
    extern __shared__ double lds[];
    begin_run<true>(G, lds);
}

__global__ __launch_bounds__(kTile) void lmpc_loop_grad_adjoint_kernel(const LmpcLoopGradDev G)
{
    extern __shared__ double lds[];
    adjoint_tick<false>(G, lds);
}

__global__ __launch_bounds__(kTile) void lmpc_loop_grad_adjoint_plants_kernel(const LmpcLoopGradDev G)
{
    extern __shared__ double lds[];
    adjoint_tick<true>(G, lds);
}

// After the last tick: d_x0 = lambda_0, d_u0 = mu_0, and NaN in everything an instance with a flag owns -- lambda carried the NaN of the tick that
// was flagged down to tick 0, but not up to the noise rows of the later ticks, nor into accumulators that had been added to before.
__global__ __launch_bounds__(kTile) void lmpc_loop_grad_finish_kernel(const LmpcLoopGradDev G)
{
    const int tid = threadIdx.x, nx = G.nx, nu = G.nu, B = G.batch;
    const int b0 = blockIdx.x * kTile, nvalid = min(kTile, B - b0);
    const double nan = __builtin_nan("");
    auto put = [&](double *dst, const double *src, const int len, const size_t tick_stride) {
        if (!dst) return;
        double MPCX_GAS *o = glw(dst) + tick_stride + (size_t)b0 * len;
        for (int idx = tid; idx < nvalid * len; idx += kTile) {
            const bool bad = gl(G.flags)[b0 + idx / len] != 0;
            if (src) o[idx] = bad ? nan : gl(src)[(size_t)b0 * len + idx];
            else if (bad) o[idx] = nan;
        }
    };
    put(G.d_x0, G.lam, nx, 0);
    put(G.d_u0, G.mu, nu, 0);
    put(G.a_yref, nullptr, G.ny, 0);
    put(G.a_plant, nullptr, nx * (nx + nu + G.ndu), 0);
    for (int s = 0; s < kLoopGradSlots; ++s) put(G.acc[s], nullptr, G.len[s], 0);
    for (int k = 0; k < G.ticks; ++k) put(G.d_noise, nullptr, nx, (size_t)k * B * nx);
}

// reduce = 1, first half: workgroup g adds the instances g 64 .. of flag 0 in instance order, an entry of the concatenated arrays per thread, into row
// g of the partials; the last entry counts them
__global__ __launch_bounds__(256) void lmpc_loop_grad_partial_kernel(const LmpcLoopGradSum S, const size_t plen)
{
    const int first = blockIdx.x * kLoopGradGroup, last = min(first + kLoopGradGroup, S.batch);
    for (size_t t = threadIdx.x; t < plen; t += blockDim.x) {
        double s = 0.0;
        if (t == plen - 1) {
            for (int b = first; b < last; ++b) s += gl(S.flags)[b] == 0 ? 1.0 : 0.0;
        } else {
            size_t e = t;
            int a = 0;
            while (e >= (size_t)S.len[a]) { e -= (size_t)S.len[a]; ++a; }
            const double MPCX_GAS *src = gl(S.src[a]);
            const size_t len = (size_t)S.len[a];
            for (int b = first; b < last; ++b)
                if (gl(S.flags)[b] == 0) s += src[(size_t)b * len + e];
        }
        glw(S.part)[(size_t)blockIdx.x * plen + t] = s;
    }
}

inline int odd(int n) { return n | 1; }

struct GradLaunch { unsigned grid; size_t lds; };
GradLaunch grad_launch(const LmpcLoopGradDev &G)
{
    const int nt = G.pk ? G.ipw : kTile;
    return {(unsigned)((G.batch + nt - 1) / nt), (size_t)nt * G.sg * sizeof(double)};
}

}  // namespace

void lmpc_loop_grad_plan_lds(LmpcLoopGradDev &G) { G.sg = odd(3 * G.nx + 2 * G.nu + G.ndu); }

int lmpc_loop_grad_prepare(const LmpcLoopGradDev &G)
{
    const GradLaunch a = grad_launch(G);
    if (a.lds > lmpc_lds_limit()) return -2;
    if (a.lds > 48 * 1024) {
        const void *const kernels[2] = {G.pk ? reinterpret_cast<const void *>(lmpc_loop_grad_begin_plants_kernel) : reinterpret_cast<const void *>(lmpc_loop_grad_begin_kernel),
                                        G.pk ? reinterpret_cast<const void *>(lmpc_loop_grad_adjoint_plants_kernel) : reinterpret_cast<const void *>(lmpc_loop_grad_adjoint_kernel)};
        for (const void *f : kernels)
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds) != hipSuccess) return -3;
    }
    return 0;
}

int lmpc_loop_grad_begin(const LmpcLoopGradDev &G, void *stream)
{
    const GradLaunch a = grad_launch(G);
    hipLaunchKernelGGL((G.pk ? lmpc_loop_grad_begin_plants_kernel : lmpc_loop_grad_begin_kernel), dim3(a.grid), dim3(kTile), a.lds,
                       reinterpret_cast<hipStream_t>(stream), G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_grad_adjoint(const LmpcLoopGradDev &G, void *stream)
{
    const GradLaunch a = grad_launch(G);
    hipLaunchKernelGGL((G.pk ? lmpc_loop_grad_adjoint_plants_kernel : lmpc_loop_grad_adjoint_kernel), dim3(a.grid), dim3(kTile), a.lds,
                       reinterpret_cast<hipStream_t>(stream), G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_grad_finish(const LmpcLoopGradDev &G, void *stream)
{
    hipLaunchKernelGGL(lmpc_loop_grad_finish_kernel, dim3((unsigned)((G.batch + kTile - 1) / kTile)), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_grad_sum(const LmpcLoopGradSum &s, void *stream)
{
    const size_t plen = lmpc_loop_grad_plen(s);
    const int groups = (int)lmpc_loop_grad_groups(s.batch);
    hipLaunchKernelGGL(lmpc_loop_grad_partial_kernel, dim3((unsigned)groups), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), s, plen);
    if (hipGetLastError() != hipSuccess) return -3;
    SensReduce r{};
    r.part = s.part; r.plen = plen; r.groups = groups; r.n_used = s.n_used;
    size_t end = 0;
    for (int k = 0; k < kSensReduceSegs; ++k) { end += (size_t)s.len[k]; r.end[k] = end; r.dst[k] = s.dst[k]; }
    return sens_reduce_launch<5>(r, stream);
}

}  // namespace mpcx
