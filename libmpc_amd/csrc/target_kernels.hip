// Batched steady-state target maps on the device (no reference counterpart: libmpc++ has no target calculator).  An instance is a model
// (A, B, Bd, C, Dd); its target for a reference r, a disturbance estimate dhat and an input reference ubar is
//     minimise 1/2 |us - ubar|^2   subject to   (I - A) xs - B us = Bd dhat,   C xs = r - Dd dhat
// which is linear in (r, dhat, ubar): us = Tr r + Td dhat + Tu ubar, xs likewise.  The map is the solution of the KKT system
//     K = [[W, S'], [S, 0]],   S = [[I - A, -B], [C, 0]],   W = blkdiag(0_nx, I_nu),   order nk = 2 nx + nu + ny
// for nrhs = ny + ndu + nu right-hand sides: r (identity in the last ny rows), dhat (Bd in the (I - A) rows, -Dd in the last ny rows), ubar
// (identity in the us rows).  K is non-singular exactly where rank S = nx + ny (every reference reachable: ny <= nu) and rank [I - A; C] = nx
// (no unobservable integrator); where nu = ny the system collapses to S z = rhs and Tu = 0.
// One instance per wavefront, grid-stride over the batch, the augmented [K | rhs] row-major in LDS (nk (nk + nrhs) doubles): Gaussian
// elimination with partial pivoting -- the pivot by a wave reduction over (magnitude, row) with a total order, rows swapped across the whole
// augmented matrix, a lane per column down its rows, reciprocal pivots -- then back-substitution with a lane per right-hand column.  Both the
// columns (nk + nrhs) and the rows (nk) may pass 64: every loop strides by the wavefront.  K(0, 0) = 0 always: nothing works without the swaps.
// Flags per instance: 0 fine; 1 singular -- a pivot column that is zero or holds a non-finite entry, or a non-finite entry of the solution.  A
// flagged instance gets NaN in all of its outputs.  Every decision is the same in all lanes; an instance's bits depend on its own inputs and on the
// dimensions alone.  Held to, element-wise against 60-digit solutions (tests/target_ref.py): |T - T*| <= c nk 2^-52 cond_inf(K) max|T*|.
//
// target_apply: us[b] = map_u[b or shared] [r_b; dhat_b; ubar_b], a thread per (instance, row), the row's sum by target_us_row
// (target_device.hpp) -- the definition the closed loop's kernels use.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "target_device.hpp"

namespace mpcx {
namespace {

__device__ __forceinline__ void target_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int target_wave_or(int v)
{
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// all matrices column-major per instance: A [nx x nx], B [nx x nu], Bd [nx x ndu], C [ny x nx], Dd [ny x ndu]
__global__ __launch_bounds__(64) void target_map(int nx, int nu, int ndu, int ny, int batch, const double *__restrict__ Ag,
                                                 const double *__restrict__ Bg, const double *__restrict__ Bdg, const double *__restrict__ Cg,
                                                 const double *__restrict__ Ddg, double *__restrict__ map_u, double *__restrict__ map_x,
                                                 int *__restrict__ flags)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int nz = nx + nu, nk = nz + nx + ny, nrhs = ny + ndu + nu, ld = nk + nrhs;
    double *M = sm;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const double *A = Ag + (size_t)b * nx * nx, *Bm = Bg + (size_t)b * nx * nu, *Bd = Bdg + (size_t)b * nx * ndu;
        const double *Cm = Cg + (size_t)b * ny * nx, *Dd = Ddg + (size_t)b * ny * ndu;
        // [K | rhs]: zero, then the blocks (a barrier between: the blocks overwrite zeros other lanes stored)
        for (int e = lane; e < nk * ld; e += 64) M[e] = 0.0;
        target_sync();
        for (int e = lane; e < nx * nx; e += 64) {                  // I - A in S, its transpose in S'
            const int j = e / nx, i = e - j * nx;
            const double v = (i == j ? 1.0 : 0.0) - A[e];
            M[(nz + i) * ld + j] = v;
            M[j * ld + nz + i] = v;
        }
        for (int e = lane; e < nx * nu; e += 64) {                  // -B
            const int j = e / nx, i = e - j * nx;
            const double v = -Bm[e];
            M[(nz + i) * ld + nx + j] = v;
            M[(nx + j) * ld + nz + i] = v;
        }
        for (int e = lane; e < ny * nx; e += 64) {                  // C
            const int j = e / ny, i = e - j * ny;
            const double v = Cm[e];
            M[(nz + nx + i) * ld + j] = v;
            M[j * ld + nz + nx + i] = v;
        }
        for (int e = lane; e < nu; e += 64) { M[(nx + e) * ld + nx + e] = 1.0; M[(nx + e) * ld + nk + ny + ndu + e] = 1.0; }      // W; ubar's columns
        for (int e = lane; e < ny; e += 64) M[(nz + nx + e) * ld + nk + e] = 1.0;                                                // r's columns
        for (int e = lane; e < nx * ndu; e += 64) { const int j = e / nx, i = e - j * nx; M[(nz + i) * ld + nk + ny + j] = Bd[e]; }
        for (int e = lane; e < ny * ndu; e += 64) { const int j = e / ny, i = e - j * ny; M[(nz + nx + i) * ld + nk + ny + j] = -Dd[e]; }
        target_sync();

        int flag = 0;
        for (int k = 0; k < nk; ++k) {
            // the largest entry of column k from row k down, the lowest row among equals: a lane over its rows in ascending order, then the
            // wavefront -- a total order, so every lane ends with the same pair
            double pv = -1.0;
            int pi = k, bad = 0;
            for (int i = k + lane; i < nk; i += 64) {
                const double v = fabs(M[i * ld + k]);
                bad |= !(v <= DBL_MAX);
                if (v > pv) { pv = v; pi = i; }
            }
            if (target_wave_or(bad)) { flag = 1; break; }
            for (int o = 32; o; o >>= 1) {
                const double ov = __shfl_xor(pv, o);
                const int oi = __shfl_xor(pi, o);
                if (ov > pv || (ov == pv && oi < pi)) { pv = ov; pi = oi; }
            }
            if (!(pv > 0.0)) { flag = 1; break; }
            if (pi != k) {
                for (int j = lane; j < ld; j += 64) { const double t = M[k * ld + j]; M[k * ld + j] = M[pi * ld + j]; M[pi * ld + j] = t; }
                target_sync();
            }
            // a lane per column right of the pivot, down its rows: column k (the multipliers) and the pivot row are only read in this step
            const double rinv = 1.0 / M[k * ld + k];
            for (int j = k + 1 + lane; j < ld; j += 64) {
                const double top = M[k * ld + j];
                for (int i = k + 1; i < nk; ++i) M[i * ld + j] -= (M[i * ld + k] * rinv) * top;
            }
            target_sync();
        }
        if (!flag) {
            int bad = 0;
            for (int c = nk + lane; c < ld; c += 64) {
                for (int i = nk - 1; i >= 0; --i) {
                    double v = M[i * ld + c];
                    for (int j = i + 1; j < nk; ++j) v -= M[i * ld + j] * M[j * ld + c];
                    v /= M[i * ld + i];
                    M[i * ld + c] = v;
                    if (i < nz) bad |= !(fabs(v) <= DBL_MAX);
                }
            }
            target_sync();
            if (target_wave_or(bad)) flag = 1;
        }
        const double nan = __builtin_nan("");
        for (int e = lane; e < nu * nrhs; e += 64) {
            const int c = e / nu, i = e - c * nu;
            map_u[(size_t)b * nu * nrhs + e] = flag ? nan : M[(nx + i) * ld + nk + c];
        }
        if (map_x)
            for (int e = lane; e < nx * nrhs; e += 64) {
                const int c = e / nx, i = e - c * nx;
                map_x[(size_t)b * nx * nrhs + e] = flag ? nan : M[i * ld + nk + c];
            }
        if (flags && lane == 0) flags[b] = flag;
        target_sync();
    }
}

constexpr int kApplyThreads = 256;

__global__ __launch_bounds__(kApplyThreads) void target_apply(int nu, int ndu, int ny, int batch, const double *__restrict__ map_u, int map_per_instance,
                                                              const double *__restrict__ r, const double *__restrict__ dhat,
                                                              const double *__restrict__ ubar, double *__restrict__ us)
{
    const size_t total = (size_t)batch * nu, step = (size_t)gridDim.x * kApplyThreads;
    const size_t len = (size_t)nu * (ny + ndu + nu);
    for (size_t idx = (size_t)blockIdx.x * kApplyThreads + threadIdx.x; idx < total; idx += step) {
        const size_t b = idx / nu;
        const int i = (int)(idx - b * nu);
        const double *T = map_u + (map_per_instance ? b * len : 0) + i;
        us[idx] = target_us_row(T, (size_t)nu, r + b * ny, ny, dhat + b * ndu, ndu, ubar + b * nu, nu);
    }
}

}  // namespace

size_t target_map_lds_bytes(int nx, int nu, int ndu, int ny)
{
    const size_t nk = (size_t)2 * nx + nu + ny;
    return nk * (nk + ny + ndu + nu) * sizeof(double);
}

// 0; -2: the augmented matrix exceeds lds_limit; -3: a launch or its configuration failed
int target_map_launch(int nx, int nu, int ndu, int ny, int batch, const double *A, const double *B, const double *Bd, const double *C, const double *Dd,
                      double *map_u, double *map_x, int *flags, size_t lds_limit, void *stream)
{
    const size_t lds = target_map_lds_bytes(nx, nu, ndu, ny);
    if (lds > lds_limit) return -2;
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(target_map), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -3;
    const int blocks = batch < 4096 ? batch : 4096;
    hipLaunchKernelGGL(target_map, dim3(blocks), dim3(64), lds, reinterpret_cast<hipStream_t>(stream), nx, nu, ndu, ny, batch, A, B, Bd, C, Dd, map_u,
                       map_x, flags);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int target_apply_launch(int nu, int ndu, int ny, int batch, const double *map_u, int map_per_instance, const double *r, const double *dhat,
                        const double *ubar, double *us, void *stream)
{
    size_t blocks = ((size_t)batch * nu + kApplyThreads - 1) / kApplyThreads;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(target_apply, dim3((unsigned)blocks), dim3(kApplyThreads), 0, reinterpret_cast<hipStream_t>(stream), nu, ndu, ny, batch, map_u,
                       map_per_instance, r, dhat, ubar, us);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mpcx
