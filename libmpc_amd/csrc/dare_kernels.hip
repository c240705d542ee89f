// Batched discrete algebraic Riccati equations on the device (no reference counterpart: libmpc++ has no Riccati solver; the host routine
// mpcx_lmpc_kalman_gain is the fixed-point iteration for one controller).  One equation per wavefront, every working matrix in LDS, by the
// structure-preserving doubling algorithm (Anderson 1978; Chu, Fan, Lin, Wang 2004):
//     a_0 = A, g_0 = B R^-1 B', h_0 = Q,   W = I + g h
//     a+ = a W^-1 a,   g+ = g + a (W^-1 g) a',   h+ = h + (a' h) (W^-1 a),   h -> X
// (g+ and h+ through their symmetrised increments, so g and h stay symmetric to the bit).  Step k holds what 2^k steps of the fixed-point
// iteration X <- A'XA - A'XB (R + B'XB)^-1 B'XA + Q reach from X = 0.
//   MPCX_DARE_CONTROL    the equation above, gain K = (R + B'XB)^-1 B'XA [m x n]
//   MPCX_DARE_ESTIMATOR  P = APA' - APC' (CPC' + R)^-1 CPA' + Q, gain L = APC' (CPC' + R)^-1 [n x m]: the control form of (A', C'), L = K'.
// The form only changes how A and the second matrix are read and where an entry of the gain is written.
// Numerics: R = L L' by Cholesky (g_0 = Y'Y, L Y = B'); W is not symmetric: [W | a | g] is eliminated with partial pivoting (rows swapped
// across the augmented matrix, so no permutation is kept) and back-substituted; the gain by the Cholesky factor of R + B'XB.
// Stopping rule: after a step, max|h+ - h| <= 2^-52 max|h+| (the increments fall quadratically: what the steps not taken would add is far
// below a rounding error).  At most kDareMaxDoublings = 40 doublings (the host routine's 100 000 fixed-point steps are 17).
// Flags per instance: 0 converged; 1 R does not factor (not positive definite, or not finite); 2 the cap was reached; 3 a non-finite
// entry of a, g or h after a step, a vanishing or non-finite pivot of W, or R + B'XB does not factor.  An unstable mode that the second
// matrix does not reach ends in 3: a squares its entries every step and overflows long before the cap.  A flagged instance gets NaN in all
// of X and of the gain.  An instance's bits depend on its own inputs and on n, m alone: one wavefront, fixed orders of summation.
// Products: lanes over the entries of the result, or 16 x 16 tiles of v_mfma_f64_16x16x4_f64 with the edges padded by zeros (DESIGN.md has
// the measurements behind kDareMfmaMinN).  LDS: 6 n^2 + m^2 + 2 m n doubles -- 72 KB at n = m = 32, the limit (c2d's request at n = 48).
// Held to, element-wise against 60-digit solutions (tests/dare_ref.py): |X - X*| <= c n 2^-52 max|X*|, the gain likewise.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace mpcx {
namespace {

constexpr int kDareMaxN = 32, kDareMaxDoublings = 40;
constexpr int kDareMfmaMinN = 9;            // n from which the n x n products go through the matrix pipe

typedef double dare_v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dare_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_or(int v)
{
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int not_finite(double v) { return !(fabs(v) <= DBL_MAX); }

// C [M x N, row-major] = A B with A(i, k) = A[i ar + k ac] (M x K) and B(k, j) = B[k br + j bc] (K x N); C is neither A nor B
__device__ __forceinline__ void dare_mm(bool mfma, double *C, int M, int N, int K, const double *A, int ar, int ac, const double *B, int br,
                                        int bc, int lane)
{
    if (mfma) {
        const int r = lane & 15, q = lane >> 4;
        for (int ti = 0; ti < M; ti += 16)
            for (int tj = 0; tj < N; tj += 16) {
                dare_v4d acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < K; k0 += 4) {
                    const int k = k0 + q;
                    const double av = (ti + r < M && k < K) ? A[(ti + r) * ar + k * ac] : 0.0;
                    const double bv = (tj + r < N && k < K) ? B[k * br + (tj + r) * bc] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
                for (int rr = 0; rr < 4; ++rr) {
                    const int row = ti + q + 4 * rr, col = tj + r;
                    if (row < M && col < N) C[row * N + col] = acc[rr];
                }
            }
    } else {
        for (int e = lane; e < M * N; e += 64) {
            const int i = e / N, j = e - i * N;
            double s = 0;
            for (int k = 0; k < K; ++k) s += A[i * ar + k * ac] * B[k * br + j * bc];
            C[e] = s;
        }
    }
    dare_sync();
}

// S [m x m, row-major, symmetric] -> its lower Cholesky factor in the lower triangle; false (the same in every lane) where a pivot is not a
// positive finite number
__device__ __forceinline__ bool dare_chol(double *S, int m, int lane)
{
    for (int k = 0; k < m; ++k) {
        const double d = S[k * m + k];
        if (!(d > 0.0) || !(d <= DBL_MAX)) return false;
        const double r = sqrt(d);
        dare_sync();
        for (int i = k + lane; i < m; i += 64) S[i * m + k] = i == k ? r : S[i * m + k] / r;
        dare_sync();
        for (int j = k + 1 + lane; j < m; j += 64) {            // a lane per column of the trailing triangle: no index divisions
            const double sjk = S[j * m + k];
            for (int i = j; i < m; ++i) S[i * m + j] -= S[i * m + k] * sjk;
        }
        dare_sync();
    }
    return true;
}

// Y [m x n, row-major] <- L^-1 Y (and then L'^-1 of that where `both`), L the lower triangle of S [m x m]; a lane per column
__device__ __forceinline__ void dare_chol_solve(const double *S, int m, double *Y, int n, bool both, int lane)
{
    for (int c = lane; c < n; c += 64) {
        for (int i = 0; i < m; ++i) {
            double v = Y[i * n + c];
            for (int j = 0; j < i; ++j) v -= S[i * m + j] * Y[j * n + c];
            Y[i * n + c] = v / S[i * m + i];
        }
        if (both)
            for (int i = m - 1; i >= 0; --i) {
                double v = Y[i * n + c];
                for (int j = i + 1; j < m; ++j) v -= S[j * m + i] * Y[j * n + c];
                Y[i * n + c] = v / S[i * m + i];
            }
    }
    dare_sync();
}

// T1 <- W^-1 T1, T2 <- W^-1 T2 (all n x n, row-major; W is destroyed): Gaussian elimination of [W | T1 | T2] with partial pivoting, then
// back-substitution with a lane per right-hand column.  false (the same in every lane) for a pivot column that is zero or not finite.
__device__ __forceinline__ bool dare_lu_solve(double *W, double *T1, double *T2, int n, int lane)
{
    auto column = [&](int j) -> double * { return j < n ? W + j : j < 2 * n ? T1 + (j - n) : T2 + (j - 2 * n); };      // stride n
    for (int k = 0; k < n; ++k) {
        double pv = -1.0;
        int pi = k, bad = 0;
        if (lane >= k && lane < n) { pv = fabs(W[lane * n + k]); pi = lane; bad = !(pv <= DBL_MAX); }
        if (wave_or(bad)) return false;
        for (int o = 32; o; o >>= 1) {            // the largest entry, the lowest row among equals: a total order, so every lane ends with the same pair
            const double ov = __shfl_xor(pv, o);
            const int oi = __shfl_xor(pi, o);
            if (ov > pv || (ov == pv && oi < pi)) { pv = ov; pi = oi; }
        }
        if (!(pv > 0.0)) return false;
        if (pi != k) {
            for (int j = lane; j < 3 * n; j += 64) { double *c = column(j); const double t = c[k * n]; c[k * n] = c[pi * n]; c[pi * n] = t; }
            dare_sync();
        }
        // a lane per column right of the pivot, down its rows: column k (the multipliers) and the pivot row are only read in this step
        const double rinv = 1.0 / W[k * n + k];
        for (int j = k + 1 + lane; j < 3 * n; j += 64) {
            double *c = column(j);
            const double top = c[k * n];
            for (int i = k + 1; i < n; ++i) c[i * n] -= (W[i * n + k] * rinv) * top;
        }
        dare_sync();
    }
    for (int c = lane; c < 2 * n; c += 64) {
        double *X = c < n ? T1 + c : T2 + (c - n);
        for (int i = n - 1; i >= 0; --i) {
            double v = X[i * n];
            for (int j = i + 1; j < n; ++j) v -= W[i * n + j] * X[j * n];
            X[i * n] = v / W[i * n + i];
        }
    }
    dare_sync();
    return true;
}

__global__ __launch_bounds__(64) void dare_sda(int form, int n, int m, int batch, bool mfma, const double *__restrict__ Ag,
                                               const double *__restrict__ Bg, const double *__restrict__ Qg, const double *__restrict__ Rg,
                                               int q_stride, int r_stride, double *__restrict__ Xg, double *__restrict__ gain,
                                               int *__restrict__ flags, int *__restrict__ iterations)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x, nn = n * n;
    const bool est = form != 0;
    double *a = sm, *g = a + nn, *h = g + nn, *W = h + nn, *T1 = W + nn, *T2 = T1 + nn, *S = T2 + nn, *Y = S + m * m, *Z = Y + m * n;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const double *A = Ag + (size_t)b * nn, *Bm = Bg + (size_t)b * n * m;
        const double *Q = Qg + (size_t)b * nn * q_stride, *R = Rg + (size_t)b * m * m * r_stride;
        // a(i, j): A (column-major) in the control form, A' in the estimator form; h = Q; S = R; Z = B' [m x n] (control: B is n x m
        // column-major; estimator: B = C', C is m x n column-major)
        for (int e = lane; e < nn; e += 64) {
            const int i = e / n, j = e - i * n;
            a[e] = est ? A[i * n + j] : A[j * n + i];
            h[e] = 0.5 * (Q[i * n + j] + Q[j * n + i]);
        }
        for (int e = lane; e < m * m; e += 64) { const int i = e / m, j = e - i * m; S[e] = 0.5 * (R[i * m + j] + R[j * m + i]); }
        for (int e = lane; e < m * n; e += 64) {
            const int k = e / n, c = e - k * n;
            const double v = est ? Bm[c * m + k] : Bm[k * n + c];
            Z[e] = v; Y[e] = v;
        }
        dare_sync();
        int flag = 0, it = 0;
        if (!dare_chol(S, m, lane)) flag = 1;
        if (!flag) {
            dare_chol_solve(S, m, Y, n, false, lane);
            dare_mm(mfma, g, n, n, m, Y, 1, n, Y, n, 1, lane);              // g = Y' Y = B R^-1 B'
            flag = 2;
            while (it < kDareMaxDoublings) {
                ++it;
                dare_mm(mfma, W, n, n, n, g, n, 1, h, n, 1, lane);
                for (int e = lane; e < nn; e += 64) { if (e / n == e % n) W[e] += 1.0; T1[e] = a[e]; T2[e] = g[e]; }
                dare_sync();
                if (!dare_lu_solve(W, T1, T2, n, lane)) { flag = 3; break; }          // T1 = W^-1 a, T2 = W^-1 g
                dare_mm(mfma, W, n, n, n, a, n, 1, T2, n, 1, lane);
                dare_mm(mfma, T2, n, n, n, W, n, 1, a, 1, n, lane);             // a (W^-1 g) a'
                int bad = 0;
                for (int e = lane; e < nn; e += 64) {
                    const int i = e / n, j = e - i * n;
                    g[e] += 0.5 * (T2[e] + T2[j * n + i]);
                    bad |= not_finite(g[e]);
                }
                dare_sync();
                dare_mm(mfma, W, n, n, n, a, 1, n, h, n, 1, lane);              // a' h
                dare_mm(mfma, T2, n, n, n, W, n, 1, T1, n, 1, lane);            // a' h W^-1 a
                double chg = 0.0, big = 0.0;
                for (int e = lane; e < nn; e += 64) {
                    const int i = e / n, j = e - i * n;
                    const double d = 0.5 * (T2[e] + T2[j * n + i]);
                    h[e] += d;
                    bad |= not_finite(h[e]);
                    chg = fmax(chg, fabs(d)); big = fmax(big, fabs(h[e]));
                }
                dare_sync();
                dare_mm(mfma, W, n, n, n, a, n, 1, T1, n, 1, lane);             // a+ = a W^-1 a: the buffers change roles
                { double *t = a; a = W; W = t; }
                for (int e = lane; e < nn; e += 64) bad |= not_finite(a[e]);
                if (wave_or(bad)) { flag = 3; break; }
                chg = wave_max(chg); big = wave_max(big);
                if (chg <= 0x1p-52 * big) { flag = 0; break; }
            }
        }
        if (!flag && gain) {
            // K = (R + B'XB)^-1 B'X A: Y = B'X, S = R + Y B, Z <- Y A (B' is not needed behind S), solved by S's Cholesky factor
            for (int e = lane; e < nn; e += 64) { const int i = e / n, j = e - i * n; W[e] = est ? A[i * n + j] : A[j * n + i]; }
            dare_mm(mfma, Y, m, n, n, Z, n, 1, h, n, 1, lane);
            dare_mm(mfma, S, m, m, n, Y, n, 1, Z, 1, n, lane);
            for (int e = lane; e < m * m; e += 64) {
                const int i = e / m, j = e - i * m;
                if (j <= i) { const double v = 0.5 * (S[i * m + j] + S[j * m + i]) + 0.5 * (R[i * m + j] + R[j * m + i]); S[i * m + j] = v; S[j * m + i] = v; }
            }
            dare_sync();
            dare_mm(mfma, Z, m, n, n, Y, n, 1, W, n, 1, lane);
            if (!dare_chol(S, m, lane)) flag = 3;
            else {
                dare_chol_solve(S, m, Z, n, true, lane);
                int bad = 0;
                for (int e = lane; e < m * n; e += 64) bad |= not_finite(Z[e]);
                if (wave_or(bad)) flag = 3;
            }
        }
        const double nan = __builtin_nan("");
        for (int e = lane; e < nn; e += 64) { const int i = e / n, j = e - i * n; Xg[(size_t)b * nn + (size_t)j * n + i] = flag ? nan : h[e]; }
        if (gain)
            for (int e = lane; e < m * n; e += 64) {          // K(r, c): column-major [m x n] in the control form; L = K', column-major [n x m]
                const int r = e / n, c = e - r * n;
                gain[(size_t)b * m * n + (est ? (size_t)r * n + c : (size_t)c * m + r)] = flag ? nan : Z[e];
            }
        if (lane == 0) {
            if (flags) flags[b] = flag;
            if (iterations) iterations[b] = it;
        }
        dare_sync();
    }
}

}  // namespace

// product: 0 the form of the size class, 1 lanes over the entries, 2 the matrix pipe
int dare_launch(int form, int n, int m, int batch, const double *A, const double *BorC, const double *Q, const double *R, int q_per_instance,
                int r_per_instance, double *X, double *gain, int *flags, int *iterations, int product, void *stream)
{
    if (n < 1 || m < 1 || n > kDareMaxN || m > kDareMaxN) return -2;
    const size_t lds = ((size_t)6 * n * n + (size_t)m * m + (size_t)2 * m * n) * sizeof(double);
    const bool mfma = product == 2 || (product == 0 && n >= kDareMfmaMinN);
    const int blocks = batch < 4096 ? batch : 4096;
    hipLaunchKernelGGL(dare_sda, dim3(blocks), dim3(64), lds, reinterpret_cast<hipStream_t>(stream), form, n, m, batch, mfma, A, BorC, Q, R,
                       q_per_instance ? 1 : 0, r_per_instance ? 1 : 0, X, gain, flags, iterations);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mpcx
