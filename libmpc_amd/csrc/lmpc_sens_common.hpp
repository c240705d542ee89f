// What the four sensitivity kernels (lmpc_sens.hip, lmpc_bank_sens.hip, lmpc_param_sens.hip, lmpc_model_sens.hip) have in
// common, each piece once: the working set decoded from the active words, S = Y[A, A] gathered and factored, the solve on that factor, the seeds
// scattered into a cotangent on w, the two products with Y, the MFMA row-tile product, the ordered reduce kernel, and on the host the LDS plan and
// the model's roll-out on the unit vectors of w.  The device pieces are free functions of one wavefront that take `lane` and LDS pointers.
// Everything lives in an anonymous namespace: each unit gets its own copy, the reduce kernel included.
#pragma once
#include "lmpc_kernel_common.hpp"

#include <vector>

namespace mpcx {

namespace {

// a pivot below this fraction of the row's own diagonal entry of S: the working set is dependent (flag 2)
constexpr double kSensPivotTol = 1e-11;

__device__ __forceinline__ v4d ld4(gdp p) { return *reinterpret_cast<const v4d MPCX_GAS *>(p); }
// element q of column c (< 16) of an MFMA B operand [nz4][64]
__device__ __forceinline__ double &sens_opnd(double *P, int c, int q) { return P[(size_t)(q >> 2) * 64 + 16 * (q & 3) + c]; }

// The working set of an instance from its active words wl, wu by ballot compaction: a variable is in A when any of its reference rows has a bit, a
// general row when bit g_refrow[r] is set.  Returns the number of rows; only the first `cap` are stored, as unified indices in idx.  With a tgt, the
// slot 2 row + (upper ? 1 : 0) of the bound that takes the row's multiplier besides: of several reference rows on one variable the lowest-numbered
// one with a bit, and the upper side where both bits are set
__device__ inline int sens_working_set(const LmpcDev &M, const uint32_t MPCX_GAS *wl, const uint32_t MPCX_GAS *wu, int aw, int nz, int mg, int ldz,
                                       int cap, int lane, int *idx, int *tgt)
{
    // 0: no bit, 1: the lower bound's, 2: the upper bound's
    auto side = [&](int rr) -> int {
        if (rr < 0 || (rr >> 5) >= aw) return 0;
        if ((wu[rr >> 5] >> (rr & 31)) & 1u) return 2;
        return (int)((wl[rr >> 5] >> (rr & 31)) & 1u);
    };
    int n = 0;
    for (int base = 0; base < nz + mg; base += 64) {
        const int e = base + lane;
        int slot = -1;
        if (e < nz) {
            for (int p = GP(boxrow_ptr)[e]; p < GP(boxrow_ptr)[e + 1]; ++p) {
                const int rr = GP(boxrow_ref)[p], sd = side(rr);
                if (sd && (slot < 0 || rr < (slot >> 1))) slot = 2 * rr + (sd - 1);
            }
        } else if (e < nz + mg) {
            const int rr = GP(g_refrow)[e - nz], sd = side(rr);
            if (sd) slot = 2 * rr + (sd - 1);
        }
        const bool in = slot >= 0;
        const unsigned long long mask = __ballot(in);
        const int pos = n + __popcll(mask & ((1ull << lane) - 1ull));
        if (in && pos < cap) { idx[pos] = e < nz ? e : ldz + (e - nz); if (tgt) tgt[pos] = slot; }
        n += __popcll(mask);
    }
    return n;
}

// S = Y[A, A] gathered as a packed lower triangle, its diagonal kept in dg, and factored in place by a left-looking Cholesky, a row per lane.
// false: a pivot at or below kSensPivotTol of the row's own diagonal entry
__device__ inline bool sens_factor(gdp Y, int ldy, const int *idx, int n, int lane, double *S, double *dg)
{
    for (int t = lane; t < n * n; t += 64) {              // (the square is walked and its lower triangle kept: independent loads, all in flight)
        const int i = t / n, j = t - i * n;
        if (j > i) continue;
        const double v = Y[(size_t)idx[j] * ldy + idx[i]];
        if (j == i) dg[i] = v;
        S[(size_t)i * (i + 1) / 2 + j] = v;
    }
    wave_sync();
    for (int k = 0; k < n; ++k) {
        const double *Lk = S + (size_t)k * (k + 1) / 2;
        for (int i = k + lane; i < n; i += 64) {
            double *Li = S + (size_t)i * (i + 1) / 2;
            double s = Li[k];
            for (int j = 0; j < k; ++j) s = fma(-Li[j], Lk[j], s);      // (not unrolled: by four it costs lmpc_model_sensitivity 1.3 %)
            Li[k] = s;
        }
        wave_sync();
        const double d = Lk[k];
        if (!(d > kSensPivotTol * dg[k])) return false;
        const double sd = sqrt(d), rd = 1.0 / sd;
        wave_sync();
        for (int i = k + lane; i < n; i += 64) { double *Li = S + (size_t)i * (i + 1) / 2; Li[k] = i == k ? sd : Li[k] * rd; }
        wave_sync();
    }
    return true;
}

// L L' x = v on the factor in S, in place
__device__ inline void sens_chol_solve(const double *S, double *V, int n, int lane)
{
    for (int k = 0; k < n; ++k) {
        if (lane == 0) V[k] /= S[(size_t)k * (k + 1) / 2 + k];
        wave_sync();
        for (int i = k + 1 + lane; i < n; i += 64) V[i] = fma(-S[(size_t)i * (i + 1) / 2 + k], V[k], V[i]);
        wave_sync();
    }
    for (int k = n - 1; k >= 0; --k) {
        const double *Lk = S + (size_t)k * (k + 1) / 2;
        if (lane == 0) V[k] /= Lk[k];
        wave_sync();
        for (int i = lane; i < k; i += 64) V[i] = fma(-Lk[i], V[k], V[i]);
        wave_sync();
    }
}

// element q of instance b's cotangent on w: the seed on cmd and the seeds on the input sequence scattered through blk (in HBM or in LDS)
template <class Blk>
__device__ inline double sens_seed(const double *seed_cmd, const double *seed_input, Blk blk, int nu, int ph, int b, int q)
{
    const int bq = q / nu, jq = q - bq * nu;
    double v = 0.0;
    if (seed_cmd && bq == blk[1]) v = gl(seed_cmd)[(size_t)b * nu + jq];
    if (seed_input)              // row i of the sequence is v_{min(i + 1, ph)} (OptSequence)
        for (int i = 0; i <= ph; ++i)
            if (blk[i + 1 <= ph ? i + 1 : ph] == bq) v += gl(seed_input)[((size_t)b * (ph + 1) + i) * nu + jq];
    return v;
}

// row qi of Y[:, 0:nz] p, p(q) the cotangent's element q where the caller keeps it (Y is symmetric: row qi read along column q)
template <class Cot>
__device__ inline double sens_rhs(gdp Y, int ldy, int nz, int qi, Cot p)
{
    double s = 0.0;
    for (int q = 0; q < nz; ++q) {
        const double pv = p(q);
        if (pv != 0.0) s = fma(Y[(size_t)q * ldy + qi], pv, s);
    }
    return s;
}

// element t of the direction q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu
template <class Cot>
__device__ inline double sens_direction(gdp Y, int ldy, int nz, int t, Cot p, const int *idx, const double *mu, int n)
{
    double s = sens_rhs(Y, ldy, nz, t, p);
    for (int i = 0; i < n; ++i) s = fma(-Y[(size_t)idx[i] * ldy + t], mu[i], s);
    return s;
}

// row tile t of a packed A operand (lmpc_pack_mfma_tiles, G k-step groups per row tile) times the B operand Bc [nz4][64] in LDS, on the f64 matrix
// pipe (v_mfma_f64_16x16x4_f64): element r of the result is row 16 t + 4 r + (lane >> 4), column lane & 15
__device__ __forceinline__ v4d sens_mfma_tile(gdp Ap, int t, int G, int nz4, const double *Bc, int lane)
{
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g) {
        const v4d a = ld4(Ap + (((size_t)t * G + g) * 64 + lane) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kb = 4 * g + e;
            if (kb < nz4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], Bc[kb * 64 + lane], acc, 0, 0, 0);
        }
    }
    return acc;
}

// The reduced forms: a workgroup adds its instances in instance order into its own row of a partials buffer [groups x plen], this kernel adds the
// rows in workgroup order, an entry per thread -- no floating-point atomics, the same bits on every launch.  Entries [end[k - 1], end[k]) of a row
// go to dst[k] (a null one is skipped; a segment that is not used ends where the one before it does), the last entry counts the instances that
// contributed and goes to n_used.  (Kernel and launch are templates on a tag so that only a unit that launches the kernel compiles it.)
constexpr int kSensReduceSegs = 5;
struct SensReduce {
    const double *part;
    size_t plen, end[kSensReduceSegs];
    double *dst[kSensReduceSegs];
    int32_t *n_used;
    int groups;
};

template <int Tag>
__global__ __launch_bounds__(256) void lmpc_sens_reduce(const SensReduce R)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R.plen) return;
    double *dst = nullptr;
    size_t first = 0;
#pragma unroll
    for (int k = kSensReduceSegs - 1; k >= 0; --k)
        if (t < R.end[k]) { dst = R.dst[k]; first = k > 0 ? R.end[k - 1] : 0; }
    const bool count = t == R.plen - 1;
    if (count ? !R.n_used : !dst) return;
    double s = 0.0;
    int g = 0;
    for (; g + 8 <= R.groups; g += 8) {           // eight loads in flight, the additions in workgroup order all the same
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = gl(R.part)[(size_t)(g + u) * R.plen + t];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; g < R.groups; ++g) s += gl(R.part)[(size_t)g * R.plen + t];
    if (count) glw(R.n_used)[0] = (int32_t)s;
    else glw(dst)[t - first] = s;
}

template <int Tag = 0>
inline int sens_reduce_launch(const SensReduce &r, void *stream)
{
    hipLaunchKernelGGL(lmpc_sens_reduce<Tag>, dim3((unsigned)((r.plen + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), r);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The LDS plan of a sensitivity launch, total(waves, cap) the doubles a workgroup of `waves` wavefronts needs for working sets of up to cap rows:
// every wavefront's slice holds the largest working set there can be (ws_limit) where `waves`, or half, a quarter ... of them, fit in a CU's LDS;
// otherwise one wavefront with the largest capacity that fits, and larger sets get flag 3.  cap <= 0: not even one row fits
struct SensLdsPlan { int waves, cap; size_t bytes; };
template <class Total>
inline SensLdsPlan sens_lds_plan(const LmpcDev &m, int waves, Total total)
{
    const size_t limit = lmpc_lds_limit() / sizeof(double);
    const int want = ws_limit(m.nz, m.mg, m.n_soft) > 1 ? ws_limit(m.nz, m.mg, m.n_soft) : 1;
    while (waves > 1 && total(waves, want) > limit) waves >>= 1;
    int cap = want;
    while (cap > 0 && total(waves, cap) > limit) --cap;
    return SensLdsPlan{waves, cap, cap > 0 ? total(waves, cap) * sizeof(double) : 0};
}

// The model rolled out from x0 = 0 on unit vector q of w (no exogenous input: the linear part), A, B column-major: each(i, x) sees the state of
// the steps i = 1 .. ph
template <class Each>
inline void sens_unit_rollout(int nx, int nu, int ph, int q, const double *A, const double *B, const int *blk, Each each)
{
    std::vector<double> x(nx, 0.0), xn(nx);
    for (int i = 1; i <= ph; ++i) {
        for (int a = 0; a < nx; ++a) {
            double s = 0.0;
            for (int c = 0; c < nx; ++c) s += A[a + (size_t)c * nx] * x[c];
            if (blk[i] == q / nu) s += B[a + (size_t)(q % nu) * nx];
            xn[a] = s;
        }
        x.swap(xn);
        each(i, x.data());
    }
}

}  // namespace

}  // namespace mpcx
