// Parameter sensitivities of a solved batch: the gradient of a loss on cmd / the input sequence with respect to the three weight
// matrices of the objective and to every bound of the QP.
//
// Notation of lmpc_sens.hip: on the working set A, w = t0 - Y[:, A] lambda, S = Y[A, A], and the leading nz x nz block of Y is H^-1.
// For a cotangent p on w
//     mu = S^-1 Y[A, 0:nz] p,     q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu      ( = H^-1 (p - N_A' mu): a direction that keeps every working row fixed )
// A bound of a working row r gets mu_r, on the side whose bit is set.  H and f are linear in the weights, every entry a rank-one term, so
//     dL / dOWeight[j, i]      = - dy_{i+1}[j]  (y_{i+1}[j] - yref_i[j])            dy = Cq q, Cq = d (outputs of the steps 1 .. ph) / d w
//     dL / dUWeight[j, i]      = - dv_{i+1}[j]  (v_{i+1}[j] - uref_i[j])            dv_i = q[blk[i] nu + .], dv_0 = 0 (lastU is data)
//     dL / dDeltaUWeight[j, i] = - (dv_{i+1} - dv_i)[j] (v_{i+1} - v_i - duref_{max(i-1, 0)})[j]
// with y, v the solve's own seq_output, seq_input (row i of seq_input is v_{min(i + 1, ph)}) and v_0 = lastU.
// The plan is lmpc_sensitivity's: a workgroup takes sixteen instances, one seed each; one wavefront per instance decodes the working set, factors S
// in LDS and forms q; then Cq Q, Q the sixteen q as one column tile, goes through the f64 matrix pipe, the wavefronts splitting the row tiles.
// reduce: a workgroup adds its instances in instance order into its own row of a partials buffer, lmpc_sens_reduce adds the rows in workgroup
// order -- no floating-point atomics, the same bits on every launch.
// The per-instance part (working set, factor, solve, q), the tile product and the reduce kernel are lmpc_sens_common.hpp's, shared with the other
// sensitivity kernels.
#include "lmpc_sens_common.hpp"

namespace mpcx {

namespace {

constexpr int kParamIpg = 16;      // instances of a workgroup: one MFMA column tile

struct LmpcParamDev {
    int batch, reduce;
    int cap;                      // rows of S a wavefront's LDS slice holds
    int rows16, G;                // rows of Cq padded to the row tile; k-step groups per row tile of its packed copy
    int m_rows;                   // rows the active words name: entries of d_lower / d_upper per instance
    const uint32_t *al, *au;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    const double *u0, *seq_output, *seq_input;
    const double *yref; long yref_bs, yref_ks;
    const double *uref; long uref_bs, uref_ks;
    const double *duref; long duref_bs, duref_ks;
    double *d_ow, *d_uw, *d_duw, *d_lo, *d_up;
    int32_t *flags, *n_used;
    double *part;                 // [groups x plen]: weights | lower | upper | instances that contributed
    const double *Cqp;            // Cq [rows16 x nz], packed
};

__host__ __device__ inline size_t param_plen(int ny, int nu, int ph, int m_rows) { return (size_t)(ny + 2 * nu) * ph + 2 * (size_t)m_rows + 1; }
// cotangents and directions as MFMA B operands | Cq Q | flags of the group's instances and the rows of each wavefront's working set (ints)
__host__ __device__ inline size_t param_shared_len(int nz16, int rows16) { return 2 * (size_t)(nz16 / 4) * 64 + (size_t)kParamIpg * rows16 + 16; }
// a wavefront's slice: S (packed lower triangle) | its original diagonal | the right-hand side | unified indices and output slots (ints)
__host__ __device__ inline size_t param_wave_len(int cap) { return (size_t)cap * (cap + 1) / 2 + 3 * (size_t)cap; }

__global__ __launch_bounds__(256) void lmpc_param_sensitivity(const LmpcDev *__restrict__ Mp, const LmpcParamDev Pd)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
    const int j16 = lane & 15, kq = lane >> 4;
    const int nu = M.nu, ny = M.ny, nz = M.nz, mg = M.mg, ph = M.ph;
    const int ldz = M.ldz, ldy = M.ldy, aw = M.active_words;
    const int nz4 = M.nz16 >> 2, cap = Pd.cap, rows16 = Pd.rows16, m_rows = Pd.m_rows, reduce = Pd.reduce;
    const int nE = (ny + 2 * nu) * ph;
    const size_t plen = param_plen(ny, nu, ph, m_rows);
    const bool bounds = Pd.d_lo || Pd.d_up;                       // reduced form: the bound rows of the partials are left alone when nobody asks for them
    double *Bp = smem;                                            // [nz4][64]  the cotangents as an MFMA B operand (column = instance)
    double *Qp = Bp + (size_t)nz4 * 64;                           // [nz4][64]  the directions q, likewise
    double *DY = Qp + (size_t)nz4 * 64;                           // [16][rows16]  Cq q of every instance
    int *flg = reinterpret_cast<int *>(DY + (size_t)kParamIpg * rows16);      // [16] flag of each instance, -1 beyond the batch
    int *wn = flg + kParamIpg;                                    // [W] rows each wavefront's instance of the round contributes
    double *slices = DY + (size_t)kParamIpg * rows16 + 16;
    auto S_of = [&](int w) -> double * { return slices + (size_t)w * param_wave_len(cap); };
    auto V_of = [&](int w) -> double * { return S_of(w) + (size_t)cap * (cap + 1) / 2 + cap; };
    auto tgt_of = [&](int w) -> int * { return reinterpret_cast<int *>(V_of(w) + cap) + cap; };
    double *S = S_of(wave), *dg = S + (size_t)cap * (cap + 1) / 2, *V = V_of(wave);
    int *idx = reinterpret_cast<int *>(V + cap), *tgt = idx + cap;
    const gdp Y = GP(Y);
    const gip blk = GP(blk);
    const double qnan = __builtin_nan("");
    const gdp yr = gl(Pd.yref), ur = gl(Pd.uref), dr = gl(Pd.duref);

    for (int g0 = blockIdx.x; g0 * kParamIpg < Pd.batch; g0 += gridDim.x) {
        const int b0 = g0 * kParamIpg;
        double *part = Pd.part ? Pd.part + (size_t)g0 * plen : nullptr;
        for (int t = tid; t < 2 * nz4 * 64; t += blockDim.x) Bp[t] = 0.0;
        // the bounds' entries start at zero: a row outside the working set has no gradient
        if (reduce) { for (int t = nE + tid; bounds && t < (int)plen - 1; t += blockDim.x) glw(part)[t] = 0.0; }
        else
            for (int t = tid; t < kParamIpg * m_rows; t += blockDim.x) {
                const int il = t / m_rows, r = t - il * m_rows;
                if (b0 + il >= Pd.batch) break;
                if (Pd.d_lo) glw(Pd.d_lo)[(size_t)(b0 + il) * m_rows + r] = 0.0;
                if (Pd.d_up) glw(Pd.d_up)[(size_t)(b0 + il) * m_rows + r] = 0.0;
            }
        __syncthreads();
        // ---- the cotangents on w: the seeds on cmd and on the input sequence scattered through blk, as lmpc_sensitivity's VJP mode
        for (int t = tid; t < kParamIpg * nz; t += blockDim.x) {
            const int il = t / nz, q = t - il * nz, b = b0 + il;
            if (b >= Pd.batch) continue;
            sens_opnd(Bp, il, q) = sens_seed(Pd.seed_cmd, Pd.seed_input, blk, nu, ph, b, q);
        }
        __syncthreads();

        // ---- per instance, one wavefront each, W instances a round
        for (int r0 = 0; r0 < kParamIpg; r0 += W) {
            const int il = r0 + wave, b = b0 + il;
            const bool valid = b < Pd.batch;
            int flag = 0, n = 0;
            auto cot = [&](int q) { return sens_opnd(Bp, il, q); };      // the instance's cotangent
            if (valid) {
                flag = (Pd.status && gl(Pd.status)[b] != 0) ? 1 : 0;
                if (!flag) {
                    // (tgt: the bound that takes the row's mu, the upper one where both bits are set)
                    n = sens_working_set(M, gl(Pd.al) + (size_t)b * aw, gl(Pd.au) + (size_t)b * aw, aw, nz, mg, ldz, cap, lane, idx, tgt);
                    if (n > cap) flag = 3;
                }
            }
            wave_sync();
            if (valid && !flag && n > 0) {
                // right-hand side Y[A, 0:nz] p, a row per lane
                for (int i = lane; i < n; i += 64) V[i] = sens_rhs(Y, ldy, nz, idx[i], cot);
                if (!sens_factor(Y, ldy, idx, n, lane, S, dg)) flag = 2;
                else sens_chol_solve(S, V, n, lane);
            }
            if (valid && !flag) {
                // q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu, an element per lane (Y is symmetric: column t read along its rows)
                for (int t = lane; t < nz; t += 64) sens_opnd(Qp, il, t) = sens_direction(Y, ldy, nz, t, cot, idx, V, n);
            }
            if (valid && !reduce) {
                // the bounds of this instance: mu on the side whose bit is set; NaN everywhere for a flagged one
                if (flag) {
                    for (int r = lane; r < m_rows; r += 64) {
                        if (Pd.d_lo) glw(Pd.d_lo)[(size_t)b * m_rows + r] = qnan;
                        if (Pd.d_up) glw(Pd.d_up)[(size_t)b * m_rows + r] = qnan;
                    }
                } else
                    for (int i = lane; i < n; i += 64) {
                        const int row = tgt[i] >> 1;
                        double *dst = (tgt[i] & 1) ? Pd.d_up : Pd.d_lo;
                        if (dst && row < m_rows) glw(dst)[(size_t)b * m_rows + row] = V[i];
                    }
            }
            if (valid && Pd.flags && lane == 0) glw(Pd.flags)[b] = flag;
            if (lane == 0) { flg[il] = valid ? flag : -1; wn[wave] = (valid && !flag) ? n : 0; }
            __syncthreads();
            if (reduce && bounds) {
                // the round's instances in instance order; within one, every working row has a slot of its own
                for (int w = 0; w < W; ++w) {
                    const double *Vw = V_of(w);
                    const int *tw = tgt_of(w);
                    for (int i = tid; i < wn[w]; i += blockDim.x) {
                        const int row = tw[i] >> 1;
                        if (row < m_rows) glw(part)[nE + (size_t)(tw[i] & 1) * m_rows + row] += Vw[i];
                    }
                    __syncthreads();
                }
            }
        }

        // ---- Cq Q: the row tiles over the wavefronts
        const int ntile = rows16 >> 4;
        for (int t = wave; t < ntile; t += W) {
            const v4d acc = sens_mfma_tile(gl(Pd.Cqp), t, Pd.G, nz4, Qp, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) DY[(size_t)j16 * rows16 + 16 * t + 4 * r + kq] = acc[r];
        }
        __syncthreads();

        // ---- the weights: an entry per thread, the instances in order
        for (int t = tid; t < nE; t += blockDim.x) {
            const int kind = t < ny * ph ? 0 : (t < (ny + nu) * ph ? 1 : 2);
            const int tt = t - (kind == 0 ? 0 : (kind == 1 ? ny * ph : (ny + nu) * ph));
            const int rows = kind == 0 ? ny : nu, i = tt / rows, j = tt - i * rows;      // [rows x ph] column-major: the setters' layout
            double *out = kind == 0 ? Pd.d_ow : (kind == 1 ? Pd.d_uw : Pd.d_duw);
            const int qn = blk[i + 1] * nu + j, qp = i > 0 ? blk[i] * nu + j : -1;
            double sum = 0.0;
            for (int il = 0; il < kParamIpg; ++il) {
                const int f = flg[il], b = b0 + il;
                if (f < 0) break;
                double c = qnan;
                if (f == 0) {
                    if (kind == 0) {
                        const double e = gl(Pd.seq_output)[((size_t)b * (ph + 1) + i + 1) * ny + j] - ref_at(yr, Pd.yref_bs, Pd.yref_ks, b, i, j);
                        c = -DY[(size_t)il * rows16 + i * ny + j] * e;
                    } else {
                        const double vn = gl(Pd.seq_input)[((size_t)b * (ph + 1) + i) * nu + j];
                        if (kind == 1) c = -sens_opnd(Qp, il, qn) * (vn - ref_at(ur, Pd.uref_bs, Pd.uref_ks, b, i, j));
                        else {
                            const double vp = i > 0 ? gl(Pd.seq_input)[((size_t)b * (ph + 1) + i - 1) * nu + j] : gl(Pd.u0)[(size_t)b * nu + j];
                            const double dq = sens_opnd(Qp, il, qn) - (qp >= 0 ? sens_opnd(Qp, il, qp) : 0.0);
                            c = -dq * (vn - vp - ref_at(dr, Pd.duref_bs, Pd.duref_ks, b, i > 0 ? i - 1 : 0, j));
                        }
                    }
                }
                if (reduce) { if (f == 0) sum += c; }
                else if (out) glw(out)[(size_t)b * rows * ph + tt] = c;
            }
            if (reduce) glw(part)[t] = sum;
        }
        if (reduce && tid == 0) {
            int cnt = 0;
            for (int il = 0; il < kParamIpg; ++il) cnt += flg[il] == 0;
            glw(part)[plen - 1] = (double)cnt;
        }
        __syncthreads();
    }
}

}  // namespace

// Cq = d (outputs of the steps 1 .. ph) / d w as the kernel's A operand source: [rows16 x nz] column-major, row (i - 1) ny + a = output a of step i,
// by rolling the model out from x0 = 0 on the unit vectors of w (no exogenous input: the linear part).  A, B, C column-major
size_t lmpc_param_sens_cq(int nx, int nu, int ny, int ph, int nz, const double *A, const double *B, const double *C, const int *blk, double *out)
{
    const int rows16 = (ny * ph + 15) / 16 * 16;
    const size_t len = (size_t)rows16 * nz;
    if (!out) return len;
    for (int q = 0; q < nz; ++q) {
        double *col = out + (size_t)q * rows16;
        for (int r = 0; r < rows16; ++r) col[r] = 0.0;
        sens_unit_rollout(nx, nu, ph, q, A, B, blk, [&](int i, const double *x) {
            for (int a = 0; a < ny; ++a) {
                double s = 0.0;
                for (int c = 0; c < nx; ++c) s += C[a + (size_t)c * ny] * x[c];
                col[(i - 1) * ny + a] = s;
            }
        });
    }
    return len;
}

size_t lmpc_param_sens_partials(const LmpcDev &m, int batch)
{
    return (size_t)((batch + kParamIpg - 1) / kParamIpg) * param_plen(m.ny, m.nu, m.ph, m.m_ref);
}

int lmpc_param_sens_launch(const LmpcDev &m, const LmpcDev *m_dev, const double *Cqp, const LmpcParamSensArgs &a, void *stream)
{
    LmpcParamDev s{};
    s.batch = a.batch; s.reduce = a.reduce ? 1 : 0;
    s.rows16 = (m.ny * m.ph + 15) / 16 * 16; s.G = (m.nz + 15) / 16; s.m_rows = m.m_ref;
    s.al = a.active_lower; s.au = a.active_upper; s.status = a.status;
    s.seed_cmd = a.seed_cmd; s.seed_input = a.seed_input;
    s.u0 = a.u0; s.seq_output = a.seq_output; s.seq_input = a.seq_input;
    s.yref = a.yref; s.yref_bs = a.yref_bs; s.yref_ks = a.yref_ks;
    s.uref = a.uref; s.uref_bs = a.uref_bs; s.uref_ks = a.uref_ks;
    s.duref = a.duref; s.duref_bs = a.duref_bs; s.duref_ks = a.duref_ks;
    s.d_ow = a.d_oweight; s.d_uw = a.d_uweight; s.d_duw = a.d_duweight; s.d_lo = a.d_lower; s.d_up = a.d_upper;
    s.flags = a.flags; s.n_used = a.n_used; s.part = a.reduce ? a.partials : nullptr; s.Cqp = Cqp;
    if (a.reduce && !a.partials) return -3;
    // the wavefronts' slices beside the shared operands
    const size_t shared = param_shared_len(m.nz16, s.rows16);
    const SensLdsPlan plan = sens_lds_plan(m, 4, [&](int waves, int cap) { return shared + waves * param_wave_len(cap); });
    if (plan.cap <= 0) return -2;
    s.cap = plan.cap;
    static LmpcLdsCache configured;
    if (lmpc_raise_dynamic_lds(configured, {reinterpret_cast<const void *>(lmpc_param_sensitivity)}, plan.bytes) != 0) return -3;
    const int groups = (a.batch + kParamIpg - 1) / kParamIpg;
    const int blocks = groups > 65536 ? 65536 : groups;
    hipLaunchKernelGGL(lmpc_param_sensitivity, dim3(blocks), dim3(64 * plan.waves), plan.bytes, static_cast<hipStream_t>(stream), m_dev, s);
    if (hipGetLastError() != hipSuccess) return -3;
    if (!a.reduce) return 0;
    const size_t eo = (size_t)m.ny * m.ph, eu = eo + (size_t)m.nu * m.ph, ed = eu + (size_t)m.nu * m.ph, mr = (size_t)m.m_ref;      // param_plen's order
    return sens_reduce_launch(SensReduce{s.part, param_plen(m.ny, m.nu, m.ph, m.m_ref), {eo, eu, ed, ed + mr, ed + 2 * mr}, {s.d_ow, s.d_uw, s.d_duw, s.d_lo, s.d_up}, s.n_used, groups}, stream);
}

}  // namespace mpcx
