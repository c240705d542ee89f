// Sensitivities of a solved batch: vector-Jacobian products of the decision vector w with respect to vin = [x0 | lastU | yref].
//
// On a working set A the solve computes lambda = S^-1 (N_A t0 - b_A), w = t0 - Y[:, A] lambda with S = Y[A, A] (the device's Y
// carries a soft row's 1 / weight on its diagonal already: LmpcController::condense).
// t0 and N t0 are the first ldy rows of the composed map MF1 times vin; the bounds of a box row do not depend on vin, those of a general row
// are lg0 - goff and ug0 - goff (lmpc_assemble_mfma), goff being MF1's next ldg rows times vin.  So for a cotangent p on w
//     g = T0' p - (MF1[A, :] + GOFF[A, :])' mu,   mu = S^-1 Y[A, 0:nz] p      (GOFF[q, :] = 0 for a box row)
// The first product does not depend on the working set: sixteen (instance, seed) columns share the operand T0' and go through the f64 matrix
// pipe (v_mfma_f64_16x16x4_f64) with the packed operands of lmpc_pack_mfma_tiles, the wavefronts of a workgroup splitting the tiles.  The rest
// is per instance, one wavefront each: decode the working set from the active bits, gather S into LDS (packed lower triangle), factor it by
// Cholesky with a relative pivot test, solve for the seeds, gather the rows of MF1.  The decode, the factor, the seed scatter and the tile product
// are lmpc_sens_common.hpp's, shared with the other sensitivity kernels.
#include "lmpc_sens_common.hpp"

namespace mpcx {

namespace {

struct LmpcSensDev {
    int batch, R, jac;            // seeds per instance; jac: the nu unit seeds on cmd
    int ipg, ctiles;              // instances per workgroup, column tiles of their (instance, seed) pairs
    int cap;                      // rows of S a wavefront's LDS slice holds
    int kin16, G;                 // rows of T0' padded to the row tile; k-step groups per row tile of its packed copy
    const uint32_t *al, *au;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    double *d_x0, *d_u0, *d_yref;
    int32_t *flags;
    const double *T0p;            // T0' = MF1[0:nz, :]' [kin16 x nz], packed
};

__host__ __device__ inline size_t sens_shared_len(const LmpcSensDev &s, int nz16) { return (size_t)s.ctiles * (nz16 / 4) * 64 + (size_t)s.ctiles * 16 * s.kin16; }
// a wavefront's slice: S (packed lower triangle) | its original diagonal | R right-hand sides | the working set's unified indices (ints)
__host__ __device__ inline size_t sens_wave_len(int cap, int R) { return (size_t)cap * (cap + 1) / 2 + cap + (size_t)R * cap + (cap + 2) / 2; }

__global__ __launch_bounds__(256) void lmpc_sensitivity(const LmpcDev *__restrict__ Mp, const LmpcSensDev Sd)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int j16 = lane & 15, kq = lane >> 4;
    const int nx = M.nx, nu = M.nu, ny = M.ny, nz = M.nz, mg = M.mg, ph = M.ph;
    const int ldz = M.ldz, ldy = M.ldy, rowsF = M.rowsF, aw = M.active_words;
    const int nz4 = M.nz16 >> 2, nin = nx + nu + ny;
    const int R = Sd.R, ipg = Sd.ipg, ncol = ipg * R, cap = Sd.cap, kin16 = Sd.kin16;
    double *Bp = smem;                                            // [ctiles][nz4][64]  the cotangents as MFMA B operands
    double *G0 = Bp + (size_t)Sd.ctiles * nz4 * 64;               // [ctiles * 16][kin16]  T0' p of every column
    double *mine = G0 + (size_t)Sd.ctiles * 16 * kin16 + (size_t)wave * sens_wave_len(cap, R);
    double *S = mine, *dg = S + (size_t)cap * (cap + 1) / 2, *V = dg + cap;
    int *idx = reinterpret_cast<int *>(V + (size_t)R * cap);
    const gdp Y = GP(Y), MF = GP(MF1);
    const gip blk = GP(blk);
    const double qnan = __builtin_nan("");
    // element q of column c's cotangent, where the B operands keep it
    auto pcol = [&](int c, int q) -> double & { return sens_opnd(Bp + (size_t)(c >> 4) * nz4 * 64, c & 15, q); };

    for (int g0 = blockIdx.x; g0 * ipg < Sd.batch; g0 += gridDim.x) {
        const int b0 = g0 * ipg;
        // ---- the cotangents on w: unit vectors on the first move, or the seeds on cmd and on the input sequence scattered through blk
        for (int t = threadIdx.x; t < Sd.ctiles * nz4 * 64; t += blockDim.x) Bp[t] = 0.0;
        __syncthreads();
        for (int t = threadIdx.x; t < ncol * nz; t += blockDim.x) {
            const int c = t / nz, q = t - c * nz, il = c / R, r = c - il * R, b = b0 + il;
            if (b >= Sd.batch) continue;
            pcol(c, q) = Sd.jac ? (q == blk[1] * nu + r ? 1.0 : 0.0) : sens_seed(Sd.seed_cmd, Sd.seed_input, blk, nu, ph, b, q);
        }
        __syncthreads();
        // ---- T0' P: row tiles x column tiles over the wavefronts
        const int ntile = kin16 >> 4;
        for (int item = wave; item < ntile * Sd.ctiles; item += W) {
            const int t = item % ntile, ct = item / ntile;
            const v4d acc = sens_mfma_tile(gl(Sd.T0p), t, Sd.G, nz4, Bp + (size_t)ct * nz4 * 64, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) G0[(size_t)(16 * ct + j16) * kin16 + 16 * t + 4 * r + kq] = acc[r];
        }
        __syncthreads();

        // ---- per instance, one wavefront each
        for (int il = wave; il < ipg; il += W) {
            const int b = b0 + il;
            if (b >= Sd.batch) break;
            int flag = (Sd.status && gl(Sd.status)[b] != 0) ? 1 : 0;
            int n = 0;
            if (!flag) {
                n = sens_working_set(M, gl(Sd.al) + (size_t)b * aw, gl(Sd.au) + (size_t)b * aw, aw, nz, mg, ldz, cap, lane, idx, nullptr);
                if (n > cap) flag = 3;
            }
            wave_sync();
            if (!flag && n > 0) {
                // right-hand sides Y[A, 0:nz] p, one (seed, row) pair per lane
                for (int t = lane; t < R * n; t += 64) {
                    const int r = t / n, i = t - r * n, c = il * R + r;
                    V[(size_t)r * cap + i] = sens_rhs(Y, ldy, nz, idx[i], [&](int q) { return pcol(c, q); });
                }
                if (!sens_factor(Y, ldy, idx, n, lane, S, dg)) flag = 2;
                // the R right-hand sides at once, a column scaled by the pivot's reciprocal: sens_chol_solve divides, and folding this solve into
                // it would change this kernel's last bits
                if (!flag) {
                    for (int k = 0; k < n; ++k) {                 // L y = v
                        const double rd = 1.0 / S[(size_t)k * (k + 1) / 2 + k];
                        for (int r = lane; r < R; r += 64) V[(size_t)r * cap + k] *= rd;
                        wave_sync();
                        const int m = n - k - 1;
                        for (int t = lane; t < R * m; t += 64) {
                            const int r = t / m, i = k + 1 + (t - r * m);
                            V[(size_t)r * cap + i] = fma(-S[(size_t)i * (i + 1) / 2 + k], V[(size_t)r * cap + k], V[(size_t)r * cap + i]);
                        }
                        wave_sync();
                    }
                    for (int k = n - 1; k >= 0; --k) {            // L' mu = y
                        const double *Lk = S + (size_t)k * (k + 1) / 2;
                        const double rd = 1.0 / Lk[k];
                        for (int r = lane; r < R; r += 64) V[(size_t)r * cap + k] *= rd;
                        wave_sync();
                        for (int t = lane; t < R * k; t += 64) {
                            const int r = t / k, i = t - r * k;
                            V[(size_t)r * cap + i] = fma(-Lk[i], V[(size_t)r * cap + k], V[(size_t)r * cap + i]);
                        }
                        wave_sync();
                    }
                }
            }
            // ---- g = T0' p - (MF1[A, :] + GOFF[A, :])' mu over the columns of x0, lastU, yref
            for (int t = lane; t < R * nin; t += 64) {
                const int r = t / nin, c = t - r * nin;
                const int col = c < nx ? c : (c < nx + nu ? M.nxp + (c - nx) : M.nxp + M.nup + (c - nx - nu));
                double g = qnan;
                if (!flag) {
                    g = G0[(size_t)(il * R + r) * kin16 + col];
                    const gdp mc = MF + (size_t)col * rowsF;
                    for (int i = 0; i < n; ++i) {
                        const int qi = idx[i];
                        double m = mc[qi];
                        if (qi >= ldz) m += mc[ldy + (qi - ldz)];
                        g = fma(-m, V[(size_t)r * cap + i], g);
                    }
                }
                const size_t row = (size_t)b * R + r;
                if (c < nx) { if (Sd.d_x0) glw(Sd.d_x0)[row * nx + c] = g; }
                else if (c < nx + nu) { if (Sd.d_u0) glw(Sd.d_u0)[row * nu + (c - nx)] = g; }
                else if (Sd.d_yref) glw(Sd.d_yref)[row * ny + (c - nx - nu)] = g;
            }
            if (Sd.flags && lane == 0) glw(Sd.flags)[b] = flag;
            wave_sync();
        }
        __syncthreads();
    }
}

}  // namespace

// T0' as the kernel's A operand: src [kin16 x nz] column-major, src(k, q) = MF1(q, k)
size_t lmpc_sens_operand(int nz, int kin, int rowsF, const double *MF1, double *out)
{
    const int kin16 = (kin + 15) / 16 * 16;
    const size_t len = lmpc_packed_len(kin16, nz);
    if (!out) return len;
    std::vector<double> src((size_t)kin16 * nz, 0.0);
    for (int q = 0; q < nz; ++q)
        for (int k = 0; k < kin; ++k) src[(size_t)q * kin16 + k] = MF1[(size_t)k * rowsF + q];
    lmpc_pack_mfma_tiles(src.data(), kin16, nz, out);
    return len;
}

int lmpc_sens_launch(const LmpcDev &m, const LmpcDev *m_dev, const double *T0p, const LmpcSensArgs &a, void *stream)
{
    LmpcSensDev s{};
    s.batch = a.batch; s.jac = a.jacobian ? 1 : 0; s.R = a.jacobian ? m.nu : 1;
    s.ipg = 16 / s.R > 1 ? 16 / s.R : 1;
    s.ctiles = (s.ipg * s.R + 15) / 16;
    s.kin16 = (m.kin + 15) / 16 * 16; s.G = (m.nz + 15) / 16;
    s.al = a.active_lower; s.au = a.active_upper; s.status = a.status;
    s.seed_cmd = a.seed_cmd; s.seed_input = a.seed_input;
    s.d_x0 = a.d_x0; s.d_u0 = a.d_u0; s.d_yref = a.d_yref; s.flags = a.flags; s.T0p = T0p;
    // the wavefronts' slices beside the shared operands, no more wavefronts than instances
    const size_t shared = sens_shared_len(s, m.nz16);
    const SensLdsPlan plan = sens_lds_plan(m, s.ipg < 4 ? (s.ipg < 2 ? 1 : 2) : 4, [&](int waves, int cap) { return shared + waves * sens_wave_len(cap, s.R); });
    if (plan.cap <= 0) return -2;
    s.cap = plan.cap;
    static LmpcLdsCache configured;
    if (lmpc_raise_dynamic_lds(configured, {reinterpret_cast<const void *>(lmpc_sensitivity)}, plan.bytes) != 0) return -3;
    int blocks = (a.batch + s.ipg - 1) / s.ipg;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(lmpc_sensitivity, dim3(blocks), dim3(64 * plan.waves), plan.bytes, static_cast<hipStream_t>(stream), m_dev, s);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mpcx
