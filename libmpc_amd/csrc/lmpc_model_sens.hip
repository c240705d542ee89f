// Model sensitivities of a solved batch: the gradient of a loss on cmd / the input sequence with respect to every entry of the
// model's matrices A, B, C, Bd and Dd, on the active set each instance was solved on.
//
// Notation of lmpc_sens.hip and lmpc_param_sens.hip: on the working set A, S = Y[A, A], and for a cotangent p on w
//     mu = S^-1 Y[A, 0:nz] p,     q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu.
// Along the trajectory (v_i = u_{i-1}, v_0 = lastU; x_i = A x_{i-1} + B v_i + Bd d_{i-1}, y_i = C x_i + Dd d_{i-1}) the response to q is
//     dv_i = q[blk[i] nu + .],    dx_0 = 0, dx_i = A dx_{i-1} + B dv_i  ( = Xq q, Xq = d (x_1 .. x_ph) / d w ),    dy_i = C dx_i
// and, with lambda the optimum's multipliers on A,
//     o_i   = W_i (y_i - yref_{i-1}) + sum over the output rows r of step i: lambda_r e_comp
//     g_i   = C' o_i + state rows: lambda_r e_comp + scalar rows: lambda_r sX + linear rows: lambda_r Fx[c, :] + [i = ph] P (x_ph - x_T)
//     pi_ph = g_ph,   pi_i = g_i + A' pi_{i+1};        do_i, eta_i the same with (dy_i, dx_i, mu_r) in place of (y_i - yref, x_i - x_T, lambda_r)
//     dL/dA = - sum_i (pi_i dx_{i-1}' + eta_i x_{i-1}'),   dL/dB = - sum_i (pi_i dv_i' + eta_i v_i'),   dL/dC = - sum_i (o_i dx_i' + do_i x_i'),
//     dL/dBd = - sum_i eta_i d_{i-1}',                     dL/dDd = - sum_i do_i d_{i-1}'                                     (i = 1 .. ph).
// lambda is not an output of the solve.  It comes from the optimum's own sequences: one backward pass gives the condensed gradient of the cost,
// grad, at w*, and S lambda = -Y[A, 0:nz] grad + [soft rows: row value - violated bound] on the factor of S that served mu -- stationarity on
// every row, plus a soft row's own relation lambda_r / rho_r = violation, whose 1 / rho_r sits on S's diagonal.
// The plan is lmpc_param_sensitivity's: a workgroup takes sixteen instances; one wavefront per instance decodes the working set, factors S in LDS
// and leaves (rows, mu, lambda) in the instance's record and q as a column of an MFMA B operand; Xq Q goes through the f64 matrix pipe; then one
// wavefront per instance forms the stage gradients and the two costates, and the workgroup sums the outer products, an output entry per thread.
// reduce: the instances are added in instance order into the workgroup's row of a partials buffer, lmpc_sens_reduce adds the rows in workgroup
// order -- no floating-point atomics, the same bits on every launch.
// The working set, the factor, the solve on it, q, the tile product and the reduce kernel are lmpc_sens_common.hpp's, shared with the other
// sensitivity kernels.
#include "lmpc_sens_common.hpp"

namespace mpcx {

namespace {

constexpr int kModelIpg = 16;      // instances of a workgroup: one MFMA column tile

struct LmpcModelDev {
    int batch, reduce;
    int cap;                      // rows of S a wavefront's LDS slice holds
    int rows16, G;                // rows of Xq padded to the row tile; k-step groups per row tile of its packed copy
    const uint32_t *al, *au;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    const double *u0, *seq_state, *seq_output, *seq_input;
    const double *yref; long yref_bs, yref_ks;
    const double *uref; long uref_bs, uref_ks;
    const double *duref; long duref_bs, duref_ks;
    const double *dmeas; long dmeas_bs, dmeas_ks;
    double *d_A, *d_B, *d_C, *d_Bd, *d_Dd;
    int32_t *flags, *n_used;
    double *part;                 // [groups x (glen + 1)]: A | B | C | Bd | Dd | instances that contributed
    const double *Xqp;            // Xq [rows16 x nz], packed
};

__host__ __device__ inline size_t model_glen(int nx, int nu, int ny, int ndu) { return (size_t)nx * (nx + nu + ndu) + (size_t)ny * (nx + ndu); }
// an instance's record: mu | lambda | unified indices of its working rows (ints)
__host__ __device__ inline size_t model_rec_len(int cap) { return 2 * (size_t)cap + (size_t)(cap + 1) / 2; }
// cotangents and directions as MFMA B operands | Xq Q | A, B, C | flags and row counts of the group's instances (ints) | the sixteen records
__host__ __device__ inline size_t model_shared_len(int nz16, int rows16, int nx, int nu, int ny, int cap)
{
    return 2 * (size_t)(nz16 / 4) * 64 + (size_t)kModelIpg * rows16 + (size_t)nx * (nx + nu) + (size_t)ny * nx + 16 + kModelIpg * model_rec_len(cap);
}
// a wavefront's slice: S (packed lower triangle) | its original diagonal | sides of the working rows (ints) | the cost's condensed gradient |
// two state vectors and an output vector of the backward pass | pi, eta [ph x nx] | o, do [ph x ny]
__host__ __device__ inline size_t model_wave_len(int cap, int nz, int nx, int ny, int ph)
{
    return (size_t)cap * (cap + 1) / 2 + (size_t)cap + (size_t)(cap + 1) / 2 + nz + 3 * (size_t)nx + ny + 2 * (size_t)ph * (nx + ny);
}

__global__ __launch_bounds__(256) void lmpc_model_sensitivity(const LmpcDev *__restrict__ Mp, const LmpcModelDev Pd)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
    const int j16 = lane & 15, kq = lane >> 4;
    const int nx = M.nx, nu = M.nu, ny = M.ny, ndu = M.ndu, nz = M.nz, mg = M.mg, ph = M.ph;
    const int ldz = M.ldz, ldy = M.ldy, aw = M.active_words;
    const int nz4 = M.nz16 >> 2, cap = Pd.cap, rows16 = Pd.rows16, reduce = Pd.reduce;
    const int nA = nx * nx, nB = nx * nu, nC = ny * nx, nBd = nx * ndu, nDd = ny * ndu;
    const int glen = nA + nB + nC + nBd + nDd;
    const size_t plen = (size_t)glen + 1, n1 = (size_t)ph + 1;
    double *Bp = smem;                                            // [nz4][64]  the cotangents as an MFMA B operand (column = instance)
    double *Qp = Bp + (size_t)nz4 * 64;                           // [nz4][64]  the directions q, likewise
    double *DX = Qp + (size_t)nz4 * 64;                           // [16][rows16]  Xq q of every instance: dx_1 .. dx_ph
    double *As = DX + (size_t)kModelIpg * rows16, *Bs = As + nA, *Cs = Bs + nB;      // the model, column-major
    int *flg = reinterpret_cast<int *>(Cs + nC);                  // [16] flag of each instance, -1 beyond the batch
    int *cnt = flg + kModelIpg;                                   // [16] rows of each instance's working set
    double *recs = Cs + nC + 16;
    double *slices = recs + kModelIpg * model_rec_len(cap);
    auto mu_of = [&](int il) -> double * { return recs + (size_t)il * model_rec_len(cap); };
    auto idx_of = [&](int il) -> int * { return reinterpret_cast<int *>(mu_of(il) + 2 * (size_t)cap); };
    auto slice_of = [&](int w) -> double * { return slices + (size_t)w * model_wave_len(cap, nz, nx, ny, ph); };
    auto pi_of = [&](int w) -> double * { return slice_of(w) + (size_t)cap * (cap + 1) / 2 + cap + (size_t)(cap + 1) / 2 + nz + 3 * (size_t)nx + ny; };
    double *S = slice_of(wave), *dg = S + (size_t)cap * (cap + 1) / 2;
    // the working rows' slots 2 row + (upper ? 1 : 0) as sens_working_set leaves them; bit 0 is read on general rows only, which have one reference
    // row each: there it says that the row's upper bound is the working one
    int *sdv = reinterpret_cast<int *>(dg + cap);
    double *grad = dg + cap + (size_t)(cap + 1) / 2, *c0 = grad + nz, *c1 = c0 + nx, *xt = c1 + nx, *ey = xt + nx;
    double *pi = ey + ny, *eta = pi + (size_t)ph * nx, *ov = eta + (size_t)ph * nx, *dov = ov + (size_t)ph * ny;
    const gdp Y = GP(Y);
    const gip blk = GP(blk);
    const gdp Wy = GP(Wy), Wu = GP(Wu), Wdu = GP(Wdu), sX = GP(sX), sU = GP(sU), gsoft = gl(MPCX_G_SOFT(M));
    const bool term = MPCX_HAS_TERMINAL(M);
    const gdp tP = gl(MPCX_TERMINAL(M)), tXT = tP + nA, tTx = tXT + nx;
    const gdp Flin = gl(MPCX_LINEAR_F(M));
    const double qnan = __builtin_nan("");
    const gdp yr = gl(Pd.yref), ur = gl(Pd.uref), dr = gl(Pd.duref), dm = gl(Pd.dmeas);
    const gdp sqx = gl(Pd.seq_state), sqy = gl(Pd.seq_output), sqv = gl(Pd.seq_input), u0p = gl(Pd.u0);
    // v_i of instance b: v_0 = lastU, v_i = row i - 1 of the sequence
    auto vin = [&](int b, int i, int j) -> double { return i > 0 ? sqv[((size_t)b * n1 + i - 1) * nu + j] : u0p[(size_t)b * nu + j]; };
    // the rate term of the increment delta_i = v_{i+1} - v_i, i = 0 .. ph - 1
    auto rate = [&](int b, int i, int j) -> double {
        return Wdu[j + (size_t)i * nu] * (vin(b, i + 1, j) - vin(b, i, j) - ref_at(dr, Pd.duref_bs, Pd.duref_ks, b, i > 0 ? i - 1 : 0, j));
    };

    for (int t = tid; t < nA + nB + nC; t += blockDim.x) As[t] = t < nA ? GP(A)[t] : (t < nA + nB ? GP(B)[t - nA] : GP(C)[t - nA - nB]);

    for (int g0 = blockIdx.x; g0 * kModelIpg < Pd.batch; g0 += gridDim.x) {
        const int b0 = g0 * kModelIpg;
        double *part = Pd.part ? Pd.part + (size_t)g0 * plen : nullptr;
        for (int t = tid; t < 2 * nz4 * 64; t += blockDim.x) Bp[t] = 0.0;
        if (reduce) for (int t = tid; t < glen; t += blockDim.x) glw(part)[t] = 0.0;       // (entry t stays with this thread to the end)
        __syncthreads();
        // ---- the cotangents on w: the seeds on cmd and on the input sequence scattered through blk, as lmpc_sensitivity's VJP mode
        for (int t = tid; t < kModelIpg * nz; t += blockDim.x) {
            const int il = t / nz, q = t - il * nz, b = b0 + il;
            if (b >= Pd.batch) continue;
            sens_opnd(Bp, il, q) = sens_seed(Pd.seed_cmd, Pd.seed_input, blk, nu, ph, b, q);
        }
        __syncthreads();

        // ---- per instance, one wavefront each, W instances a round: working set, factor, mu, q, lambda
        for (int r0 = 0; r0 < kModelIpg; r0 += W) {
            const int il = r0 + wave, b = b0 + il;
            const bool valid = b < Pd.batch;
            double *V = mu_of(il), *R = V + cap;
            int *idx = idx_of(il);
            int flag = 0, n = 0;
            auto cot = [&](int q) { return sens_opnd(Bp, il, q); };      // the instance's cotangent
            if (valid) {
                flag = (Pd.status && gl(Pd.status)[b] != 0) ? 1 : 0;
                if (!flag) {
                    n = sens_working_set(M, gl(Pd.al) + (size_t)b * aw, gl(Pd.au) + (size_t)b * aw, aw, nz, mg, ldz, cap, lane, idx, sdv);
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
            if (valid && !flag && n > 0) {
                // the cost's condensed gradient at the optimum: one backward pass over the solve's own sequences
                for (int t = lane; t < nz; t += 64) grad[t] = 0.0;
                for (int a = lane; a < nx; a += 64) {
                    c0[a] = 0.0;
                    if (term) {           // x_ph - x_T, x_T = xT + Tx [yref_{ph-1}; d_{ph-1}]
                        double s = tXT[a];
                        for (int j = 0; j < ny; ++j) s = fma(tTx[a + (size_t)j * nx], ref_at(yr, Pd.yref_bs, Pd.yref_ks, b, ph - 1, j), s);
                        for (int d = 0; d < ndu; ++d) s = fma(tTx[a + (size_t)(ny + d) * nx], ref_at(dm, Pd.dmeas_bs, Pd.dmeas_ks, b, ph - 1, d), s);
                        xt[a] = sqx[((size_t)b * n1 + ph) * nx + a] - s;
                    }
                }
                wave_sync();
                double *cp = c0, *cn = c1;
                for (int i = ph; i >= 1; --i) {
                    for (int j = lane; j < ny; j += 64)
                        ey[j] = Wy[j + (size_t)i * ny] * (sqy[((size_t)b * n1 + i) * ny + j] - ref_at(yr, Pd.yref_bs, Pd.yref_ks, b, i - 1, j));
                    wave_sync();
                    for (int a = lane; a < nx; a += 64) {
                        double s = 0.0;
                        for (int j = 0; j < ny; ++j) s = fma(Cs[j + (size_t)a * ny], ey[j], s);
                        if (i < ph) for (int c = 0; c < nx; ++c) s = fma(As[c + (size_t)a * nx], cp[c], s);
                        else if (term) for (int c = 0; c < nx; ++c) s = fma(tP[a + (size_t)c * nx], xt[c], s);
                        cn[a] = s;
                    }
                    wave_sync();
                    for (int j = lane; j < nu; j += 64) {
                        double s = Wu[j + (size_t)i * nu] * (vin(b, i, j) - ref_at(ur, Pd.uref_bs, Pd.uref_ks, b, i - 1, j)) + rate(b, i - 1, j);
                        if (i < ph) s -= rate(b, i, j);
                        for (int a = 0; a < nx; ++a) s = fma(Bs[a + (size_t)j * nx], cn[a], s);
                        grad[blk[i] * nu + j] += s;
                    }
                    double *sw = cp; cp = cn; cn = sw;
                    wave_sync();
                }
                // S lambda = -Y[A, 0:nz] grad, and on a soft row its violation besides
                for (int k = lane; k < n; k += 64) {
                    const int qi = idx[k];
                    double s = 0.0;
                    for (int q = 0; q < nz; ++q) s = fma(-Y[(size_t)q * ldy + qi], grad[q], s);
                    const int rr = qi - ldz;
                    if (rr >= 0 && gsoft[rr] > 0.0) {
                        const int kind = GP(g_kind)[rr], st = GP(g_step)[rr], cpn = GP(g_comp)[rr];
                        const gdp xs = sqx + ((size_t)b * n1 + st) * nx;
                        double v = 0.0;
                        if (kind == G_STATE) v = xs[cpn];
                        else if (kind == G_OUTPUT) v = sqy[((size_t)b * n1 + st) * ny + cpn];
                        else if (kind == G_SCALAR) {
                            for (int c = 0; c < nx; ++c) v = fma(sX[c], xs[c], v);
                            for (int j = 0; j < nu; ++j) v = fma(sU[j], vin(b, st, j), v);
                        } else if (kind == G_LINEAR) {
                            const gdp F = Flin + (size_t)cpn * (nx + nu);
                            for (int c = 0; c < nx; ++c) v = fma(F[c], xs[c], v);
                            for (int j = 0; j < nu; ++j) v = fma(F[nx + j], vin(b, st, j), v);
                        } else v = vin(b, st, cpn) - vin(b, st - 1, cpn);
                        s += v - ((sdv[k] & 1) ? GP(ug0)[rr] : GP(lg0)[rr]);
                    }
                    R[k] = s;
                }
                wave_sync();
                sens_chol_solve(S, R, n, lane);
            }
            if (valid && Pd.flags && lane == 0) glw(Pd.flags)[b] = flag;
            if (lane == 0) { flg[il] = valid ? flag : -1; cnt[il] = (valid && !flag) ? n : 0; }
            wave_sync();
        }
        __syncthreads();

        // ---- Xq Q: the row tiles over the wavefronts
        const int ntile = rows16 >> 4;
        for (int t = wave; t < ntile; t += W) {
            const v4d acc = sens_mfma_tile(gl(Pd.Xqp), t, Pd.G, nz4, Qp, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) DX[(size_t)j16 * rows16 + 16 * t + 4 * r + kq] = acc[r];
        }
        __syncthreads();

        // ---- per instance again: the stage gradients from the row tables, the two costates; then the outer products, an entry per thread
        for (int r0 = 0; r0 < kModelIpg; r0 += W) {
            const int il = r0 + wave, b = b0 + il;
            if (flg[il] == 0) {
                const double *V = mu_of(il), *R = V + cap, *dx = DX + (size_t)il * rows16;
                const int *idx = idx_of(il);
                const int n = cnt[il];
                for (int t = lane; t < ph * nx; t += 64) { pi[t] = 0.0; eta[t] = 0.0; }
                for (int t = lane; t < ph * ny; t += 64) {
                    const int i = t / ny + 1, j = t - (i - 1) * ny;
                    const double w = Wy[j + (size_t)i * ny];
                    double s = 0.0;
                    for (int c = 0; c < nx; ++c) s = fma(Cs[j + (size_t)c * ny], dx[(i - 1) * nx + c], s);
                    ov[t] = w * (sqy[((size_t)b * n1 + i) * ny + j] - ref_at(yr, Pd.yref_bs, Pd.yref_ks, b, i - 1, j));
                    dov[t] = w * s;
                }
                if (term)
                    for (int a = lane; a < nx; a += 64) {
                        double s = tXT[a];
                        for (int j = 0; j < ny; ++j) s = fma(tTx[a + (size_t)j * nx], ref_at(yr, Pd.yref_bs, Pd.yref_ks, b, ph - 1, j), s);
                        for (int d = 0; d < ndu; ++d) s = fma(tTx[a + (size_t)(ny + d) * nx], ref_at(dm, Pd.dmeas_bs, Pd.dmeas_ks, b, ph - 1, d), s);
                        xt[a] = sqx[((size_t)b * n1 + ph) * nx + a] - s;
                    }
                wave_sync();
                // the working rows one after the other; an entry is always touched by the same lane
                for (int k = 0; k < n; ++k) {
                    const int rr = idx[k] - ldz;
                    if (rr < 0) continue;
                    const int kind = GP(g_kind)[rr], st = GP(g_step)[rr], cpn = GP(g_comp)[rr];
                    if (st < 1) continue;
                    const double lam = R[k], mu = V[k];
                    if (kind == G_OUTPUT) { if (lane == (cpn & 63)) { ov[(st - 1) * ny + cpn] += lam; dov[(st - 1) * ny + cpn] += mu; } }
                    else if (kind == G_STATE) { if (lane == (cpn & 63)) { pi[(st - 1) * nx + cpn] += lam; eta[(st - 1) * nx + cpn] += mu; } }
                    else if (kind == G_SCALAR || kind == G_LINEAR) {
                        const gdp F = kind == G_SCALAR ? sX : Flin + (size_t)cpn * (nx + nu);
                        for (int c = lane; c < nx; c += 64) { pi[(st - 1) * nx + c] = fma(lam, F[c], pi[(st - 1) * nx + c]); eta[(st - 1) * nx + c] = fma(mu, F[c], eta[(st - 1) * nx + c]); }
                    }
                }
                wave_sync();
                for (int i = ph; i >= 1; --i) {
                    double *pc = pi + (size_t)(i - 1) * nx, *ec = eta + (size_t)(i - 1) * nx;
                    const double *oc = ov + (size_t)(i - 1) * ny, *dc = dov + (size_t)(i - 1) * ny;
                    for (int a = lane; a < nx; a += 64) {
                        double s = pc[a], e = ec[a];
                        for (int j = 0; j < ny; ++j) { s = fma(Cs[j + (size_t)a * ny], oc[j], s); e = fma(Cs[j + (size_t)a * ny], dc[j], e); }
                        if (i < ph)
                            for (int c = 0; c < nx; ++c) { s = fma(As[c + (size_t)a * nx], pc[nx + c], s); e = fma(As[c + (size_t)a * nx], ec[nx + c], e); }
                        else if (term)
                            for (int c = 0; c < nx; ++c) { s = fma(tP[a + (size_t)c * nx], xt[c], s); e = fma(tP[a + (size_t)c * nx], dx[(ph - 1) * nx + c], e); }
                        pc[a] = s; ec[a] = e;
                    }
                    wave_sync();
                }
            }
            __syncthreads();
            for (int t = tid; t < glen; t += blockDim.x) {
                const int kind = t < nA ? 0 : (t < nA + nB ? 1 : (t < nA + nB + nC ? 2 : (t < nA + nB + nC + nBd ? 3 : 4)));
                const int tt = t - (kind == 0 ? 0 : (kind == 1 ? nA : (kind == 2 ? nA + nB : (kind == 3 ? nA + nB + nC : nA + nB + nC + nBd))));
                const int rows = (kind == 2 || kind == 4) ? ny : nx, c = tt / rows, r = tt - c * rows;      // column-major: the setters' layout
                const int len = kind == 0 ? nA : (kind == 1 ? nB : (kind == 2 ? nC : (kind == 3 ? nBd : nDd)));
                double *out = kind == 0 ? Pd.d_A : (kind == 1 ? Pd.d_B : (kind == 2 ? Pd.d_C : (kind == 3 ? Pd.d_Bd : Pd.d_Dd)));
                double sum = 0.0;
                for (int w = 0; w < W; ++w) {
                    const int iw = r0 + w, bw = b0 + iw, f = flg[iw];
                    if (f < 0) break;
                    double v = qnan;
                    if (f == 0) {
                        const double *pw = pi_of(w), *ew = pw + (size_t)ph * nx, *ow = ew + (size_t)ph * nx, *dw = ow + (size_t)ph * ny;
                        const double *dx = DX + (size_t)iw * rows16;
                        const gdp xs = sqx + (size_t)bw * n1 * nx;
                        double s = 0.0;
                        for (int i = 1; i <= ph; ++i) {
                            if (kind == 0) {
                                s = fma(ew[(i - 1) * nx + r], xs[(size_t)(i - 1) * nx + c], s);
                                if (i > 1) s = fma(pw[(i - 1) * nx + r], dx[(i - 2) * nx + c], s);
                            } else if (kind == 1) {
                                s = fma(ew[(i - 1) * nx + r], vin(bw, i, c), s);
                                s = fma(pw[(i - 1) * nx + r], sens_opnd(Qp, iw, blk[i] * nu + c), s);
                            } else if (kind == 2) {
                                s = fma(dw[(i - 1) * ny + r], xs[(size_t)i * nx + c], s);
                                s = fma(ow[(i - 1) * ny + r], dx[(i - 1) * nx + c], s);
                            } else if (kind == 3) s = fma(ew[(i - 1) * nx + r], ref_at(dm, Pd.dmeas_bs, Pd.dmeas_ks, bw, i - 1, c), s);
                            else s = fma(dw[(i - 1) * ny + r], ref_at(dm, Pd.dmeas_bs, Pd.dmeas_ks, bw, i - 1, c), s);
                        }
                        v = -s;
                    }
                    if (reduce) { if (f == 0) sum += v; }
                    else if (out) glw(out)[(size_t)bw * len + tt] = v;
                }
                if (reduce) glw(part)[t] += sum;
            }
            __syncthreads();
        }
        if (reduce && tid == 0) {
            int used = 0;
            for (int il = 0; il < kModelIpg; ++il) used += flg[il] == 0;
            glw(part)[plen - 1] = (double)used;
        }
        __syncthreads();
    }
}

}  // namespace

// Xq = d (states of the steps 1 .. ph) / d w as the kernel's A operand source: [rows16 x nz] column-major, row (i - 1) nx + a = state a of step i,
// by rolling the model out from x0 = 0 on the unit vectors of w (no exogenous input: the linear part).  A, B column-major
size_t lmpc_model_sens_xq(int nx, int nu, int ph, int nz, const double *A, const double *B, const int *blk, double *out)
{
    const int rows16 = (nx * ph + 15) / 16 * 16;
    const size_t len = (size_t)rows16 * nz;
    if (!out) return len;
    for (int q = 0; q < nz; ++q) {
        double *col = out + (size_t)q * rows16;
        for (int r = 0; r < rows16; ++r) col[r] = 0.0;
        sens_unit_rollout(nx, nu, ph, q, A, B, blk, [&](int i, const double *x) { for (int a = 0; a < nx; ++a) col[(i - 1) * nx + a] = x[a]; });
    }
    return len;
}

size_t lmpc_model_sens_partials(const LmpcDev &m, int batch)
{
    return (size_t)((batch + kModelIpg - 1) / kModelIpg) * (model_glen(m.nx, m.nu, m.ny, m.ndu) + 1);
}

int lmpc_model_sens_launch(const LmpcDev &m, const LmpcDev *m_dev, const double *Xqp, const LmpcModelSensArgs &a, void *stream)
{
    LmpcModelDev s{};
    s.batch = a.batch; s.reduce = a.reduce ? 1 : 0;
    s.rows16 = (m.nx * m.ph + 15) / 16 * 16; s.G = (m.nz + 15) / 16;
    s.al = a.active_lower; s.au = a.active_upper; s.status = a.status;
    s.seed_cmd = a.seed_cmd; s.seed_input = a.seed_input;
    s.u0 = a.u0; s.seq_state = a.seq_state; s.seq_output = a.seq_output; s.seq_input = a.seq_input;
    s.yref = a.yref; s.yref_bs = a.yref_bs; s.yref_ks = a.yref_ks;
    s.uref = a.uref; s.uref_bs = a.uref_bs; s.uref_ks = a.uref_ks;
    s.duref = a.duref; s.duref_bs = a.duref_bs; s.duref_ks = a.duref_ks;
    s.dmeas = a.dmeas; s.dmeas_bs = a.dmeas_bs; s.dmeas_ks = a.dmeas_ks;
    s.d_A = a.d_A; s.d_B = a.d_B; s.d_C = a.d_C; s.d_Bd = m.ndu > 0 ? a.d_Bd : nullptr; s.d_Dd = m.ndu > 0 ? a.d_Dd : nullptr;
    s.flags = a.flags; s.n_used = a.n_used; s.part = a.reduce ? a.partials : nullptr; s.Xqp = Xqp;
    if (a.reduce && !a.partials) return -3;
    // the wavefronts' slices beside the shared operands and the sixteen records, which grow with the capacity as well
    const SensLdsPlan plan = sens_lds_plan(m, 4, [&](int waves, int cap) {
        return model_shared_len(m.nz16, s.rows16, m.nx, m.nu, m.ny, cap) + waves * model_wave_len(cap, m.nz, m.nx, m.ny, m.ph);
    });
    if (plan.cap <= 0) return -2;
    s.cap = plan.cap;
    static LmpcLdsCache configured;
    if (lmpc_raise_dynamic_lds(configured, {reinterpret_cast<const void *>(lmpc_model_sensitivity)}, plan.bytes) != 0) return -3;
    const int groups = (a.batch + kModelIpg - 1) / kModelIpg;
    const int blocks = groups > 65536 ? 65536 : groups;
    hipLaunchKernelGGL(lmpc_model_sensitivity, dim3(blocks), dim3(64 * plan.waves), plan.bytes, static_cast<hipStream_t>(stream), m_dev, s);
    if (hipGetLastError() != hipSuccess) return -3;
    if (!a.reduce) return 0;
    const size_t eA = (size_t)m.nx * m.nx, eB = eA + (size_t)m.nx * m.nu, eC = eB + (size_t)m.ny * m.nx, eBd = eC + (size_t)m.nx * m.ndu;      // model_glen's order
    const size_t glen = model_glen(m.nx, m.nu, m.ny, m.ndu);
    return sens_reduce_launch(SensReduce{s.part, glen + 1, {eA, eB, eC, eBd, glen}, {s.d_A, s.d_B, s.d_C, s.d_Bd, s.d_Dd}, s.n_used, groups}, stream);
}

}  // namespace mpcx
