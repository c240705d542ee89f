// Sensitivities of a solved batch of a bank: vector-Jacobian products of the decision vector w with respect to
// vin = [x0 | lastU | yref], every instance on its own controller.
//
// A bank's controllers carry no composed affine maps (MF1), so 4.8's formula is restated without them.  On the working set A, with
// S = Y[A, A] and a cotangent p on w,
//     mu = S^-1 Y[A, 0:nz] p,     q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu,     g = -F' q - OFF[A, :]' mu
// F = df/dvin is the linear term's dependence on the data and OFF = d(offset of a general row)/dvin (its bounds are lg0 - off, ug0 - off).  Both
// are the linear part of the roll-out in lmpc_assemble_generic, so both products are its adjoint and need no matrix of the condensed problem:
//     dv_i = q[blk[i] nu + .],  dx_0 = 0,  dx_i = A dx_{i-1} + B dv_i                                       i = 1 .. ph
//     do_i  = Wy_i C dx_i                                                  (d_yref sums these, and Tx' P dx_ph of the terminal target)
//     gam_i = C' (do_i + output rows' mu_r e_comp) + state rows' mu_r e_comp + scalar / linear rows' mu_r sX / Fx[c, :] + [i = ph] P dx_ph
//     eta_ph = gam_ph,  eta_i = gam_i + A' eta_{i+1},      d_x0 = -A' eta_1 - gam_0
//     d_u0 = Wdu[:, 0] dv_1 + (rate rows of step 1) mu_r e_comp - (scalar / linear rows of step 0) mu_r sU / Fu[c, :]
// gam_0 and the last term of d_u0 belong to rows of step 0, which are in the condensed problem only where a slack variable makes them soft.
//
// One wavefront per instance, the whole kernel without a workgroup barrier.  Every matrix differs from instance to instance: there is no shared
// operand for the matrix pipe.  The seeds of an instance (nu unit seeds in Jacobian mode) are served one after another on one factor of S.
// The working-set decode, the factor of S, the solve on it and the seed scatter are lmpc_sens_common.hpp's, shared with the other sensitivity kernels;
// the roll-out of the direction is lmpc_bank_common.hpp's, shared with the bank's gradient kernel (lmpc_bank_grad.hip).
#include "lmpc_bank_common.hpp"

namespace mpcx {

namespace {

struct LmpcBankSensDev {
    LmpcBankSensArgs a;
    int nx, nu, ny, ph, nz, mg, ldz, ldy, aw, term;      // controller 0's: the same for every controller of a bank
    int R;                                               // seeds per instance
    int cap;                                             // rows of S a wavefront's LDS slice holds
};

// a wavefront's slice: S (packed lower triangle) | its original diagonal | one right-hand side | the working set's unified indices and the kind,
// step and component of its general rows (ints) | blk (ints) | A, B, C | p, q | dx [(ph + 1) x nx] and P dx_ph | do [ph x ny] | gam [(ph + 1) x nx] |
// the sums of d_u0.  Nothing a recursion over the horizon reads lies in HBM: a step of it costs LDS latency, not a trip to memory
__host__ __device__ inline size_t bank_wave_len(int cap, int nx, int nu, int ny, int ph, int nz)
{
    return (size_t)cap * (cap + 1) / 2 + 2 * (size_t)cap + 2 * (size_t)cap + (size_t)(ph + 2) / 2 + (size_t)nx * (nx + nu) + (size_t)ny * nx +
           2 * (size_t)bank_even(nz) + (size_t)(ph + 2) * nx + (size_t)ph * ny + (size_t)(ph + 1) * nx + nu;
}

__global__ __launch_bounds__(256) void lmpc_bank_sensitivity(const LmpcBankSensDev Sd)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;       // one instance per wavefront; the grid covers the batch
    if (b >= Sd.a.s.batch) return;                                        // (a whole wavefront: the kernel has no workgroup barrier)
    const LmpcSensArgs &Ar = Sd.a.s;
    const int nx = Sd.nx, nu = Sd.nu, ny = Sd.ny, ph = Sd.ph, nz = Sd.nz, mg = Sd.mg, ldz = Sd.ldz, ldy = Sd.ldy, aw = Sd.aw;
    const int cap = Sd.cap, R = Sd.R, nzp = bank_even(nz);
    const bool jac = Ar.jacobian, term = Sd.term != 0;
    const double qnan = __builtin_nan("");

    double *S = smem + (size_t)wave * bank_wave_len(cap, nx, nu, ny, ph, nz);
    double *dg = S + (size_t)cap * (cap + 1) / 2, *V = dg + cap;
    int *idx = reinterpret_cast<int *>(V + cap), *rkind = idx + cap, *rstep = rkind + cap, *rcomp = rstep + cap;
    int *blk = reinterpret_cast<int *>(V + 3 * (size_t)cap);
    double *As = V + 3 * (size_t)cap + (size_t)(ph + 2) / 2, *Bs = As + (size_t)nx * nx, *Cs = Bs + (size_t)nx * nu;
    double *pv = Cs + (size_t)ny * nx, *qv = pv + nzp;
    double *dx = qv + nzp, *pdx = dx + (size_t)(ph + 1) * nx;
    double *dov = pdx + nx, *gam = dov + (size_t)ph * ny, *du = gam + (size_t)(ph + 1) * nx;

    // the instance's controller; an index outside the bank is answered like an instance that was not solved
    const int km = __builtin_amdgcn_readfirstlane(Sd.a.n_models <= 0 ? 0 : (Sd.a.model_index ? (int)gl(Sd.a.model_index)[b] : b));
    const bool known = km >= 0 && km < (Sd.a.n_models > 0 ? Sd.a.n_models : 1);
    const LmpcDev &M = Sd.a.models[known ? km : 0];
    int flag = (!known || (Ar.status && gl(Ar.status)[b] != 0)) ? 1 : 0;
    int n = 0;
    if (!flag) {
        n = sens_working_set(M, gl(Ar.active_lower) + (size_t)b * aw, gl(Ar.active_upper) + (size_t)b * aw, aw, nz, mg, ldz, cap, lane, idx, nullptr);
        if (n > cap) flag = 3;
    }
    wave_sync();
    const gdp Y = GP(Y);
    if (!flag) {
        const int nA = nx * nx, nB = nx * nu, nC = ny * nx;
        for (int t = lane; t < nA + nB + nC; t += 64) As[t] = t < nA ? GP(A)[t] : (t < nA + nB ? GP(B)[t - nA] : GP(C)[t - nA - nB]);
        for (int i = lane; i <= ph; i += 64) blk[i] = GP(blk)[i];
        for (int k = lane; k < n; k += 64) {
            const int rr = idx[k] - ldz;
            rkind[k] = rr >= 0 ? GP(g_kind)[rr] : -1; rstep[k] = rr >= 0 ? GP(g_step)[rr] : 0; rcomp[k] = rr >= 0 ? GP(g_comp)[rr] : 0;
        }
        wave_sync();
        if (n > 0 && !sens_factor(Y, ldy, idx, n, lane, S, dg)) flag = 2;
    }
    wave_sync();

    for (int r = 0; r < R; ++r) {
        const size_t row = (size_t)b * R + r;
        if (flag) {
            for (int a = lane; a < nx; a += 64) if (Ar.d_x0) glw(Ar.d_x0)[row * nx + a] = qnan;
            for (int j = lane; j < nu; j += 64) if (Ar.d_u0) glw(Ar.d_u0)[row * nu + j] = qnan;
            for (int j = lane; j < ny; j += 64) if (Ar.d_yref) glw(Ar.d_yref)[row * ny + j] = qnan;
            continue;
        }
        // ---- the cotangent on w: a unit vector on the first move (then Y p is a column of Y), or the seeds scattered through blk
        const int col = blk[1] * nu + r;
        if (!jac) {
            for (int t = lane; t < nzp; t += 64) pv[t] = t < nz ? sens_seed(Ar.seed_cmd, Ar.seed_input, blk, nu, ph, b, t) : 0.0;
            wave_sync();
        }
        // ---- mu = S^-1 Y[A, 0:nz] p, a row per lane (Y is symmetric: row idx[i] of a column)
        for (int i = lane; i < n; i += 64) {
            const int qi = idx[i];
            V[i] = jac ? Y[(size_t)col * ldy + qi] : sens_rhs(Y, ldy, nz, qi, [&](int q) { return pv[q]; });
        }
        wave_sync();
        sens_chol_solve(S, V, n, lane);
        // ---- q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu: a lane owns element pairs of the contiguous columns, one 16-byte load each (ldy is even)
        for (int e = 2 * lane; e < nz; e += 128) {
            double s0 = 0.0, s1 = 0.0;
            if (jac) { const d2 y = ld2(Y + (size_t)col * ldy + e); s0 = y.x; s1 = y.y; }
            else
                for (int q = 0; q < nz; ++q) {
                    const double p = pv[q];
                    if (p != 0.0) { const d2 y = ld2(Y + (size_t)q * ldy + e); s0 = fma(y.x, p, s0); s1 = fma(y.y, p, s1); }
                }
            for (int i = 0; i < n; ++i) {
                const d2 y = ld2(Y + (size_t)idx[i] * ldy + e);
                s0 = fma(-y.x, V[i], s0); s1 = fma(-y.y, V[i], s1);
            }
            qv[e] = s0; qv[e + 1] = e + 1 < nz ? s1 : 0.0;
        }
        wave_sync();
        // ---- forward: the direction through the instance's model
        bank_rollout(As, Bs, Cs, GP(Wy), blk, qv, nx, nu, ny, ph, lane, dx, dov);
        const double *dxph = dx + (size_t)ph * nx;
        const gdp tP = gl(MPCX_TERMINAL(M)), tTx = tP + (size_t)nx * nx + nx;
        for (int a = lane; a < nx; a += 64) {
            double s = 0.0;
            if (term) for (int c = 0; c < nx; ++c) s = fma(tP[a + (size_t)c * nx], dxph[c], s);
            pdx[a] = s;
        }
        for (int t = lane; t < (ph + 1) * nx; t += 64) gam[t] = 0.0;
        for (int j = lane; j < nu; j += 64) du[j] = GP(Wdu)[j] * qv[blk[1] * nu + j];
        wave_sync();
        // d_yref: the cost's part of do_i alone, and the terminal target's Tx-columns of yref
        for (int j = lane; j < ny; j += 64) {
            double s = 0.0;
            for (int i = 0; i < ph; ++i) s += dov[i * ny + j];
            if (term) for (int a = 0; a < nx; ++a) s = fma(tTx[a + (size_t)j * nx], pdx[a], s);
            if (Ar.d_yref) glw(Ar.d_yref)[row * ny + j] = s;
        }
        for (int a = lane; a < nx; a += 64) gam[(size_t)ph * nx + a] = pdx[a];
        // ---- the working rows one after the other; an entry is always touched by the same lane
        for (int k = 0; k < n; ++k) {
            const int kind = rkind[k], st = rstep[k], cpn = rcomp[k];
            if (kind < 0) continue;
            const double mu = V[k];
            if (kind == G_OUTPUT) {
                if (st >= 1) { if (lane == (cpn & 63)) dov[(st - 1) * ny + cpn] += mu; }
                else for (int c = lane; c < nx; c += 64) gam[c] = fma(mu, Cs[cpn + (size_t)c * ny], gam[c]);
            } else if (kind == G_STATE) {
                if (lane == (cpn & 63)) gam[(size_t)st * nx + cpn] += mu;
            } else if (kind == G_SCALAR || kind == G_LINEAR) {
                const gdp Fx = kind == G_SCALAR ? GP(sX) : gl(MPCX_LINEAR_F(M)) + (size_t)cpn * (nx + nu);
                const gdp Fu = kind == G_SCALAR ? GP(sU) : Fx + nx;
                for (int c = lane; c < nx; c += 64) gam[(size_t)st * nx + c] = fma(mu, Fx[c], gam[(size_t)st * nx + c]);
                if (st == 0) for (int j = lane; j < nu; j += 64) du[j] = fma(-mu, Fu[j], du[j]);
            } else if (kind == G_RATE && st == 1) {
                if (lane == (cpn & 63)) du[cpn] += mu;
            }
        }
        wave_sync();
        // ---- backward: eta_i = gam_i + C' do_i + A' eta_{i+1}, in place: the output terms of every step at once, then the chain
        for (int t = lane; t < ph * nx; t += 64) {
            const int i = t / nx + 1, a = t - (i - 1) * nx;
            const double *dc = dov + (size_t)(i - 1) * ny;
            double s = gam[(size_t)i * nx + a];
#pragma unroll 4
            for (int j = 0; j < ny; ++j) s = fma(Cs[j + (size_t)a * ny], dc[j], s);
            gam[(size_t)i * nx + a] = s;
        }
        wave_sync();
        for (int i = ph - 1; i >= 1; --i) {
            double *gc = gam + (size_t)i * nx;
            for (int a = lane; a < nx; a += 64) {
                double s = gc[a];
#pragma unroll 4
                for (int c = 0; c < nx; ++c) s = fma(As[c + (size_t)a * nx], gc[nx + c], s);
                gc[a] = s;
            }
            wave_sync();
        }
        for (int a = lane; a < nx; a += 64) {
            double s = gam[a];
#pragma unroll 4
            for (int c = 0; c < nx; ++c) s = fma(As[c + (size_t)a * nx], gam[nx + c], s);
            if (Ar.d_x0) glw(Ar.d_x0)[row * nx + a] = -s;
        }
        for (int j = lane; j < nu; j += 64) if (Ar.d_u0) glw(Ar.d_u0)[row * nu + j] = du[j];
        wave_sync();
    }
    if (Ar.flags && lane == 0) glw(Ar.flags)[b] = flag;
}

}  // namespace

int lmpc_bank_sens_launch(const LmpcDev &m, const LmpcBankSensArgs &a, void *stream)
{
    LmpcBankSensDev s{};
    s.a = a;
    s.nx = m.nx; s.nu = m.nu; s.ny = m.ny; s.ph = m.ph; s.nz = m.nz; s.mg = m.mg; s.ldz = m.ldz; s.ldy = m.ldy; s.aw = m.active_words;
    s.term = MPCX_HAS_TERMINAL(m) ? 1 : 0;
    s.R = a.s.jacobian ? m.nu : 1;
    const SensLdsPlan plan = sens_lds_plan(m, 4, [&](int waves, int cap) { return waves * bank_wave_len(cap, m.nx, m.nu, m.ny, m.ph, m.nz); });
    if (plan.cap <= 0) return -2;
    s.cap = plan.cap;
    static LmpcLdsCache configured;
    if (lmpc_raise_dynamic_lds(configured, {reinterpret_cast<const void *>(lmpc_bank_sensitivity)}, plan.bytes) != 0) return -3;
    const int blocks = (a.s.batch + plan.waves - 1) / plan.waves;
    hipLaunchKernelGGL(lmpc_bank_sensitivity, dim3(blocks), dim3(64 * plan.waves), plan.bytes, static_cast<hipStream_t>(stream), s);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mpcx
