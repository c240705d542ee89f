// Gradients of a solved batch of a bank: the gradient of a loss on cmd / the input sequence with respect to the three weight
// matrices, to every bound of the QP and to every entry of A, B, C, Bd, Dd -- of the controller each instance was solved with.
//
// The formulas are 4.9's and 4.10's (lmpc_param_sens.hip, lmpc_model_sens.hip).  A bank's controllers share no operand, so the products with the
// host-built Cq and Xq are restated as 4.8b restates the data gradients: on the working set A, S = Y[A, A], and for the cotangent p on w
//     mu = S^-1 Y[A, 0:nz] p,     q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu,
//     dv_i = q[blk[i] nu + .],    dx_0 = 0, dx_i = A dx_{i-1} + B dv_i,    dy_i = C dx_i                         (bank_rollout, i = 1 .. ph)
// Weights and bounds, with y, v the solve's own seq_output, seq_input (row i of seq_input is v_{min(i + 1, ph)}), v_0 = lastU:
//     dL / dOWeight[j, i]      = - dy_{i+1}[j] (y_{i+1}[j] - yref_i[j])
//     dL / dUWeight[j, i]      = - dv_{i+1}[j] (v_{i+1}[j] - uref_i[j])
//     dL / dDeltaUWeight[j, i] = - (dv_{i+1} - dv_i)[j] (v_{i+1} - v_i - duref_{max(i-1, 0)})[j]
//     a bound of a working row r gets mu_r on the side whose bit is set (the upper one where both are), every other bound zero
// Model, with lambda the optimum's multipliers on A (recomputed: S lambda = -Y[A, 0:nz] grad + [soft rows: row value - violated bound], grad the
// cost's condensed gradient at w* by one backward pass over the optimum's sequences):
//     o_i   = W_i (y_i - yref_{i-1}) + output rows of step i: lambda_r e_comp
//     g_i   = C' o_i + state rows: lambda_r e_comp + scalar rows: lambda_r sX + linear rows: lambda_r Fx[c, :] + [i = ph] P (x_ph - x_T)
//     pi_ph = g_ph,   pi_i = g_i + A' pi_{i+1};        do_i, eta_i the same with (dy_i, dx_i, mu_r) in place of (y_i - yref, x_i - x_T, lambda_r)
//     dL/dA = - sum_i (pi_i dx_{i-1}' + eta_i x_{i-1}'),   dL/dB = - sum_i (pi_i dv_i' + eta_i v_i'),   dL/dC = - sum_i (o_i dx_i' + do_i x_i'),
//     dL/dBd = - sum_i eta_i d_{i-1}',                     dL/dDd = - sum_i do_i d_{i-1}'
//
// One wavefront per instance, the whole kernel without a workgroup barrier; an LDS entry is always touched by the same lane; every lane loop
// strides by 64.  Nothing a recursion over the horizon reads lies in HBM: the model, the optimum's sequences and the stage terms of the cost are
// staged in LDS first.  No floating-point atomics: two launches give the same bits.  The per-controller sums are a second kernel,
// lmpc_bank_grad_reduce, that walks each controller's instances in the caller's order, an entry per thread.
// The working-set decode, the factor of S and the solves on it are lmpc_sens_common.hpp's, the roll-out lmpc_bank_common.hpp's.
#include "lmpc_bank_common.hpp"

namespace mpcx {

namespace {

struct LmpcBankGradDev {
    LmpcBankGradArgs a;
    int nx, nu, ny, ndu, ph, nz, mg, ldz, ldy, aw, term, m_rows;      // controller 0's: the same for every controller of a bank
    int cap;                                             // rows of S a wavefront's LDS slice holds
    int model;                                           // a model output is asked for: the slice has the second pass's arrays
};

// a wavefront's slice: [S (packed lower triangle) | its original diagonal], and once mu and lambda are solved pi, eta [ph x nx] in the same place |
// mu | lambda | the working set's unified indices, output slots and the kind, step and component of its general rows (ints) | blk (ints) |
// A, B, C | p, q | dx [(ph + 1) x nx] | do [ph x ny]; for the model outputs besides: x [(ph + 1) x nx] | v [(ph + 1) x nu] | the cost's
// condensed gradient | the input terms of its stages [ph x nu] | two state vectors of the backward pass and x_ph - x_T | o [ph x ny]
__host__ __device__ inline size_t bank_grad_wave_len(int cap, int nx, int nu, int ny, int ph, int nz, bool model)
{
    const size_t fac = (size_t)cap * (cap + 1) / 2 + cap, cos = model ? 2 * (size_t)ph * nx : 0;
    size_t len = (fac > cos ? fac : cos) + 2 * (size_t)cap + 3 * (size_t)cap + (size_t)(ph + 2) / 2 + (size_t)nx * (nx + nu) + (size_t)ny * nx +
                 2 * (size_t)bank_even(nz) + (size_t)(ph + 1) * nx + (size_t)ph * ny;
    if (model) len += (size_t)(ph + 1) * (nx + nu) + (size_t)bank_even(nz) + (size_t)ph * nu + 3 * (size_t)nx + (size_t)ph * ny;
    return len;
}

__global__ __launch_bounds__(256) void lmpc_bank_gradient(const LmpcBankGradDev Gd)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;       // one instance per wavefront; the grid covers the batch
    const LmpcBankGradArgs &Ar = Gd.a;
    if (b >= Ar.batch) return;                                            // (a whole wavefront: the kernel has no workgroup barrier)
    const int nx = Gd.nx, nu = Gd.nu, ny = Gd.ny, ndu = Gd.ndu, ph = Gd.ph, nz = Gd.nz, mg = Gd.mg, ldz = Gd.ldz, ldy = Gd.ldy, aw = Gd.aw;
    const int cap = Gd.cap, m_rows = Gd.m_rows, nzp = bank_even(nz);
    const bool model = Gd.model != 0, term = Gd.term != 0;
    const int nA = nx * nx, nB = nx * nu, nC = ny * nx, nBd = nx * ndu, nDd = ny * ndu, nOW = ny * ph, nUW = nu * ph;
    const size_t n1 = (size_t)ph + 1;
    const double qnan = __builtin_nan("");

    double *S = smem + (size_t)wave * bank_grad_wave_len(cap, nx, nu, ny, ph, nz, model);
    double *dg = S + (size_t)cap * (cap + 1) / 2;
    const size_t fac = (size_t)cap * (cap + 1) / 2 + cap, cos = model ? 2 * (size_t)ph * nx : 0;
    double *V = S + (fac > cos ? fac : cos), *R = V + cap;
    int *idx = reinterpret_cast<int *>(R + cap), *tgt = idx + cap, *rkind = tgt + cap, *rstep = rkind + cap, *rcomp = rstep + cap;
    int *blk = reinterpret_cast<int *>(R + 4 * (size_t)cap);
    double *As = R + 4 * (size_t)cap + (size_t)(ph + 2) / 2, *Bs = As + nA, *Cs = Bs + nB;
    double *pv = Cs + nC, *qv = pv + nzp;
    double *dx = qv + nzp, *dov = dx + n1 * nx;
    // the second pass's arrays (model outputs only)
    double *Xs = dov + (size_t)ph * ny, *vs = Xs + n1 * nx, *grad = vs + n1 * nu, *gu = grad + nzp;
    double *c0 = gu + (size_t)ph * nu, *c1 = c0 + nx, *xt = c1 + nx, *ov = xt + nx;
    double *pi = S, *eta = S + (size_t)ph * nx;           // where S and its diagonal were, once mu and lambda are solved

    // the instance's controller; an index outside the bank is answered like an instance that was not solved
    const int km = __builtin_amdgcn_readfirstlane(Ar.n_models <= 0 ? 0 : (Ar.model_index ? (int)gl(Ar.model_index)[b] : b));
    const bool known = km >= 0 && km < (Ar.n_models > 0 ? Ar.n_models : 1);
    const LmpcDev &M = Ar.models[known ? km : 0];
    int flag = (!known || (Ar.status && gl(Ar.status)[b] != 0)) ? 1 : 0;
    int n = 0;
    if (!flag) {
        // (tgt: the bound that takes the row's mu, the upper one where both bits are set)
        n = sens_working_set(M, gl(Ar.active_lower) + (size_t)b * aw, gl(Ar.active_upper) + (size_t)b * aw, aw, nz, mg, ldz, cap, lane, idx, tgt);
        if (n > cap) flag = 3;
    }
    wave_sync();
    const gdp Y = GP(Y);
    if (!flag) {
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
    if (Ar.flags && lane == 0) glw(Ar.flags)[b] = flag;

    // row b of an output that was asked for
    auto fill = [&](double *out, int len, double v) {
        if (out) for (int t = lane; t < len; t += 64) glw(out)[(size_t)b * len + t] = v;
    };
    if (flag) {
        fill(Ar.d_oweight, nOW, qnan); fill(Ar.d_uweight, nUW, qnan); fill(Ar.d_duweight, nUW, qnan);
        fill(Ar.d_lower, m_rows, qnan); fill(Ar.d_upper, m_rows, qnan);
        fill(Ar.d_A, nA, qnan); fill(Ar.d_B, nB, qnan); fill(Ar.d_C, nC, qnan); fill(Ar.d_Bd, nBd, qnan); fill(Ar.d_Dd, nDd, qnan);
        return;
    }

    // ---- the cotangent on w: the seeds scattered through blk
    for (int t = lane; t < nzp; t += 64) pv[t] = t < nz ? sens_seed(Ar.seed_cmd, Ar.seed_input, blk, nu, ph, b, t) : 0.0;
    wave_sync();
    // ---- mu = S^-1 Y[A, 0:nz] p, a row per lane (Y is symmetric: row idx[i] of a column)
    for (int i = lane; i < n; i += 64) V[i] = sens_rhs(Y, ldy, nz, idx[i], [&](int q) { return pv[q]; });
    wave_sync();
    sens_chol_solve(S, V, n, lane);
    // ---- q = Y[0:nz, 0:nz] p - Y[0:nz, A] mu: a lane owns element pairs of the contiguous columns, one 16-byte load each (ldy is even)
    for (int e = 2 * lane; e < nz; e += 128) {
        double s0 = 0.0, s1 = 0.0;
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
    // ---- forward: the direction through the instance's model, dx and do_i = Wy_i C dx_i
    bank_rollout(As, Bs, Cs, GP(Wy), blk, qv, nx, nu, ny, ph, lane, dx, dov);

    // the references in the solved batch's modes; a null array is the controller's own
    const gdp yr = gl(Ar.yref ? Ar.yref : M.yref_s), ur = gl(Ar.uref ? Ar.uref : M.uref_s), dr = gl(Ar.duref ? Ar.duref : M.duref_s);
    const gdp dm = gl(Ar.dmeas ? Ar.dmeas : M.dmeas_s);
    const gdp sqy = gl(Ar.seq_output), sqv = gl(Ar.seq_input), u0p = gl(Ar.u0);

    // ---- the bounds: every entry of a requested row written once, mu_r in the slot of a working row, zero everywhere else
    if (Ar.d_lower || Ar.d_upper)
        for (int r = lane; r < m_rows; r += 64) {
            double lo = 0.0, up = 0.0;
            for (int i = 0; i < n; ++i) {
                const int t = tgt[i];
                if ((t >> 1) == r) { if (t & 1) up = V[i]; else lo = V[i]; }
            }
            if (Ar.d_lower) glw(Ar.d_lower)[(size_t)b * m_rows + r] = lo;
            if (Ar.d_upper) glw(Ar.d_upper)[(size_t)b * m_rows + r] = up;
        }
    // ---- the weights, [rows x ph] column-major: the setters' layout
    if (Ar.d_oweight)
        for (int t = lane; t < nOW; t += 64) {
            const int i = t / ny, j = t - i * ny;
            const double *xi = dx + (size_t)(i + 1) * nx;
            double dy = 0.0;
#pragma unroll 4
            for (int c = 0; c < nx; ++c) dy = fma(Cs[j + (size_t)c * ny], xi[c], dy);
            glw(Ar.d_oweight)[(size_t)b * nOW + t] = -dy * (sqy[((size_t)b * n1 + i + 1) * ny + j] - ref_at(yr, Ar.yref_bs, Ar.yref_ks, b, i, j));
        }
    if (Ar.d_uweight || Ar.d_duweight)
        for (int t = lane; t < nUW; t += 64) {
            const int i = t / nu, j = t - i * nu;
            const double dn = qv[blk[i + 1] * nu + j], dp = i > 0 ? qv[blk[i] * nu + j] : 0.0;
            const double vn = sqv[((size_t)b * n1 + i) * nu + j];
            const double vp = i > 0 ? sqv[((size_t)b * n1 + i - 1) * nu + j] : u0p[(size_t)b * nu + j];
            if (Ar.d_uweight) glw(Ar.d_uweight)[(size_t)b * nUW + t] = -dn * (vn - ref_at(ur, Ar.uref_bs, Ar.uref_ks, b, i, j));
            if (Ar.d_duweight)      // (duref is read one column late from i = 1, as the assembly of the linear term reads it)
                glw(Ar.d_duweight)[(size_t)b * nUW + t] = -(dn - dp) * (vn - vp - ref_at(dr, Ar.duref_bs, Ar.duref_ks, b, i > 0 ? i - 1 : 0, j));
        }
    if (!model) return;

    // ==== the model: the optimum's sequences and the stage terms of the cost into LDS
    const gdp sqx = gl(Ar.seq_state);
    const gdp Wy = GP(Wy), Wu = GP(Wu), Wdu = GP(Wdu), sX = GP(sX), sU = GP(sU), gsoft = gl(MPCX_G_SOFT(M));
    const gdp tP = gl(MPCX_TERMINAL(M)), tXT = tP + nA, tTx = tXT + nx;
    const gdp Flin = gl(MPCX_LINEAR_F(M));
    for (int t = lane; t < (int)n1 * nx; t += 64) Xs[t] = sqx[(size_t)b * n1 * nx + t];
    // v_0 = lastU, v_i = row i - 1 of the sequence
    for (int t = lane; t < (int)n1 * nu; t += 64) vs[t] = t < nu ? u0p[(size_t)b * nu + t] : sqv[(size_t)b * n1 * nu + t - nu];
    for (int t = lane; t < ph * ny; t += 64) {
        const int i = t / ny + 1, j = t - (i - 1) * ny;
        ov[t] = Wy[j + (size_t)i * ny] * (sqy[((size_t)b * n1 + i) * ny + j] - ref_at(yr, Ar.yref_bs, Ar.yref_ks, b, i - 1, j));
    }
    for (int t = lane; t < nzp; t += 64) grad[t] = 0.0;
    for (int a = lane; a < nx; a += 64) {
        c0[a] = 0.0;
        double s = 0.0;
        if (term) {           // x_ph - x_T, x_T = xT + Tx [yref_{ph-1}; d_{ph-1}]
            s = tXT[a];
            for (int j = 0; j < ny; ++j) s = fma(tTx[a + (size_t)j * nx], ref_at(yr, Ar.yref_bs, Ar.yref_ks, b, ph - 1, j), s);
            for (int d = 0; d < ndu; ++d) s = fma(tTx[a + (size_t)(ny + d) * nx], ref_at(dm, Ar.dmeas_bs, Ar.dmeas_ks, b, ph - 1, d), s);
            s = sqx[((size_t)b * n1 + ph) * nx + a] - s;
        }
        xt[a] = s;
    }
    wave_sync();
    // the input term of stage i = 1 .. ph: Wu_i (v_i - uref_{i-1}) + r_{i-1} - r_i, r_i the rate term of the increment v_{i+1} - v_i
    auto rate = [&](int i, int j) -> double {
        return Wdu[j + (size_t)i * nu] * (vs[(i + 1) * nu + j] - vs[i * nu + j] - ref_at(dr, Ar.duref_bs, Ar.duref_ks, b, i > 0 ? i - 1 : 0, j));
    };
    for (int t = lane; t < ph * nu; t += 64) {
        const int i = t / nu + 1, j = t - (i - 1) * nu;
        double s = Wu[j + (size_t)i * nu] * (vs[i * nu + j] - ref_at(ur, Ar.uref_bs, Ar.uref_ks, b, i - 1, j)) + rate(i - 1, j);
        if (i < ph) s -= rate(i, j);
        gu[t] = s;
    }
    wave_sync();
    if (n > 0) {
        // ---- the cost's condensed gradient at the optimum: one backward pass, every operand in LDS
        double *cp = c0, *cn = c1;
        for (int i = ph; i >= 1; --i) {
            const double *ey = ov + (size_t)(i - 1) * ny;
            for (int a = lane; a < nx; a += 64) {
                double s = 0.0;
                for (int j = 0; j < ny; ++j) s = fma(Cs[j + (size_t)a * ny], ey[j], s);
                if (i < ph) for (int c = 0; c < nx; ++c) s = fma(As[c + (size_t)a * nx], cp[c], s);
                else if (term) for (int c = 0; c < nx; ++c) s = fma(tP[a + (size_t)c * nx], xt[c], s);
                cn[a] = s;
            }
            wave_sync();
            for (int j = lane; j < nu; j += 64) {
                double s = gu[(i - 1) * nu + j];
                for (int a = 0; a < nx; ++a) s = fma(Bs[a + (size_t)j * nx], cn[a], s);
                grad[blk[i] * nu + j] += s;
            }
            double *sw = cp; cp = cn; cn = sw;
            wave_sync();
        }
        // ---- S lambda = -Y[A, 0:nz] grad, and on a soft row its violation besides; the factor of S serves a second time
        for (int k = lane; k < n; k += 64) {
            const int qi = idx[k];
            double s = 0.0;
            for (int q = 0; q < nz; ++q) s = fma(-Y[(size_t)q * ldy + qi], grad[q], s);
            const int rr = qi - ldz;
            if (rr >= 0 && gsoft[rr] > 0.0) {
                const int kind = rkind[k], st = rstep[k], cpn = rcomp[k];
                const double *xs = Xs + (size_t)st * nx, *vt = vs + (size_t)st * nu;
                double v = 0.0;
                if (kind == G_STATE) v = xs[cpn];
                else if (kind == G_OUTPUT) v = sqy[((size_t)b * n1 + st) * ny + cpn];
                else if (kind == G_SCALAR) {
                    for (int c = 0; c < nx; ++c) v = fma(sX[c], xs[c], v);
                    for (int j = 0; j < nu; ++j) v = fma(sU[j], vt[j], v);
                } else if (kind == G_LINEAR) {
                    const gdp F = Flin + (size_t)cpn * (nx + nu);
                    for (int c = 0; c < nx; ++c) v = fma(F[c], xs[c], v);
                    for (int j = 0; j < nu; ++j) v = fma(F[nx + j], vt[j], v);
                } else v = vt[cpn] - (st > 0 ? vt[cpn - nu] : 0.0);
                s += v - ((tgt[k] & 1) ? GP(ug0)[rr] : GP(lg0)[rr]);
            }
            R[k] = s;
        }
        wave_sync();
        sens_chol_solve(S, R, n, lane);
    }
    wave_sync();
    // ---- S is dead: the stage gradients of the two costates take its place, the working rows one after the other
    for (int t = lane; t < ph * nx; t += 64) { pi[t] = 0.0; eta[t] = 0.0; }
    wave_sync();
    for (int k = 0; k < n; ++k) {
        const int kind = rkind[k], st = rstep[k], cpn = rcomp[k];
        if (kind < 0 || st < 1) continue;
        const double lam = R[k], mu = V[k];
        if (kind == G_OUTPUT) { if (lane == (cpn & 63)) { ov[(st - 1) * ny + cpn] += lam; dov[(st - 1) * ny + cpn] += mu; } }
        else if (kind == G_STATE) { if (lane == (cpn & 63)) { pi[(st - 1) * nx + cpn] += lam; eta[(st - 1) * nx + cpn] += mu; } }
        else if (kind == G_SCALAR || kind == G_LINEAR) {
            const gdp F = kind == G_SCALAR ? sX : Flin + (size_t)cpn * (nx + nu);
            for (int c = lane; c < nx; c += 64) { pi[(st - 1) * nx + c] = fma(lam, F[c], pi[(st - 1) * nx + c]); eta[(st - 1) * nx + c] = fma(mu, F[c], eta[(st - 1) * nx + c]); }
        }
    }
    wave_sync();
    // ---- the two costates side by side
    const double *dxph = dx + (size_t)ph * nx;
    for (int i = ph; i >= 1; --i) {
        double *pc = pi + (size_t)(i - 1) * nx, *ec = eta + (size_t)(i - 1) * nx;
        const double *oc = ov + (size_t)(i - 1) * ny, *dc = dov + (size_t)(i - 1) * ny;
        for (int a = lane; a < nx; a += 64) {
            double s = pc[a], e = ec[a];
            for (int j = 0; j < ny; ++j) { s = fma(Cs[j + (size_t)a * ny], oc[j], s); e = fma(Cs[j + (size_t)a * ny], dc[j], e); }
            if (i < ph)
                for (int c = 0; c < nx; ++c) { s = fma(As[c + (size_t)a * nx], pc[nx + c], s); e = fma(As[c + (size_t)a * nx], ec[nx + c], e); }
            else if (term)
                for (int c = 0; c < nx; ++c) { s = fma(tP[a + (size_t)c * nx], xt[c], s); e = fma(tP[a + (size_t)c * nx], dxph[c], e); }
            pc[a] = s; ec[a] = e;
        }
        wave_sync();
    }
    // ---- the outer-product sums, an entry per lane, column-major: the setters' layout
    const int glen = nA + nB + nC + nBd + nDd;
    for (int t = lane; t < glen; t += 64) {
        const int kind = t < nA ? 0 : (t < nA + nB ? 1 : (t < nA + nB + nC ? 2 : (t < nA + nB + nC + nBd ? 3 : 4)));
        const int tt = t - (kind == 0 ? 0 : (kind == 1 ? nA : (kind == 2 ? nA + nB : (kind == 3 ? nA + nB + nC : nA + nB + nC + nBd))));
        const int rows = (kind == 2 || kind == 4) ? ny : nx, c = tt / rows, r = tt - c * rows;
        const int len = kind == 0 ? nA : (kind == 1 ? nB : (kind == 2 ? nC : (kind == 3 ? nBd : nDd)));
        double *out = kind == 0 ? Ar.d_A : (kind == 1 ? Ar.d_B : (kind == 2 ? Ar.d_C : (kind == 3 ? Ar.d_Bd : Ar.d_Dd)));
        if (!out) continue;
        double s = 0.0;
        for (int i = 1; i <= ph; ++i) {
            if (kind == 0) {
                s = fma(eta[(i - 1) * nx + r], Xs[(size_t)(i - 1) * nx + c], s);
                if (i > 1) s = fma(pi[(i - 1) * nx + r], dx[(size_t)(i - 1) * nx + c], s);
            } else if (kind == 1) {
                s = fma(eta[(i - 1) * nx + r], vs[i * nu + c], s);
                s = fma(pi[(i - 1) * nx + r], qv[blk[i] * nu + c], s);
            } else if (kind == 2) {
                s = fma(dov[(i - 1) * ny + r], Xs[(size_t)i * nx + c], s);
                s = fma(ov[(i - 1) * ny + r], dx[(size_t)i * nx + c], s);
            } else if (kind == 3) s = fma(eta[(i - 1) * nx + r], ref_at(dm, Ar.dmeas_bs, Ar.dmeas_ks, b, i - 1, c), s);
            else s = fma(dov[(i - 1) * ny + r], ref_at(dm, Ar.dmeas_bs, Ar.dmeas_ks, b, i - 1, c), s);
        }
        glw(out)[(size_t)b * len + tt] = -s;
    }
}

// The per-controller sums: row k of a c_* array is the sum of the d_* rows of controller k's instances whose flag is 0, added in the order of
// order[offsets[k] .. offsets[k + 1]) -- an entry per thread, no floating-point atomics, the same bits on every launch.  Entries [end[s - 1], end[s])
// of a controller's row belong to output s (one that is not asked for ends where the one before it does); the entry behind the last counts the
// instances that contributed.  Whether an instance contributed: its flag where the caller has the flags written, otherwise whether the first entry
// of its row of `probe` is a number (a flagged instance's rows are NaN throughout)
constexpr int kBankGradOuts = 10;
struct BankGradReduce {
    const double *src[kBankGradOuts];
    double *dst[kBankGradOuts];
    int len[kBankGradOuts];
    size_t end[kBankGradOuts];
    const int32_t *flags;
    const double *probe; size_t probe_len;
    const int32_t *order, *offsets;
    int32_t *n_used;
    int K, batch;
};

__global__ __launch_bounds__(256) void lmpc_bank_grad_reduce(const BankGradReduce R)
{
    const size_t rowlen = R.end[kBankGradOuts - 1], per = rowlen + 1;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)R.K * per) return;
    const int k = (int)(t / per);
    const size_t e = t - (size_t)k * per;
    const bool count = e == rowlen;
    const double *src = nullptr;
    double *dst = nullptr;
    size_t first = 0;
    int len = 0;
#pragma unroll
    for (int s = kBankGradOuts - 1; s >= 0; --s)
        if (e < R.end[s]) { src = R.src[s]; dst = R.dst[s]; len = R.len[s]; first = s > 0 ? R.end[s - 1] : 0; }
    if (count ? !R.n_used : !dst) return;
    int p0 = gl(R.offsets)[k], p1 = gl(R.offsets)[k + 1];
    p0 = p0 < 0 ? 0 : p0; p1 = p1 > R.batch ? R.batch : p1;
    double sum = 0.0;
    int used = 0;
    for (int p = p0; p < p1; ++p) {
        const int b = gl(R.order)[p];
        if (b < 0 || b >= R.batch) continue;
        bool ok;
        if (R.flags) ok = gl(R.flags)[b] == 0;
        else { const double v = gl(R.probe)[(size_t)b * R.probe_len]; ok = v == v; }
        if (!ok) continue;
        ++used;
        if (!count) sum += gl(src)[(size_t)b * len + (e - first)];
    }
    if (count) glw(R.n_used)[k] = used;
    else glw(dst)[(size_t)k * len + (e - first)] = sum;
}

}  // namespace

int lmpc_bank_grad_launch(const LmpcDev &m, const LmpcBankGradArgs &a, void *stream)
{
    LmpcBankGradDev s{};
    s.a = a;
    if (m.ndu <= 0) { s.a.d_Bd = s.a.d_Dd = nullptr; s.a.c_Bd = s.a.c_Dd = nullptr; }
    s.nx = m.nx; s.nu = m.nu; s.ny = m.ny; s.ndu = m.ndu; s.ph = m.ph; s.nz = m.nz; s.mg = m.mg; s.ldz = m.ldz; s.ldy = m.ldy; s.aw = m.active_words;
    s.term = MPCX_HAS_TERMINAL(m) ? 1 : 0;
    s.m_rows = m.m_ref;
    s.model = (s.a.d_A || s.a.d_B || s.a.d_C || s.a.d_Bd || s.a.d_Dd) ? 1 : 0;
    const bool model = s.model != 0;
    const SensLdsPlan plan = sens_lds_plan(m, 4, [&](int waves, int cap) { return waves * bank_grad_wave_len(cap, m.nx, m.nu, m.ny, m.ph, m.nz, model); });
    if (plan.cap <= 0) return -2;
    s.cap = plan.cap;
    static LmpcLdsCache configured;
    if (lmpc_raise_dynamic_lds(configured, {reinterpret_cast<const void *>(lmpc_bank_gradient)}, plan.bytes) != 0) return -3;
    const int blocks = (a.batch + plan.waves - 1) / plan.waves;
    hipLaunchKernelGGL(lmpc_bank_gradient, dim3(blocks), dim3(64 * plan.waves), plan.bytes, static_cast<hipStream_t>(stream), s);
    if (hipGetLastError() != hipSuccess) return -3;

    const LmpcBankGradArgs &g = s.a;
    double *const dst[kBankGradOuts] = {g.c_oweight, g.c_uweight, g.c_duweight, g.c_lower, g.c_upper, g.c_A, g.c_B, g.c_C, g.c_Bd, g.c_Dd};
    const double *const src[kBankGradOuts] = {g.d_oweight, g.d_uweight, g.d_duweight, g.d_lower, g.d_upper, g.d_A, g.d_B, g.d_C, g.d_Bd, g.d_Dd};
    const int len[kBankGradOuts] = {m.ny * m.ph, m.nu * m.ph, m.nu * m.ph, m.m_ref, m.m_ref, m.nx * m.nx, m.nx * m.nu, m.ny * m.nx, m.nx * m.ndu, m.ny * m.ndu};
    BankGradReduce r{};
    size_t end = 0;
    bool any = g.n_used != nullptr;
    for (int k = 0; k < kBankGradOuts; ++k) {
        r.src[k] = src[k]; r.dst[k] = dst[k]; r.len[k] = len[k];
        if (dst[k]) {
            if (!src[k]) return -3;                    // (the sums read the per-instance rows)
            end += (size_t)len[k]; any = true;
        }
        r.end[k] = end;
        if (src[k] && !r.probe && len[k] > 0) { r.probe = src[k]; r.probe_len = (size_t)len[k]; }
    }
    if (!any) return 0;
    if (!g.group_order || !g.group_offsets || g.n_models < 1 || (!g.flags && !r.probe)) return -3;
    r.flags = g.flags; r.order = g.group_order; r.offsets = g.group_offsets; r.n_used = g.n_used; r.K = g.n_models; r.batch = g.batch;
    const size_t total = (size_t)r.K * (end + 1);
    hipLaunchKernelGGL(lmpc_bank_grad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), r);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mpcx
