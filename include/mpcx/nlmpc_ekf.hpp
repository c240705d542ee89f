// Output feedback for the closed loop around the batched NLMPC solve (mpcx_nlmpc_loop_create_observed, mpcx_nlmpc_ekf_step_batch,
// include/mpcx.h): an extended Kalman filter in the advance step.  The solve of tick k reads the estimate xhat_k (it is the loop's x
// buffer); the advance step moves the truth, measures it and updates the estimate and its covariance, all from tick-k data:
//
//   x_{k+1}  = Phi(x_k, cmd_k, p_plant) + w_k                    Phi: loop_plant_reg of mpcx/nlmpc_loop.hpp, the step without noise
//   y_{k+1}  = Cm x_{k+1} + v_k
//   xhat-    = Phi(xhat_k, cmd_k, p_ctrl)
//   F[:, j]  = (Phi(xhat_k + h_j e_j) - Phi(xhat_k - h_j e_j)) / (x+_j - x-_j),   h_j = 2^-17 max(1, |xhat_k,j|); the divisor is the
//              difference of the two perturbed values as stored
//   P-       = F P_k F' + Q
//   S        = Cm P- Cm' + R,  K = P- Cm' S^-1 (Cholesky of S)
//   xhat_{k+1} = xhat- + K (y_{k+1} - Cm xhat-)
//   P_{k+1}  = sym((I - K Cm) P- (I - K Cm)' + K R K')          Joseph form, then (P + P') / 2
//
// A pivot of S that is not > 0 or not finite (tested before the square root and before any division) skips the update of that tick:
// xhat_{k+1} = xhat-, P_{k+1} = sym(P-), bit 0 of the instance's flag word is set.
//
// Shape.  An instance is a group of G = 2 NX + 2 adjacent lanes of the block's one wavefront (64 / G instances per block).  Every lane
// evaluates Phi ONCE, at its own point, through one call site: lane 0 the truth with the plant's parameters, lane 1 xhat_k, lanes
// 2 + 2j and 3 + 2j xhat_k +- h_j e_j.  One instruction stream: equal inputs give equal bits whatever the compiler fuses, so that
// without noise and mismatch the estimate IS the truth, bit for bit.  Everything after Phi is spelled with explicit fma: no product
// is left for the compiler to contract one way here and another way there.  F, P, P-, Cm P-, S and K live in the group's LDS slice
// with an odd leading dimension (and an odd slice length: the lanes of different instances start in different banks); the products
// are FMA loops with compile-time NX, spread over 2 NX lanes (a row and half of its columns each); ny is a run-time value <= NX.
// The Cholesky factorisation runs right-looking on the group's lanes, two wave barriers per column; its verdict is read by every
// lane from the same LDS words, hence group-uniform.  Lanes whose slot holds no instance (the wavefront's tail, the last block's
// surplus) run along on the last instance's inputs and store nothing to memory: every lane of the wavefront reaches every barrier.
// No register array has a run-time subscript, there is no scratch, every store is an ordinary vector store.
//
// As in mpcx/nlmpc_loop.hpp the bodies take the tick as an argument and run unchanged in the lock-step interpreter of tests/emu.
#pragma once

#include "nlmpc_loop.hpp"

namespace mpcx {

// the filter of an observed loop, next to NlmpcLoopDev (whose x is the estimate: what the solve reads)
struct NlmpcEkfDev {
    int ny;
    const double *cb;                       // the constant block: Cm [ny x nx] | Q [nx x nx] | R [ny x ny] | P0 [nx x nx], column-major
    const double *xhat0;                    // the caller's [B x nx] or null (x0)
    const double *meas_noise;               // [ticks x B x ny] or null
    double *xt;                             // the truth [B x nx]
    double *P;                              // [B x nx nx]
    double *traj_xhat, *traj_y, *traj_P;    // [(ticks+1) x B x nx], [ticks x B x ny], [(ticks+1) x B x nx nx] or null
    int *flags;                             // [B]
};

namespace engine {

// what one filter step reads and writes, the rows of the tick already picked (the loop's advance step and the stand-alone step fill it)
struct EkfIo {
    int batch, substeps, nparams, ny;
    const double *cm, *q, *r;               // the constant block
    const double *xt;                       // truth [B x nx], or null: no plant in this call (then y is given)
    const double *xhat, *P, *u;             // [B x nx], [B x nx nx], [B x nu]
    const double *p_plant, *p_ctrl;         // [B x nparams] or null (the controller's)
    const double *w, *v, *y;                // [B x nx], [B x ny], [B x ny] or null
    double *xt_out, *traj_x, *u_out, *traj_u;          // with a plant only
    double *xhat_out, *traj_xhat, *P_out, *traj_P, *traj_y;   // the traj_ rows may be null
    int *flags;
    int sticky;                             // 1: a skipped update sets bit 0 and nothing clears it (the loop); 0: the word is written
};

template <int NX> struct EkfLay {
    static_assert(NX % 2 == 0 && NX <= 30, "a group is 2 NX + 2 lanes of one wavefront, a lane takes half a row");
    static constexpr int G = 2 * NX + 2;                // lanes per instance
    static constexpr int IPW = 64 / G;                  // instances per block
    static constexpr int SLOTS = (64 + G - 1) / G;      // ... and slices: the wavefront's tail has one of its own
    static constexpr int LD = NX | 1, MAT = NX * LD;
    static constexpr int F = 0, P = MAT, T = 2 * MAT, PM = 3 * MAT, K = 4 * MAT, S = 5 * MAT;      // F: later I - K Cm; P: later K R; S: later the new P
    static constexpr int XT = 6 * MAT, XM = XT + NX, DM = XM + NX, NU = DM + NX;                   // x_{k+1}, xhat-, x-_j, the innovation
    static constexpr int SLICE = (6 * MAT + 4 * NX) | 1;
    static constexpr int DOUBLES = SLOTS * SLICE;
};

constexpr double kEkfRel = 0x1p-17;         // finite-difference step relative to max(1, |xhat_j|)
constexpr double kEkfHuge = 1.7976931348623157e308;

template <class Mdl>
__device__ __forceinline__ void ekf_group(const NlmpcDev &M, const EkfIo &io, double *lds)
{
    constexpr int NX = Mdl::NX, NU = Mdl::NU, H = NX / 2;
    using Y = EkfLay<NX>;
    constexpr int LD = Y::LD;
    const int lane = (int)threadIdx.x, slot = lane / Y::G, g = lane - slot * Y::G;
    const int braw = (int)blockIdx.x * Y::IPW + slot;
    const bool valid = slot < Y::IPW && braw < io.batch;
    const size_t b = (size_t)min(braw, io.batch - 1);
    const int m = io.ny;
    double *W = lds + slot * Y::SLICE;
    double *F = W + Y::F, *P = W + Y::P, *T = W + Y::T, *Pm = W + Y::PM, *Kt = W + Y::K, *S = W + Y::S;
    double *XT = W + Y::XT, *XM = W + Y::XM, *DM = W + Y::DM, *IN = W + Y::NU;
    const double __attribute__((address_space(1))) *cm = loop_gin(io.cm), *q = loop_gin(io.q), *r = loop_gin(io.r);

    for (int idx = g; idx < NX * NX; idx += Y::G) P[idx % NX + (idx / NX) * LD] = loop_gin(io.P)[b * (NX * NX) + idx];

    // ---- the lane's point, and Phi at it
    const bool truth = g == 0 && io.xt != nullptr;
    const int j = (g - 2) >> 1;             // the perturbed coordinate of lanes >= 2
    const double *src = truth ? io.xt : io.xhat;
    const double *pc = io.p_ctrl ? io.p_ctrl + b * io.nparams : M.params;
    const double *p = truth && io.p_plant ? io.p_plant + b * io.nparams : pc;
    double x[NX], u[NU], xp = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = loop_gin(src)[b * NX + i];
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = loop_gin(io.u)[b * NU + i];
    if (g >= 2) {
#pragma unroll
        for (int i = 0; i < NX; ++i)
            if (i == j) {
                const double h = kEkfRel * fmax(1.0, fabs(x[i]));
                x[i] = (g & 1) ? x[i] - h : x[i] + h;
                xp = x[i];
            }
    }
    loop_plant_reg<Mdl>(M, p, io.substeps, x, u);
    if (truth) {
        if (io.w) {
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] += loop_gin(io.w)[b * NX + i];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) XT[i] = x[i];
        if (valid) {
#pragma unroll
            for (int i = 0; i < NX; ++i) { loop_gout(io.xt_out)[b * NX + i] = x[i]; loop_gout(io.traj_x)[b * NX + i] = x[i]; }
#pragma unroll
            for (int i = 0; i < NU; ++i) { loop_gout(io.u_out)[b * NU + i] = u[i]; loop_gout(io.traj_u)[b * NU + i] = u[i]; }
        }
    }
    if (g == 1) {
#pragma unroll
        for (int i = 0; i < NX; ++i) XM[i] = x[i];
    }
    if (g >= 2 && (g & 1)) {                // the minus column waits in P-'s place
#pragma unroll
        for (int i = 0; i < NX; ++i) Pm[i + j * LD] = x[i];
        DM[j] = xp;
    }
    nl_wave_sync();
    if (g >= 2 && !(g & 1)) {
        const double den = xp - DM[j];
#pragma unroll
        for (int i = 0; i < NX; ++i) F[i + j * LD] = (x[i] - Pm[i + j * LD]) / den;
    }
    // ---- the measurement and the innovation: two sums of one spelling, so that Cm x - Cm xhat- is 0 where x and xhat- are the same bits
    if (g < m) {
        double cx = 0.0, yv;
#pragma unroll
        for (int l = 0; l < NX; ++l) cx = fma(cm[g + l * m], XM[l], cx);
        if (io.xt) {
            yv = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) yv = fma(cm[g + l * m], XT[l], yv);
            if (io.v) yv += loop_gin(io.v)[b * m + g];
        } else {
            yv = loop_gin(io.y)[b * m + g];
        }
        IN[g] = yv - cx;
        if (valid && io.traj_y) loop_gout(io.traj_y)[b * m + g] = yv;
    }
    nl_wave_sync();

    // ---- P- = F P F' + Q: lane g < 2 NX takes row g / 2 and half of its columns
    const int row = g >> 1, c0 = (g & 1) * H;
    const bool worker = g < 2 * NX;
    if (worker) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = fma(F[row + l * LD], P[l + c * LD], acc);
            T[row + c * LD] = acc;
        }
    }
    nl_wave_sync();
    if (worker) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            double acc = q[row + c * NX];
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = fma(T[row + l * LD], F[c + l * LD], acc);
            Pm[row + c * LD] = acc;
        }
    }
    nl_wave_sync();
    // ---- Cm P- [m x NX] (in K's place), S = Cm P- Cm' + R
    if (worker && row < m) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = fma(cm[row + l * m], Pm[l + c * LD], acc);
            Kt[row + c * LD] = acc;
        }
    }
    nl_wave_sync();
    if (worker && row < m) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            if (c < m) {
                double acc = r[row + c * m];
#pragma unroll
                for (int l = 0; l < NX; ++l) acc = fma(Kt[row + l * LD], cm[c + l * m], acc);
                S[row + c * LD] = acc;
            }
        }
    }
    nl_wave_sync();
    // ---- S = L L', right-looking, lane g < m owns row g; every lane reads every pivot: the verdict is the group's
    bool ok = true;
    for (int kk = 0; kk < m; ++kk) {
        const double piv = S[kk + kk * LD];
        const bool good = piv > 0.0 && piv <= kEkfHuge;
        ok = ok && good;
        const double d = good ? sqrt(piv) : 1.0;
        double lrk = 0.0;
        if (g > kk && g < m) { lrk = S[g + kk * LD] / d; S[g + kk * LD] = lrk; }
        nl_wave_sync();
        if (g == kk) S[kk + kk * LD] = d;
        if (g > kk && g < m)
            for (int c = kk + 1; c <= g; ++c) S[g + c * LD] = fma(-lrk, S[c + kk * LD], S[g + c * LD]);
        nl_wave_sync();
    }
    // ---- K' = S^-1 (Cm P-): lane g < NX solves its own column in place
    if (g < NX) {
        for (int i = 0; i < m; ++i) {
            double t = Kt[i + g * LD];
            for (int s = 0; s < i; ++s) t = fma(-S[i + s * LD], Kt[s + g * LD], t);
            Kt[i + g * LD] = t / S[i + i * LD];
        }
        for (int i = m - 1; i >= 0; --i) {
            double t = Kt[i + g * LD];
            for (int s = i + 1; s < m; ++s) t = fma(-S[s + i * LD], Kt[s + g * LD], t);
            Kt[i + g * LD] = t / S[i + i * LD];
        }
    }
    nl_wave_sync();
    // ---- the estimate
    if (g < NX) {
        double acc = XM[g];
        for (int s = 0; s < m; ++s) acc = fma(Kt[s + g * LD], IN[s], acc);
        const double v = ok ? acc : XM[g];
        if (valid) {
            loop_gout(io.xhat_out)[b * NX + g] = v;
            if (io.traj_xhat) loop_gout(io.traj_xhat)[b * NX + g] = v;
        }
    }
    // ---- Joseph form: A = I - K Cm (in F's place), K R (in P's place), A P- (in T's place), A P- A' + K R K' (in S's place)
    if (worker) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            double acc = row == c ? 1.0 : 0.0;
            for (int s = 0; s < m; ++s) acc = fma(-Kt[s + row * LD], cm[s + c * m], acc);
            F[row + c * LD] = acc;
            if (c < m) {
                double kr = 0.0;
                for (int s = 0; s < m; ++s) kr = fma(Kt[s + row * LD], r[s + c * m], kr);
                P[row + c * LD] = kr;
            }
        }
    }
    nl_wave_sync();
    if (worker) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = fma(F[row + l * LD], Pm[l + c * LD], acc);
            T[row + c * LD] = acc;
        }
    }
    nl_wave_sync();
    if (worker) {
        for (int cc = 0; cc < H; ++cc) {
            const int c = c0 + cc;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = fma(T[row + l * LD], F[c + l * LD], acc);
            for (int s = 0; s < m; ++s) acc = fma(P[row + s * LD], Kt[s + c * LD], acc);
            S[row + c * LD] = acc;
        }
    }
    nl_wave_sync();
    const double *N = ok ? S : Pm;
    for (int idx = g; idx < NX * NX; idx += Y::G) {
        const int i = idx % NX, c = idx / NX;
        const double v = 0.5 * (N[i + c * LD] + N[c + i * LD]);
        if (valid) {
            loop_gout(io.P_out)[b * (NX * NX) + idx] = v;
            if (io.traj_P) loop_gout(io.traj_P)[b * (NX * NX) + idx] = v;
        }
    }
    if (g == 0 && valid) {
        if (!io.sticky) loop_gout(io.flags)[b] = ok ? 0 : 1;
        else if (!ok) loop_gout(io.flags)[b] = loop_gin(io.flags)[b] | 1;
    }
}

// tick k of the block's instances of an observed loop: the caller has made sure that k < L.ticks
template <class Mdl>
__device__ __forceinline__ void ekf_advance_tile(const NlmpcDev &M, const NlmpcLoopDev &L, const NlmpcEkfDev &E, const int k, double *lds)
{
    constexpr int NX = Mdl::NX, NU = Mdl::NU;
    using Y = EkfLay<NX>;
    const size_t B = (size_t)L.batch, at = (size_t)k * B, m = (size_t)E.ny;
    EkfIo io;
    io.batch = L.batch; io.substeps = L.substeps; io.nparams = L.nparams; io.ny = E.ny;
    io.cm = E.cb; io.q = E.cb + m * NX; io.r = io.q + NX * NX;
    io.xt = E.xt; io.xhat = L.x; io.P = E.P; io.u = L.cmd;
    io.p_plant = L.plant_params ? L.plant_params : L.params; io.p_ctrl = L.params;
    io.w = L.noise ? L.noise + at * NX : nullptr; io.v = E.meas_noise ? E.meas_noise + at * m : nullptr; io.y = nullptr;
    io.xt_out = E.xt; io.traj_x = L.traj_x + (at + B) * NX; io.u_out = L.u; io.traj_u = L.traj_u + at * NU;
    io.xhat_out = L.x; io.traj_xhat = E.traj_xhat + (at + B) * NX; io.P_out = E.P;
    io.traj_P = E.traj_P ? E.traj_P + (at + B) * (NX * NX) : nullptr; io.traj_y = E.traj_y + at * m;
    io.flags = E.flags; io.sticky = 1;
    ekf_group<Mdl>(M, io, lds);
    const int lane = (int)threadIdx.x, slot = lane / Y::G, b = (int)blockIdx.x * Y::IPW + slot;
    if (lane != slot * Y::G || slot >= Y::IPW || b >= L.batch) return;
    if (L.traj_cost) loop_gout(L.traj_cost)[at + b] = loop_gin(L.cost)[b];
    if (L.traj_status) loop_gout(L.traj_status)[at + b] = loop_gin(L.status)[b];
    if (L.traj_solver_status) loop_gout(L.traj_solver_status)[at + b] = loop_gin(L.solver_status)[b];
    if (L.traj_is_feasible) loop_gout(L.traj_is_feasible)[at + b] = loop_gin(L.is_feasible)[b];
    if (L.traj_iterations) loop_gout(L.traj_iterations)[at + b] = loop_gin(L.iterations)[b];
}

// the filter step alone (mpcx_nlmpc_ekf_step_batch): the measurement y of the new state is given, there is no plant in the call.
// xhat_next may be xhat and P_next may be P: a group has read its instance's rows before it writes them
template <class Mdl>
__device__ __forceinline__ void ekf_step_tile(const NlmpcDev &M, const int batch, const double *xhat, const double *P, const double *u, const double *y,
                                              const double *params, const int nparams, const double *cb, const int ny, const int substeps,
                                              double *xhat_next, double *P_next, int *flags, double *lds)
{
    constexpr int NX = Mdl::NX;
    EkfIo io;
    io.batch = batch; io.substeps = substeps; io.nparams = nparams; io.ny = ny;
    io.cm = cb; io.q = cb + (size_t)ny * NX; io.r = io.q + NX * NX;
    io.xt = nullptr; io.xhat = xhat; io.P = P; io.u = u;
    io.p_plant = nullptr; io.p_ctrl = params;
    io.w = nullptr; io.v = nullptr; io.y = y;
    io.xt_out = nullptr; io.traj_x = nullptr; io.u_out = nullptr; io.traj_u = nullptr;
    io.xhat_out = xhat_next; io.traj_xhat = nullptr; io.P_out = P_next; io.traj_P = nullptr; io.traj_y = nullptr;
    io.flags = flags; io.sticky = 0;
    ekf_group<Mdl>(M, io, lds);
}

}  // namespace engine
}  // namespace mpcx
