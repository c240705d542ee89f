// The closed loop around the batched LMPC solve (mpcx_lmpc_loop_*, include/mpcx.h): what runs between two solves of a receding-horizon
// run, on the device, so that a tick is "solve, advance" with no host work in between.
//
//   lmpc_loop_begin    x <- x0, u <- u0, row 0 of traj_x, the preview windows of tick 0, tick counter <- 0
//   lmpc_loop_advance  tick k = the counter: x <- A_p x + B_p cmd + Bd_p d_k + w_k, u <- cmd, the tick's row of every trajectory, the
//                      active sets handed to the next solve's warm start, the preview windows of tick k + 1, counter <- k + 1
//
// Shape: one wavefront per block, lane <-> instance of a tile of 64 instances.  The instance-major arrays ([B x n], a tile of them is one
// contiguous run) go through LDS both ways -- global accesses walk the run element by element across the lanes, the lane then reads its own
// instance's row from LDS at an odd stride.  The plant [A_p | B_p | Bd_p] is the same for every lane: it is read through the constant
// address space, i.e. by scalar loads into SGPRs, and feeds the FMAs as a scalar operand.  No register arrays (the dimensions are run-time
// values), hence no scratch.  The tick number is device state: the kernel's arguments are the same at every tick, so a captured graph of one
// tick replays unchanged; a replay with the counter at `ticks` returns before its first store.
//
// Per-instance plants (a Monte-Carlo run over B plants, a bank whose every controller is its own plant) cannot be scalar operands:
//   lmpc_loop_pack_plants     head of every run: the plants, from the caller's array or from the bank's model structs, into the order below; a
//                             bank's "shared" exogenous input (each controller's own) into a [B x ndu] array
//   lmpc_loop_advance_plants  the same tick with lane <-> (instance, state row): a wavefront holds 64 / nx instances, its lanes accumulate their
//                             rows' nx + nu + ndu terms in the uniform kernel's order (the two agree bit for bit on equal plants); term j of a
//                             tile is one contiguous run of the packed array, read by consecutive lanes, the loads of a group of terms in flight
//                             together; the lane's sum is an element of the tile's run of x and goes straight out
//
// Output feedback (an observed loop, mpcx_lmpc_loop_create_observed): the solve reads an estimate xhat instead of the true state x, and the tick
// also measures and estimates, everything from tick-k data (predictor form):
//   y = C x + Dd d_k + v_k,  e = y - (C xhat + Dd d_k),  x <- A_p x + B_p cmd + Bd_p d_k + w_k,  xhat <- A xhat + B cmd + Bd d_k + L e
//   lmpc_loop_pack_observer     head of every run: the estimator [A | B | Bd | L] and the measurement [C | Dd] of each instance's controller in the
//                               per-tile order of the plants; a block that is the same for every instance is one tile, read at tile stride 0
//   lmpc_loop_advance_observed  the per-instance kernel's shape for every plant: an instance's [x | xhat | cmd | d | e] side by side in LDS; first
//                               the lanes of an instance take its output rows (y and yhat share a coefficient load, e to LDS, y to its log), then,
//                               a barrier later, its state rows: the plant's sum and the estimator's, both straight out
//
// Offset-free tracking (mpcx_lmpc_loop_create_offset_free): an observed loop whose estimator carries [xhat; dhat].  The solve reads dhat_k as its
// per-instance exogenous input, and the descriptor's dmeas becomes the true disturbance d_k, which the controller never sees:
//   y = C x + Dd d_k + v_k,  e = y - (C xhat + Dd dhat),  x <- A_p x + B_p cmd + Bd_p d_k + w_k,  xhat <- A xhat + B cmd + Bd dhat + Lx e,  dhat <- dhat + Ld e
//   the same two kernels, instantiated a second time: an instance's LDS row is [x | xhat | cmd | dhat | e | d], Ld a fourth packed block, and the
//   lanes that took the state rows also take the ndu rows of dhat
//
// Steady-state targets (mpcx_lmpc_loop_create_offset_free_target): an offset-free loop whose solve reads us_k = T [r_k; dhat_k; ubar_k] as its
// per-instance input reference, r_k and ubar_k step 0 of the tick's yref and uref.  us_0 is the begin kernel's (from dhat0, the caller's map as it
// lies); us_{k+1} the advance kernel's of tick k, a third instantiation: the instance's LDS row also holds [r_{k+1} | dhat_{k+1} | ubar_{k+1}] --
// dhat_{k+1} in a slot of its own, the dhat_k slot is still being read by the estimator rows of other lanes -- and, one barrier behind the rows of
// dhat, the instance's lanes take the nu rows of us over T, a fifth packed block.  The row's sum is target_us_row (target_device.hpp), the one
// mpcx_target_apply_batch uses.
#include <hip/hip_runtime.h>

#include "lmpc_device.hpp"
#include "target_device.hpp"

namespace mpcx {

namespace {

constexpr int kTile = 64;                         // instances per block = lanes of its one wavefront

#define LOOP_GAS __attribute__((address_space(1)))
#define LOOP_CAS __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ const T LOOP_GAS *gin(const T *p) { return (const T LOOP_GAS *)p; }
template <typename T> __device__ __forceinline__ T LOOP_GAS *gout(T *p) { return (T LOOP_GAS *)p; }

// the window of ph rows starting at row `row0` of every preview array, for the tile's instances: per instance one contiguous run of
// ph * n doubles in the source ([B x (ticks + ph) x n]) and in the staging buffer the solve reads as a per-step reference ([B x ph x n])
__device__ __forceinline__ void gather_windows(const LmpcLoopDev &L, const int b0, const int nvalid, const int row0, const int tid)
{
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!L.pv_src[a]) continue;
        const int n = L.pv_n[a], run = L.ph * n;
        const size_t src_bs = (size_t)(L.ticks + L.ph) * n;
        const double LOOP_GAS *src = gin(L.pv_src[a]) + (size_t)row0 * n;
        double LOOP_GAS *dst = gout(L.pv_dst[a]);
        for (int idx = tid; idx < nvalid * run; idx += kTile) {
            const int r = idx / run, c = idx - r * run;
            dst[(size_t)b0 * run + idx] = src[(size_t)(b0 + r) * src_bs + c];
        }
    }
}

// step 0 of tick k's yref (which = 0: r_k) or uref (1: ubar_k) of instance b; a null source is a bank's "shared" mode: each controller's own
__device__ __forceinline__ const double *target_ref(const LmpcLoopDev &L, const int which, const int b, const int k)
{
    const double *src = which ? L.ub_src : L.r_src;
    if (!src) {
        const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : b];
        return which ? M.uref_s : M.yref_s;
    }
    return src + (size_t)b * (which ? L.ub_bs : L.r_bs) + (size_t)k * (which ? L.ub_tick : L.r_tick);
}
struct ZeroOperand { __device__ double operator[](int) const { return 0.0; } };      // dhat0 = NULL

__global__ __launch_bounds__(kTile) void lmpc_loop_begin_kernel(const LmpcLoopDev L)
{
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kTile;
    const int nvalid = min(kTile, L.batch - b0);
    const size_t xo = (size_t)b0 * L.nx, uo = (size_t)b0 * L.nu;
    double *const xtrue = L.ek ? L.xt : L.x;      // an observed loop keeps the true state apart: x is the estimate, xhat0 or x0
    for (int idx = tid; idx < nvalid * L.nx; idx += kTile) {
        const double v = gin(L.x0)[xo + idx];
        gout(xtrue)[xo + idx] = v;
        gout(L.traj_x)[xo + idx] = v;
    }
    if (L.ek) {
        const double *const h0 = L.xhat0 ? L.xhat0 : L.x0;
        for (int idx = tid; idx < nvalid * L.nx; idx += kTile) {
            const double v = gin(h0)[xo + idx];
            gout(L.x)[xo + idx] = v;
            if (L.traj_xhat) gout(L.traj_xhat)[xo + idx] = v;
        }
    }
    for (int idx = tid; idx < nvalid * L.nu; idx += kTile) gout(L.u)[uo + idx] = gin(L.u0)[uo + idx];
    if (L.dobs) {
        const size_t eo = (size_t)b0 * L.ndu;
        for (int idx = tid; idx < nvalid * L.ndu; idx += kTile) {
            const double v = L.dhat0 ? gin(L.dhat0)[eo + idx] : 0.0;
            gout(L.dhat)[eo + idx] = v;
            if (L.traj_dhat) gout(L.traj_dhat)[eo + idx] = v;
        }
    }
    if (L.tgt) {                                  // us_0 = T [r_0; dhat0; ubar_0], a thread per (instance, row), T as the caller has it: column-major [nu x nrhs]
        const int nu = L.nu, ndu = L.ndu, ny = L.ny;
        for (int idx = tid; idx < nvalid * nu; idx += kTile) {
            const int b = b0 + idx / nu, i = idx % nu;
            const double *T = (L.tmap_batch ? L.tmap_batch + (size_t)b * nu * (ny + ndu + nu) : L.tmap) + i;
            const double *d = L.dhat0 ? L.dhat0 + (size_t)b * ndu : nullptr;
            double v;
            if (d) v = target_us_row(T, (size_t)nu, target_ref(L, 0, b, 0), ny, d, ndu, target_ref(L, 1, b, 0), nu);
            else v = target_us_row(T, (size_t)nu, target_ref(L, 0, b, 0), ny, ZeroOperand{}, ndu, target_ref(L, 1, b, 0), nu);
            gout(L.us)[uo + idx] = v;
            if (L.traj_us) gout(L.traj_us)[uo + idx] = v;
        }
    }
    gather_windows(L, b0, nvalid, 0, tid);
    if (blockIdx.x == 0 && tid == 0) { gout(L.state)[0] = 0; gout(L.state)[1] = 0; }
}

// What every advance kernel ends a tick with: the tick's row of the per-instance logs, the active sets handed to the next solve, the preview windows
// of tick k + 1, and the ticket that moves the counter.
__device__ __forceinline__ void finish_tick(const LmpcLoopDev &L, const int b0, const int nvalid, const int k, const int tid)
{
    const int B = L.batch;
    // the tick's row of the per-instance logs
    if (tid < nvalid) {
        const int b = b0 + tid;
        const size_t at = (size_t)k * B + b;
        if (L.traj_cost) gout(L.traj_cost)[at] = gin(L.cost)[b];
        if (L.traj_status) gout(L.traj_status)[at] = gin(L.status)[b];
        if (L.traj_solver_status) gout(L.traj_solver_status)[at] = gin(L.solver_status)[b];
        if (L.traj_iterations) gout(L.traj_iterations)[at] = gin(L.iterations)[b];
        if (L.traj_polish_rounds) gout(L.traj_polish_rounds)[at] = gin(L.polish_rounds)[b];
        if (L.traj_active_count) gout(L.traj_active_count)[at] = gin(L.active_count)[b];
    }
    // this tick's active sets become the next solve's first working sets
    if (L.warm_lower) {
        const size_t ao = (size_t)b0 * L.aw;
        for (int idx = tid; idx < nvalid * L.aw; idx += kTile) {
            gout(L.warm_lower)[ao + idx] = gin(L.active_lower)[ao + idx];
            gout(L.warm_upper)[ao + idx] = gin(L.active_upper)[ao + idx];
        }
    }
    if (k + 1 < L.ticks) gather_windows(L, b0, nvalid, k + 1, tid);

    // the counter moves when the last block is through: a block that starts late still reads tick k
    __threadfence();
    if (tid == 0) {
        const int done = atomicAdd(L.state + 1, 1);
        if (done == (int)gridDim.x - 1) {
            __hip_atomic_store(L.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(L.state, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// kPlants: a plant per instance.  The tile is then the ipw = 64 / nx instances whose rows fill the wavefront's lanes (from nx = 33 on one instance,
// a lane taking rows lane, lane + 64, ...; lanes past ipw * nx idle), and the packed coefficients are read as: tile t, term j (the nx columns of
// A_b, then the nu of B_b, then the ndu of Bd_b), instance q of the tile, row i at ((t * nterms + j) * ipw + q) * nx + i -- a term is one run of
// ipw * nx doubles of which lane (q, i) reads element q * nx + i, and the terms of a row are one loop.  Sum order per row in both forms: acc = 0,
// fma over A by ascending column, then B, then Bd, the noise added at the store.
template <bool kPlants>
__device__ __forceinline__ void advance_tick(const LmpcLoopDev &L, double *lds)
{
    const int tid = threadIdx.x;
    const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(L.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k >= L.ticks) return;                     // a replay past the run's end: nothing is written
    const int nx = L.nx, nu = L.nu, ndu = L.ndu, B = L.batch;
    // LDS rows: the uniform form keeps a tile of x, of cmd and of d apart; the per-instance form keeps an instance's [x | cmd | d] side by side, the
    // operands of its terms in the terms' order
    const int sx = kPlants ? L.sv : L.sx, su = kPlants ? L.sv : L.su, sd = kPlants ? L.sv : L.sd;
    const int nt = kPlants ? L.ipw : kTile;       // instances of the block's tile
    const int b0 = blockIdx.x * nt;
    const int nvalid = min(nt, B - b0);
    double *xin = lds, *cin = kPlants ? xin + nx : xin + nt * sx, *din = kPlants ? cin + nu : cin + nt * su, *xout = din + nt * sd;
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;

    // in: the tile's states, commands and exogenous-input samples, one contiguous run each
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {
        const int r = idx / nx, c = idx - r * nx;
        xin[r * sx + c] = gin(L.x)[xo + idx];
    }
    double LOOP_GAS *tu = gout(L.traj_u) + (size_t)k * B * nu;
    for (int idx = tid; idx < nvalid * nu; idx += kTile) {
        const int r = idx / nu, c = idx - r * nu;
        const double v = gin(L.cmd)[uo + idx];
        cin[r * su + c] = v;
        gout(L.u)[uo + idx] = v;                  // lastU of the next tick: the command as it is
        tu[uo + idx] = v;
    }
    if (ndu > 0) {                                // d_k: column 0 of this tick's exogenous input, wherever its layout keeps it
        const double LOOP_GAS *dk = gin(L.dmeas) + (size_t)k * L.d_tick;
        for (int idx = tid; idx < nvalid * ndu; idx += kTile) {
            const int r = idx / ndu, c = idx - r * ndu;
            din[r * sd + c] = dk[(size_t)(b0 + r) * L.d_bs + c];
        }
    }
    __syncthreads();

    if constexpr (kPlants) {
        // the plant step of the lane's (instance, row): every term one coalesced request of the wavefront, eight of them (then four) in flight
        // together; the sum is element q * nx + i of the tile's run of x (every read of which the barrier above put ahead of these stores)
        const int lpi = min(nx, kTile);           // lanes per instance
        const int q = tid / lpi;
        if (q < nvalid) {
            const int nterms = nx + nu + ndu;
            const size_t width = (size_t)nt * nx;
            const double LOOP_GAS *P = gin(L.pk) + (size_t)blockIdx.x * nterms * width + q * nx;
            const double *v = xin + q * sx;
            double LOOP_GAS *tx = gout(L.traj_x) + (size_t)(k + 1) * B * nx;
            const double LOOP_GAS *w = L.noise ? gin(L.noise) + (size_t)k * B * nx : nullptr;
            for (int i = tid - q * lpi; i < nx; i += lpi) {
                const double LOOP_GAS *Pi = P + i;
                double acc = 0.0;
                int j = 0;
#pragma unroll 1
                for (; j + 8 <= nterms; j += 8) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc = fma(Pi[(j + e) * width], v[j + e], acc);
                }
#pragma unroll 1
                for (; j + 4 <= nterms; j += 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = fma(Pi[(j + e) * width], v[j + e], acc);
                }
#pragma unroll 1
                for (; j < nterms; ++j) acc = fma(Pi[j * width], v[j], acc);
                const size_t at = xo + q * nx + i;
                if (w) acc += w[at];
                gout(L.x)[at] = acc;
                tx[at] = acc;
            }
        }
    } else {
        // the plant step of the lane's instance, row by row of [A_p | B_p | Bd_p] (row-major, the rows of the three side by side per matrix)
        if (tid < nvalid) {
            const double LOOP_CAS *Ap = (const double LOOP_CAS *)L.plant;
            const double LOOP_CAS *Bp = Ap + nx * nx, *Dp = Bp + nx * nu;
            const double *xr = xin + tid * sx, *ur = cin + tid * su, *dr = din + tid * sd;
            for (int i = 0; i < nx; ++i) {
                double acc = 0.0;
#pragma unroll 8
                for (int j = 0; j < nx; ++j) acc = fma(Ap[i * nx + j], xr[j], acc);
#pragma unroll 4
                for (int j = 0; j < nu; ++j) acc = fma(Bp[i * nu + j], ur[j], acc);
#pragma unroll 2
                for (int j = 0; j < ndu; ++j) acc = fma(Dp[i * ndu + j], dr[j], acc);
                xout[tid * sx + i] = acc;
            }
        }
        __syncthreads();

        // out: the new state (plus the process disturbance the controller knows nothing about) to the loop's x and to row k + 1 of traj_x
        {
            double LOOP_GAS *tx = gout(L.traj_x) + (size_t)(k + 1) * B * nx;
            const double LOOP_GAS *w = L.noise ? gin(L.noise) + (size_t)k * B * nx : nullptr;
            for (int idx = tid; idx < nvalid * nx; idx += kTile) {
                const int r = idx / nx, c = idx - r * nx;
                double v = xout[r * sx + c];
                if (w) v += w[xo + idx];
                gout(L.x)[xo + idx] = v;
                tx[xo + idx] = v;
            }
        }
    }
    finish_tick(L, b0, nvalid, k, tid);
}

// n terms behind acc in ascending order: term j is P[j * width] -- one coalesced request of the wavefront -- times v[j] from LDS, the loads of eight
// terms (then four) in flight together
__device__ __forceinline__ double row_terms(const double LOOP_GAS *P, const size_t width, const double *v, const int n, double acc)
{
    int j = 0;
#pragma unroll 1
    for (; j + 8 <= n; j += 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fma(P[(j + e) * width], v[j + e], acc);
    }
#pragma unroll 1
    for (; j + 4 <= n; j += 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fma(P[(j + e) * width], v[j + e], acc);
    }
#pragma unroll 1
    for (; j < n; ++j) acc = fma(P[j * width], v[j], acc);
    return acc;
}

// the same for the two output sums, which share their coefficients: y over the true state's operands, yh over the estimate's
__device__ __forceinline__ void output_terms(const double LOOP_GAS *M, const size_t width, const double *vx, const double *vh, const int n, double &y, double &yh)
{
    int j = 0;
#pragma unroll 1
    for (; j + 4 <= n; j += 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double c = M[(j + e) * width];
            y = fma(c, vx[j + e], y);
            yh = fma(c, vh[j + e], yh);
        }
    }
#pragma unroll 1
    for (; j < n; ++j) {
        const double c = M[j * width];
        y = fma(c, vx[j], y);
        yh = fma(c, vh[j], yh);
    }
}

// The tick of an observed loop.  Tiles, lanes and the packed order are the per-instance kernel's (above); the estimator block has nx + nu + ndu + ny
// terms of nx rows, the measurement block nx + ndu terms of ny rows (lane (q, i) reads element q * ny + i of a term's run of ipw * ny), each block
// at its own tile stride.  Sum order, every row from acc = 0 by ascending column: y over C, then Dd, then + v_k; yhat the same without v_k; x as
// above; xhat over A, B, Bd -- the plant's order -- then L, nothing added at the store.  Hence e = 0 exactly where xhat = x bitwise and v_k is
// absent, and xhat <- x's own bits where the plant is the controller's model and no w_k comes on top.
// kOff, the tick of an offset-free loop: the slot behind cmd holds dhat_k (the operand of yhat's Dd terms and of the estimator's Bd terms, so the
// estimator's row is still one chain over hin ...), the true d_k has a slot of its own behind e (the operand of y's Dd terms and of the plant's Bd_p
// terms), and dhat <- dhat + (Ld e summed from 0 by ascending column).  With Ld = 0 and dhat = d bitwise every sum is the observed tick's.
// kTgt (with kOff), the tick of a loop with steady-state targets: behind d the row holds [r_{k+1} | dhat_{k+1} | ubar_{k+1}], the operands of
// us_{k+1} in T's column order; r and ubar come in with everything else, dhat_{k+1} from the lane that stores it, and a barrier later the lanes of
// the instance take the nu rows of us.  Nothing else of the tick changes: with T = [0 | 0 | I] the solve is given ubar's bits.
template <bool kOff, bool kTgt = false>
__device__ __forceinline__ void advance_observed(const LmpcLoopDev &L, double *lds)
{
    static_assert(kOff || !kTgt, "targets need the disturbance estimate");
    const int tid = threadIdx.x;
    const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(L.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k >= L.ticks) return;                     // a replay past the run's end: nothing is written
    const int nx = L.nx, nu = L.nu, ndu = L.ndu, ny = L.ny, B = L.batch, so = L.so;
    const int nt = L.ipw;
    const int b0 = blockIdx.x * nt;
    const int nvalid = min(nt, B - b0);
    double *xin = lds, *hin = xin + nx, *cin = hin + nx, *din = cin + nu, *ein = din + ndu;   // an instance's row: the estimator's operands are hin ... in its terms' order
    double *tin = din;                            // the disturbance that acts on the plant and on the measurement
    if constexpr (kOff) tin = ein + ny;
    double *rin = tin + ndu, *nin = rin + ny, *bin = nin + ndu;      // (kTgt) r, dhat and ubar of tick k + 1
    const size_t xo = (size_t)b0 * nx, uo = (size_t)b0 * nu;

    // in: the tile's true states, estimates, commands and exogenous-input samples, one contiguous run each
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {
        const int r = idx / nx, c = idx - r * nx;
        xin[r * so + c] = gin(L.xt)[xo + idx];
        hin[r * so + c] = gin(L.x)[xo + idx];
    }
    double LOOP_GAS *tu = gout(L.traj_u) + (size_t)k * B * nu;
    for (int idx = tid; idx < nvalid * nu; idx += kTile) {
        const int r = idx / nu, c = idx - r * nu;
        const double v = gin(L.cmd)[uo + idx];
        cin[r * so + c] = v;
        gout(L.u)[uo + idx] = v;                  // lastU of the next tick: the command as it is
        tu[uo + idx] = v;
    }
    if (ndu > 0) {
        const double LOOP_GAS *dk = gin(L.dmeas) + (size_t)k * L.d_tick;
        for (int idx = tid; idx < nvalid * ndu; idx += kTile) {
            const int r = idx / ndu, c = idx - r * ndu;
            tin[r * so + c] = dk[(size_t)(b0 + r) * L.d_bs + c];
            if constexpr (kOff) din[r * so + c] = gin(L.dhat)[(size_t)b0 * ndu + idx];      // dhat_k: no read of it behind this barrier
        }
    }
    if constexpr (kTgt) {
        for (int idx = tid; idx < nvalid * ny; idx += kTile) {
            const int r = idx / ny, c = idx - r * ny;
            rin[r * so + c] = target_ref(L, 0, b0 + r, k + 1)[c];
        }
        for (int idx = tid; idx < nvalid * nu; idx += kTile) {
            const int r = idx / nu, c = idx - r * nu;
            bin[r * so + c] = target_ref(L, 1, b0 + r, k + 1)[c];
        }
    }
    __syncthreads();

    const int lpi = min(nx, kTile);               // lanes per instance
    const int q = tid / lpi;
    const bool mine = q < nvalid;
    // the measurement and the innovation of the lane's (instance, output row)
    if (mine) {
        const size_t width = (size_t)nt * ny;
        const double LOOP_GAS *M = gin(L.mk) + (size_t)blockIdx.x * L.mk_ts + q * ny;
        const double *xr = xin + q * so, *hr = hin + q * so, *dr = din + q * so, *tr = tin + q * so;
        const size_t yo = ((size_t)k * B + b0 + q) * ny;
        const double LOOP_GAS *vn = L.meas_noise ? gin(L.meas_noise) + yo : nullptr;
        for (int i = tid - q * lpi; i < ny; i += lpi) {
            double y = 0.0, yh = 0.0;
            output_terms(M + i, width, xr, hr, nx, y, yh);
            output_terms(M + i + nx * width, width, tr, dr, ndu, y, yh);
            if (vn) y += vn[i];
            ein[q * so + i] = y - yh;
            if (L.traj_y) gout(L.traj_y)[yo + i] = y;
        }
    }
    __syncthreads();

    // the plant step and the estimator step of the lane's (instance, state row); every read of x and xhat is ahead of the first barrier
    if (mine) {
        const size_t width = (size_t)nt * nx;
        const double LOOP_GAS *P = gin(L.ok) + (size_t)blockIdx.x * L.ok_ts + q * nx;
        const double LOOP_GAS *E = gin(L.ek) + (size_t)blockIdx.x * L.ek_ts + q * nx;
        const double *xr = xin + q * so, *hr = hin + q * so, *cr = cin + q * so;
        double LOOP_GAS *tx = gout(L.traj_x) + (size_t)(k + 1) * B * nx;
        double LOOP_GAS *th = L.traj_xhat ? gout(L.traj_xhat) + (size_t)(k + 1) * B * nx : nullptr;
        const double LOOP_GAS *w = L.noise ? gin(L.noise) + (size_t)k * B * nx : nullptr;
        for (int i = tid - q * lpi; i < nx; i += lpi) {
            double acc = row_terms(P + i, width, xr, nx, 0.0);
            if constexpr (kOff) {
                acc = row_terms(P + i + nx * width, width, cr, nu, acc);
                acc = row_terms(P + i + (nx + nu) * width, width, tin + q * so, ndu, acc);
            } else acc = row_terms(P + i + nx * width, width, cr, nu + ndu, acc);
            const double est = row_terms(E + i, width, hr, nx + nu + ndu + ny, 0.0);
            const size_t at = xo + q * nx + i;
            if (w) acc += w[at];
            gout(L.xt)[at] = acc;
            tx[at] = acc;
            gout(L.x)[at] = est;
            if (th) th[at] = est;
        }
        if constexpr (kOff) {                     // the rows of dhat, by the same lanes: ny terms of Ld, lane (q, i) reading element q * ndu + i of a term
            const size_t wd = (size_t)nt * ndu;
            const double LOOP_GAS *G = gin(L.dk) + (size_t)blockIdx.x * L.dk_ts + q * ndu;
            const double *er = ein + q * so, *dr = din + q * so;
            double LOOP_GAS *td = L.traj_dhat ? gout(L.traj_dhat) + (size_t)(k + 1) * B * ndu : nullptr;
            for (int i = tid - q * lpi; i < ndu; i += lpi) {
                const double v = dr[i] + row_terms(G + i, wd, er, ny, 0.0);
                const size_t at = (size_t)(b0 + q) * ndu + i;
                gout(L.dhat)[at] = v;
                if (td) td[at] = v;
                if constexpr (kTgt) nin[q * so + i] = v;
            }
        }
    }
    if constexpr (kTgt) {
        __syncthreads();
        if (mine) {                               // the rows of us_{k+1}: nrhs terms of T, lane (q, i) reading element q * nu + i of a term
            const size_t wt = (size_t)nt * nu;
            const double LOOP_GAS *T = gin(L.tk) + (size_t)blockIdx.x * L.tk_ts + q * nu;
            double LOOP_GAS *ts = L.traj_us ? gout(L.traj_us) + (size_t)(k + 1) * B * nu : nullptr;
            for (int i = tid - q * lpi; i < nu; i += lpi) {
                const double v = target_us_row(T + i, wt, rin + q * so, ny, nin + q * so, ndu, bin + q * so, nu);
                const size_t at = (size_t)(b0 + q) * nu + i;
                gout(L.us)[at] = v;
                if (ts) ts[at] = v;
            }
        }
    }
    finish_tick(L, b0, nvalid, k, tid);
}

__global__ __launch_bounds__(kTile) void lmpc_loop_advance_kernel(const LmpcLoopDev L)
{
    extern __shared__ double lds[];
    advance_tick<false>(L, lds);
}

// (a block is one wavefront and a compute unit sees a few of them: registers are better spent on a group of terms in flight than on occupancy)
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(1, 4))) void lmpc_loop_advance_plants_kernel(const LmpcLoopDev L)
{
    extern __shared__ double lds[];
    advance_tick<true>(L, lds);
}

__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(1, 4))) void lmpc_loop_advance_observed_kernel(const LmpcLoopDev L)
{
    extern __shared__ double lds[];
    advance_observed<false>(L, lds);
}

__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(1, 4))) void lmpc_loop_advance_offset_free_kernel(const LmpcLoopDev L)
{
    extern __shared__ double lds[];
    advance_observed<true>(L, lds);
}

__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(1, 4))) void lmpc_loop_advance_offset_free_target_kernel(const LmpcLoopDev L)
{
    extern __shared__ double lds[];
    advance_observed<true, true>(L, lds);
}

constexpr int kPackThreads = 256;

// Head of a run: the plants in the advance kernel's order, from the caller's array ([B x nx (nx + nu + ndu)], A_b | B_b | Bd_b column-major: term j
// of instance b is the run of nx doubles at (b nterms + j) nx) or from the model struct of each instance's controller; the padding of the last
// tile is zero.  And each controller's own exogenous input, step 0, as the [B x ndu] array the advance kernel addresses per instance.
__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_plants_kernel(const LmpcLoopDev L)
{
    const int nx = L.nx, nu = L.nu, ndu = L.ndu, B = L.batch, ipw = L.ipw;
    const size_t first = (size_t)blockIdx.x * kPackThreads + threadIdx.x, step = (size_t)gridDim.x * kPackThreads;
    if (L.pk) {
        const size_t nterms = (size_t)(nx + nu + ndu), width = (size_t)ipw * nx, per_tile = nterms * width;
        const size_t total = (size_t)((B + ipw - 1) / ipw) * per_tile;
        for (size_t idx = first; idx < total; idx += step) {
            const size_t t = idx / per_tile, rem = idx - t * per_tile;
            const int j = (int)(rem / width), qi = (int)(rem - j * width);
            const int q = qi / nx, i = qi - q * nx;
            const size_t b = t * ipw + q;
            double v = 0.0;
            if (b < (size_t)B) {
                if (L.pk_src) v = gin(L.pk_src)[(b * nterms + j) * nx + i];
                else {
                    const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
                    v = j < nx ? M.A[j * nx + i] : j < nx + nu ? M.B[(j - nx) * nx + i] : M.Bd[(j - nx - nu) * nx + i];
                }
            }
            gout(L.pk)[idx] = v;
        }
    }
    if (L.d_own) {
        for (size_t idx = first; idx < (size_t)B * ndu; idx += step) {
            const size_t b = idx / ndu;
            const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
            gout(L.d_own)[idx] = M.dmeas_s[idx - b * ndu];
        }
    }
}

// Head of a run of an observed loop: its blocks in the advance kernel's order.  The plant where it is one for the batch (from the row-major
// `plant`: one tile, every instance of it the same), the estimator [A | B | Bd | L] and the measurement [C | Dd] from the handle's model or from
// the model struct of each instance's controller, the gain from the one for the batch or from the caller's per-instance array.  A block with tile
// stride 0 is one tile.  kOff, an offset-free loop: the gain is [(nx + ndu) x ny], its first nx rows the estimator block's, the others the fourth block.
template <bool kOff>
__device__ __forceinline__ void pack_observer(const LmpcLoopDev &L)
{
    const int nx = L.nx, nu = L.nu, ndu = L.ndu, ny = L.ny, B = L.batch, ipw = L.ipw;
    const size_t first = (size_t)blockIdx.x * kPackThreads + threadIdx.x, step = (size_t)gridDim.x * kPackThreads;
    const size_t tiles = (size_t)((B + ipw - 1) / ipw);
    const int npl = nx + nu + ndu;
    const int ldg = kOff ? nx + ndu : nx;         // rows of a gain
    if (L.ok != L.pk) {
        const size_t width = (size_t)ipw * nx, total = (size_t)npl * width;
        const double *Ap = L.plant, *Bp = Ap + nx * nx, *Dp = Bp + nx * nu;
        for (size_t idx = first; idx < total; idx += step) {
            const int j = (int)(idx / width), i = (int)((idx - j * width) % nx);
            gout(L.ok)[idx] = j < nx ? Ap[i * nx + j] : j < nx + nu ? Bp[i * nu + (j - nx)] : Dp[i * ndu + (j - nx - nu)];
        }
    }
    {
        const size_t width = (size_t)ipw * nx, per_tile = (size_t)(npl + ny) * width;
        const size_t total = (L.ek_ts ? tiles : 1) * per_tile;
        for (size_t idx = first; idx < total; idx += step) {
            const size_t t = idx / per_tile, rem = idx - t * per_tile;
            const int j = (int)(rem / width), qi = (int)(rem - j * width);
            const int q = qi / nx, i = qi - q * nx;
            const size_t b = L.ek_ts ? t * ipw + q : 0;
            double v = 0.0;
            if (b < (size_t)B) {
                if (j >= npl) v = L.gain_batch ? gin(L.gain_batch)[(b * ny + (j - npl)) * ldg + i] : L.gain[(j - npl) * ldg + i];
                else if (L.mA) v = j < nx ? L.mA[j * nx + i] : j < nx + nu ? L.mB[(j - nx) * nx + i] : L.mBd[(j - nx - nu) * nx + i];
                else {
                    const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
                    v = j < nx ? M.A[j * nx + i] : j < nx + nu ? M.B[(j - nx) * nx + i] : M.Bd[(j - nx - nu) * nx + i];
                }
            }
            gout(L.ek)[idx] = v;
        }
    }
    {
        const size_t width = (size_t)ipw * ny, per_tile = (size_t)(nx + ndu) * width;
        const size_t total = (L.mk_ts ? tiles : 1) * per_tile;
        for (size_t idx = first; idx < total; idx += step) {
            const size_t t = idx / per_tile, rem = idx - t * per_tile;
            const int j = (int)(rem / width), qi = (int)(rem - j * width);
            const int q = qi / ny, i = qi - q * ny;
            const size_t b = L.mk_ts ? t * ipw + q : 0;
            double v = 0.0;
            if (b < (size_t)B) {
                if (L.mC) v = j < nx ? L.mC[j * ny + i] : L.mDd[(j - nx) * ny + i];
                else {
                    const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
                    v = j < nx ? M.C[j * ny + i] : M.Dd[(j - nx) * ny + i];
                }
            }
            gout(L.mk)[idx] = v;
        }
    }
    if constexpr (kOff) {
        const size_t width = (size_t)ipw * ndu, per_tile = (size_t)ny * width;
        const size_t total = (L.dk_ts ? tiles : 1) * per_tile;
        for (size_t idx = first; idx < total; idx += step) {
            const size_t t = idx / per_tile, rem = idx - t * per_tile;
            const int j = (int)(rem / width), qi = (int)(rem - j * width);
            const int q = qi / ndu, i = qi - q * ndu;
            const size_t b = L.dk_ts ? t * ipw + q : 0;
            double v = 0.0;
            if (b < (size_t)B) v = L.gain_batch ? gin(L.gain_batch)[(b * ny + j) * ldg + nx + i] : L.gain[j * ldg + nx + i];
            gout(L.dk)[idx] = v;
        }
    }
}

__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_observer_kernel(const LmpcLoopDev L) { pack_observer<false>(L); }
__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_offset_free_kernel(const LmpcLoopDev L) { pack_observer<true>(L); }

// ... and of a loop with targets, behind the two above: T in the advance kernel's order, from the one map for the batch (one tile) or the caller's
// per-instance array, both column-major [nu x nrhs]
__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_target_kernel(const LmpcLoopDev L)
{
    const int nu = L.nu, B = L.batch, ipw = L.ipw, nrhs = L.ny + L.ndu + L.nu;
    const size_t first = (size_t)blockIdx.x * kPackThreads + threadIdx.x, step = (size_t)gridDim.x * kPackThreads;
    const size_t tiles = (size_t)((B + ipw - 1) / ipw);
    const size_t width = (size_t)ipw * nu, per_tile = (size_t)nrhs * width;
    const size_t total = (L.tk_ts ? tiles : 1) * per_tile;
    for (size_t idx = first; idx < total; idx += step) {
        const size_t t = idx / per_tile, rem = idx - t * per_tile;
        const int j = (int)(rem / width), qi = (int)(rem - j * width);
        const int q = qi / nu, i = qi - q * nu;
        const size_t b = L.tk_ts ? t * ipw + q : 0;
        double v = 0.0;
        if (b < (size_t)B) v = L.tmap_batch ? gin(L.tmap_batch)[(b * nrhs + j) * nu + i] : L.tmap[j * nu + i];
        gout(L.tk)[idx] = v;
    }
}

inline int odd(int n) { return n | 1; }

}  // namespace

void lmpc_loop_plan_lds(LmpcLoopDev &L)
{
    L.sx = odd(L.nx); L.su = odd(L.nu); L.sd = L.ndu > 0 ? odd(L.ndu) : 0;
    L.ipw = L.nx < kTile ? kTile / L.nx : 1; L.sv = odd(L.nx + L.nu + L.ndu);
    L.so = odd(2 * L.nx + L.nu + L.ndu + L.ny + (L.dobs ? L.ndu : 0) + (L.tgt ? L.ny + L.ndu + L.nu : 0));
}

size_t lmpc_loop_packed_len(const LmpcLoopDev &L) { return (size_t)((L.batch + L.ipw - 1) / L.ipw) * (L.nx + L.nu + L.ndu) * L.ipw * L.nx; }

size_t lmpc_loop_block_len(const LmpcLoopDev &L, int which, size_t tiles)
{
    const size_t terms = which == 0 ? L.nx + L.nu + L.ndu : which == 1 ? L.nx + L.nu + L.ndu + L.ny : which == 2 ? L.nx + L.ndu : which == 3 ? L.ny : L.ny + L.ndu + L.nu;
    return tiles * terms * L.ipw * (which == 2 ? L.ny : which == 3 ? L.ndu : which == 4 ? L.nu : L.nx);
}

static size_t observed_lds_bytes(const LmpcLoopDev &L) { return (size_t)L.ipw * L.so * sizeof(double); }

size_t lmpc_loop_lds_bytes(const LmpcLoopDev &L) { return (size_t)kTile * (2 * L.sx + L.su + L.sd) * sizeof(double); }

int lmpc_loop_prepare(const LmpcLoopDev &L)
{
    if (L.ek) {                                   // the observed kernel's tile: a few KB unless one instance has thousands of states
        const size_t bytes = observed_lds_bytes(L);
        if (bytes > lmpc_lds_limit()) return -2;
        const void *kernel = L.tgt    ? reinterpret_cast<const void *>(lmpc_loop_advance_offset_free_target_kernel)
                             : L.dobs ? reinterpret_cast<const void *>(lmpc_loop_advance_offset_free_kernel)
                                      : reinterpret_cast<const void *>(lmpc_loop_advance_observed_kernel);
        if (bytes > 48 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return -3;
        return 0;
    }
    if (L.pk) return 0;                           // the per-instance kernel's tile: [x | cmd | d] of at most 64 instances of 1 state ... one of many
    const size_t bytes = lmpc_loop_lds_bytes(L);
    if (bytes > lmpc_lds_limit()) return -2;
    if (bytes > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(lmpc_loop_advance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return -3;
    return 0;
}

int lmpc_loop_begin(const LmpcLoopDev &L, void *stream)
{
    const int blocks = (L.batch + kTile - 1) / kTile;
    hipLaunchKernelGGL(lmpc_loop_begin_kernel, dim3(blocks), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_pack_plants(const LmpcLoopDev &L, void *stream)
{
    if (!L.pk && !L.d_own) return 0;
    const size_t n = L.pk ? lmpc_loop_packed_len(L) : (size_t)L.batch * L.ndu;
    size_t blocks = (n + kPackThreads - 1) / kPackThreads;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(lmpc_loop_pack_plants_kernel, dim3((unsigned)blocks), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_pack_observer(const LmpcLoopDev &L, void *stream)
{
    if (!L.ek) return 0;
    const size_t tiles = (size_t)((L.batch + L.ipw - 1) / L.ipw);
    size_t n = lmpc_loop_block_len(L, 1, L.ek_ts ? tiles : 1);
    if (lmpc_loop_block_len(L, 2, L.mk_ts ? tiles : 1) > n) n = lmpc_loop_block_len(L, 2, L.mk_ts ? tiles : 1);
    if (L.dobs && lmpc_loop_block_len(L, 3, L.dk_ts ? tiles : 1) > n) n = lmpc_loop_block_len(L, 3, L.dk_ts ? tiles : 1);
    size_t blocks = (n + kPackThreads - 1) / kPackThreads;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    if (L.dobs) hipLaunchKernelGGL(lmpc_loop_pack_offset_free_kernel, dim3((unsigned)blocks), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    else hipLaunchKernelGGL(lmpc_loop_pack_observer_kernel, dim3((unsigned)blocks), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    if (L.tgt) {
        blocks = (lmpc_loop_block_len(L, 4, L.tk_ts ? tiles : 1) + kPackThreads - 1) / kPackThreads;
        if (blocks > 2048) blocks = 2048;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(lmpc_loop_pack_target_kernel, dim3((unsigned)blocks), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_advance(const LmpcLoopDev &L, void *stream)
{
    if (L.ek) {
        const int tiles = (L.batch + L.ipw - 1) / L.ipw;
        if (L.tgt) hipLaunchKernelGGL(lmpc_loop_advance_offset_free_target_kernel, dim3(tiles), dim3(kTile), observed_lds_bytes(L), reinterpret_cast<hipStream_t>(stream), L);
        else if (L.dobs) hipLaunchKernelGGL(lmpc_loop_advance_offset_free_kernel, dim3(tiles), dim3(kTile), observed_lds_bytes(L), reinterpret_cast<hipStream_t>(stream), L);
        else hipLaunchKernelGGL(lmpc_loop_advance_observed_kernel, dim3(tiles), dim3(kTile), observed_lds_bytes(L), reinterpret_cast<hipStream_t>(stream), L);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    if (L.pk) {
        const int tiles = (L.batch + L.ipw - 1) / L.ipw;
        const size_t lds = (size_t)L.ipw * L.sv * sizeof(double);
        hipLaunchKernelGGL(lmpc_loop_advance_plants_kernel, dim3(tiles), dim3(kTile), lds, reinterpret_cast<hipStream_t>(stream), L);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    const int blocks = (L.batch + kTile - 1) / kTile;
    hipLaunchKernelGGL(lmpc_loop_advance_kernel, dim3(blocks), dim3(kTile), lmpc_loop_lds_bytes(L), reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mpcx
