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
//   lmpc_loop_advance_plants  the same tick with lane <-> (instance, state row): a wavefront holds ipw = 64 / nx instances, its lanes accumulate their
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
//
// Lanes and rows.  mpcx_lmpc_create refuses nx, nu, ndu or ny above 64 ("one lane per component"), so where a lane is an (instance, row) an instance
// has lpi = nx lanes and a wavefront ipw = 64 / nx instances: 1 for nx = 33 .. 64 (64 - nx idle lanes), 2 for nx = 32 (none idle), more below.  Every
// state row has its lane.  The other rows of an instance (ny, ndu, nu of them) are taken by the same nx lanes and can outnumber them (nx = 2, ny = 3):
// those loops stride by lpi.
//
// The packed blocks (LoopBlock, lmpc_loop_block_shape in lmpc_device.hpp): a block is `terms` columns of `rows` coefficients per instance, laid out
// tile t, term j, instance q of the tile, row i at ((t * terms + j) * ipw + q) * rows + i -- a term of a tile is one run of ipw * rows doubles of which
// lane (q, i) reads element q * rows + i.  A tile stride of 0 is one tile, the same for every instance; the padding of the last tile is zero.
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

// What every tick begins with, in two parts with the kernel's own staging of its states between them (the order of the global loads -- states,
// commands, d_k -- is the one the kernels' register allocation was measured with).  begin_tick: the tick number and the block's tile of nt
// instances; false past the run's end, where a replay writes nothing.
struct Tick { int k, b0, nvalid; };
__device__ __forceinline__ bool begin_tick(const LmpcLoopDev &L, const int nt, Tick &T)
{
    T.k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(L.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    T.b0 = blockIdx.x * nt;
    T.nvalid = min(nt, L.batch - T.b0);
    return T.k < L.ticks;
}
// stage_inputs: the tile's commands, one contiguous run, into LDS at row stride su, to u (lastU of the next tick: the command as it is) and to the
// tick's row of traj_u.  And d_k, column 0 of this tick's exogenous input wherever its layout keeps it, into LDS at row stride sd; an offset-free
// loop's dhat_k ([B x ndu]) rides in that loop, into hin at the same stride (null: there is none).
__device__ __forceinline__ void stage_inputs(const LmpcLoopDev &L, const Tick T, double *cin, const int su, double *din, const int sd, const double *dhat, double *hin)
{
    const int tid = threadIdx.x;
    const int nu = L.nu, ndu = L.ndu, B = L.batch;
    const size_t uo = (size_t)T.b0 * nu;
    double LOOP_GAS *tu = gout(L.traj_u) + (size_t)T.k * B * nu;
    for (int idx = tid; idx < T.nvalid * nu; idx += kTile) {
        const int r = idx / nu, c = idx - r * nu;
        const double v = gin(L.cmd)[uo + idx];
        cin[r * su + c] = v;
        gout(L.u)[uo + idx] = v;
        tu[uo + idx] = v;
    }
    if (ndu > 0) {
        const double LOOP_GAS *dk = gin(L.dmeas) + (size_t)T.k * L.d_tick;
        for (int idx = tid; idx < T.nvalid * ndu; idx += kTile) {
            const int r = idx / ndu, c = idx - r * ndu;
            din[r * sd + c] = dk[(size_t)(T.b0 + r) * L.d_bs + c];
            if (dhat) hin[r * sd + c] = gin(dhat)[(size_t)T.b0 * ndu + idx];
        }
    }
}

// kPlants: a plant per instance, lane <-> (instance, state row) of a tile of ipw instances (the file's head), the plant block's terms -- the nx
// columns of A_b, then the nu of B_b, then the ndu of Bd_b -- one loop per row.  Sum order per row in both forms: acc = 0, fma over A by ascending
// column, then B, then Bd, the noise added at the store.
template <bool kPlants>
__device__ __forceinline__ void advance_tick(const LmpcLoopDev &L, double *lds)
{
    const int tid = threadIdx.x;
    const int nx = L.nx, nu = L.nu, B = L.batch;
    // LDS rows: the uniform form keeps a tile of x, of cmd and of d apart; the per-instance form keeps an instance's [x | cmd | d] side by side, the
    // operands of its terms in the terms' order
    const int sx = kPlants ? L.sv : L.sx, su = kPlants ? L.sv : L.su, sd = kPlants ? L.sv : L.sd;
    const int nt = kPlants ? L.ipw : kTile;       // instances of the block's tile
    double *xin = lds, *cin = kPlants ? xin + nx : xin + nt * sx, *din = kPlants ? cin + nu : cin + nt * su, *xout = din + nt * sd;
    Tick T;
    if (!begin_tick(L, nt, T)) return;
    const int k = T.k, b0 = T.b0, nvalid = T.nvalid;
    const size_t xo = (size_t)b0 * nx;
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {      // the tile's states, one contiguous run
        const int r = idx / nx, c = idx - r * nx;
        xin[r * sx + c] = gin(L.x)[xo + idx];
    }
    stage_inputs(L, T, cin, su, din, sd, nullptr, nullptr);
    __syncthreads();

    if constexpr (kPlants) {
        // the plant step of the lane's (instance, row): every term one coalesced request of the wavefront; the sum is element q * nx + i of the
        // tile's run of x (every read of which the barrier above put ahead of these stores)
        const int lpi = min(nx, kTile);           // lanes per instance: nx (the file's head)
        const int q = tid / lpi;
        if (q < nvalid) {
            const LoopBlockShape s = lmpc_loop_block_shape(L, kPlantBlock);
            const size_t width = (size_t)nt * s.rows;
            const double LOOP_GAS *P = gin(L.pk) + (size_t)blockIdx.x * s.terms * width + q * nx;      // (a tile per block: the stride is a tile's length)
            const double *v = xin + q * sx;
            double LOOP_GAS *tx = gout(L.traj_x) + (size_t)(k + 1) * B * nx;
            const double LOOP_GAS *w = L.noise ? gin(L.noise) + (size_t)k * B * nx : nullptr;
            for (int i = tid - q * lpi; i < nx; i += lpi) {
                double acc = row_terms(P + i, width, v, s.terms, 0.0);
                const size_t at = xo + q * nx + i;
                if (w) acc += w[at];
                gout(L.x)[at] = acc;
                tx[at] = acc;
            }
        }
    } else {
        // the plant step of the lane's instance, row by row of [A_p | B_p | Bd_p] (row-major, the rows of the three side by side per matrix)
        const int ndu = L.ndu;
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

// The tick of an observed loop.  Tiles and lanes are the per-instance kernel's; each block at its own tile stride.  Sum order, every row from
// acc = 0 by ascending column: y over C, then Dd, then + v_k; yhat the same without v_k; x as above; xhat over A, B, Bd -- the plant's order -- then
// L, nothing added at the store.  Hence e = 0 exactly where xhat = x bitwise and v_k is absent, and xhat <- x's own bits where the plant is the
// controller's model and no w_k comes on top.
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
    const int nx = L.nx, nu = L.nu, ndu = L.ndu, ny = L.ny, B = L.batch, so = L.so;
    const int nt = L.ipw;
    double *xin = lds, *hin = xin + nx, *cin = hin + nx, *din = cin + nu, *ein = din + ndu;   // an instance's row: the estimator's operands are hin ... in its terms' order
    double *tin = din;                            // the disturbance that acts on the plant and on the measurement
    if constexpr (kOff) tin = ein + ny;
    double *rin = tin + ndu, *nin = rin + ny, *bin = nin + ndu;      // (kTgt) r, dhat and ubar of tick k + 1
    Tick T;
    if (!begin_tick(L, nt, T)) return;
    const int k = T.k, b0 = T.b0, nvalid = T.nvalid;
    const size_t xo = (size_t)b0 * nx;
    for (int idx = tid; idx < nvalid * nx; idx += kTile) {      // the tile's true states and estimates, one contiguous run each
        const int r = idx / nx, c = idx - r * nx;
        xin[r * so + c] = gin(L.xt)[xo + idx];
        hin[r * so + c] = gin(L.x)[xo + idx];
    }
    stage_inputs(L, T, cin, so, tin, so, kOff ? L.dhat : nullptr, din);      // (dhat_k: no read of it behind this barrier)
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

    const int lpi = min(nx, kTile);               // lanes per instance: nx (the file's head)
    const int q = tid / lpi;
    const bool mine = q < nvalid;
    // the measurement and the innovation of the lane's (instance, output row): the measurement block's nx terms of C, then its ndu of Dd
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
            const double est = row_terms(E + i, width, hr, lmpc_loop_block_shape(L, kEstimatorBlock).terms, 0.0);
            const size_t at = xo + q * nx + i;
            if (w) acc += w[at];
            gout(L.xt)[at] = acc;
            tx[at] = acc;
            gout(L.x)[at] = est;
            if (th) th[at] = est;
        }
        if constexpr (kOff) {                     // the rows of dhat, by the same lanes: the ny terms of Ld
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
        if (mine) {                               // the rows of us_{k+1}: the ny + ndu + nu terms of T
            const size_t wt = (size_t)nt * nu;
            const double LOOP_GAS *Tm = gin(L.tk) + (size_t)blockIdx.x * L.tk_ts + q * nu;
            double LOOP_GAS *ts = L.traj_us ? gout(L.traj_us) + (size_t)(k + 1) * B * nu : nullptr;
            for (int i = tid - q * lpi; i < nu; i += lpi) {
                const double v = target_us_row(Tm + i, wt, rin + q * so, ny, nin + q * so, ndu, bin + q * so, nu);
                const size_t at = (size_t)(b0 + q) * nu + i;
                gout(L.us)[at] = v;
                if (ts) ts[at] = v;
            }
        }
    }
    finish_tick(L, b0, nvalid, k, tid);
}

using LoopKernel = void (*)(const LmpcLoopDev);

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

// Head of a run: one packed block in the advance kernels' order (the file's head), a grid-stride loop over its elements.  value(b, j, i) is the
// coefficient of term j, row i of instance b; a block of one tile is filled from instance 0.
template <typename Value>
__device__ __forceinline__ void pack_block(const LmpcLoopDev &L, const LoopBlock blk, Value value)
{
    const LoopBlockShape s = lmpc_loop_block_shape(L, blk);
    const LoopBlockBuf buf = lmpc_loop_block_buf(L, blk);
    const int ipw = L.ipw;
    const bool per_instance = buf.ts != 0;
    const size_t first = (size_t)blockIdx.x * kPackThreads + threadIdx.x, step = (size_t)gridDim.x * kPackThreads;
    const size_t width = (size_t)ipw * s.rows, per_tile = (size_t)s.terms * width, total = lmpc_loop_block_len(L, blk);
    double LOOP_GAS *out = gout(buf.p);
    for (size_t idx = first; idx < total; idx += step) {
        const size_t t = idx / per_tile, rem = idx - t * per_tile;
        const int j = (int)(rem / width), qi = (int)(rem - j * width);
        const int q = qi / s.rows, i = qi - q * s.rows;
        const size_t b = per_instance ? t * ipw + q : 0;
        out[idx] = b < (size_t)L.batch ? value(b, j, i) : 0.0;
    }
}

// The model of instance b's controller is the handle's, or in a bank the struct of the controller the instance uses; column-major all.
// Column j, row i of its [A | B | Bd] ...
__device__ __forceinline__ double state_coeff(const LmpcLoopDev &L, const size_t b, const int j, const int i)
{
    const int nx = L.nx, nu = L.nu;
    const auto of = [=](const double *A, const double *Bm, const double *Bd) {
        return j < nx ? A[j * nx + i] : j < nx + nu ? Bm[(j - nx) * nx + i] : Bd[(j - nx - nu) * nx + i];
    };
    if (L.mA) return of(L.mA, L.mB, L.mBd);
    const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
    return of(M.A, M.B, M.Bd);
}
// ... and of its [C | Dd]
__device__ __forceinline__ double output_coeff(const LmpcLoopDev &L, const size_t b, const int j, const int i)
{
    const int nx = L.nx, ny = L.ny;
    const auto of = [=](const double *Cm, const double *Dd) { return j < nx ? Cm[j * ny + i] : Dd[(j - nx) * ny + i]; };
    if (L.mC) return of(L.mC, L.mDd);
    const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
    return of(M.C, M.Dd);
}
// column c, row r of instance b's observer gain [ldg x ny], column-major: the one for the batch, or the caller's per-instance array
__device__ __forceinline__ double gain_coeff(const LmpcLoopDev &L, const int ldg, const size_t b, const int c, const int r)
{
    return L.gain_batch ? gin(L.gain_batch)[(b * L.ny + c) * ldg + r] : L.gain[c * ldg + r];
}

// The plants of a loop that has one per instance, from the caller's array ([B x nx (nx + nu + ndu)], A_b | B_b | Bd_b column-major: term j of
// instance b is the run of nx doubles at (b nterms + j) nx) or from each instance's controller.  And each controller's own exogenous input, step 0,
// as the [B x ndu] array the advance kernel addresses per instance.
__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_plants_kernel(const LmpcLoopDev L)
{
    if (L.pk) {
        const size_t nterms = (size_t)lmpc_loop_block_shape(L, kPlantBlock).terms;
        const int nx = L.nx;
        pack_block(L, kPlantBlock, [&](const size_t b, const int j, const int i) {
            return L.pk_src ? gin(L.pk_src)[(b * nterms + j) * nx + i] : state_coeff(L, b, j, i);
        });
    }
    if (L.d_own) {
        const int ndu = L.ndu;
        const size_t first = (size_t)blockIdx.x * kPackThreads + threadIdx.x, step = (size_t)gridDim.x * kPackThreads;
        for (size_t idx = first; idx < (size_t)L.batch * ndu; idx += step) {
            const size_t b = idx / ndu;
            const LmpcDev &M = L.models[L.model_index ? L.model_index[b] : (int)b];
            gout(L.d_own)[idx] = M.dmeas_s[idx - b * ndu];
        }
    }
}

// The blocks of an observed loop: the plant where it is one for the batch (one tile from the row-major `plant`), the estimator [A | B | Bd | L] and
// the measurement [C | Dd].  kOff, an offset-free loop: the gain is [(nx + ndu) x ny], its first nx rows the estimator block's, the others Ld's.
template <bool kOff>
__device__ __forceinline__ void pack_observer(const LmpcLoopDev &L)
{
    const int nx = L.nx, nu = L.nu, ndu = L.ndu;
    const int npl = nx + nu + ndu;
    const int ldg = kOff ? nx + ndu : nx;         // rows of a gain
    if (!L.pk) {                                  // one plant for the batch: one tile of it, from the row-major `plant`
        const double *Ap = L.plant, *Bp = Ap + nx * nx, *Dp = Bp + nx * nu;
        pack_block(L, kPlantBlock, [&](const size_t, const int j, const int i) {
            return j < nx ? Ap[i * nx + j] : j < nx + nu ? Bp[i * nu + (j - nx)] : Dp[i * ndu + (j - nx - nu)];
        });
    }
    pack_block(L, kEstimatorBlock, [&](const size_t b, const int j, const int i) { return j < npl ? state_coeff(L, b, j, i) : gain_coeff(L, ldg, b, j - npl, i); });
    pack_block(L, kMeasurementBlock, [&](const size_t b, const int j, const int i) { return output_coeff(L, b, j, i); });
    if constexpr (kOff) pack_block(L, kDisturbanceGainBlock, [&](const size_t b, const int j, const int i) { return gain_coeff(L, ldg, b, j, nx + i); });
}

__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_observer_kernel(const LmpcLoopDev L) { pack_observer<false>(L); }
__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_offset_free_kernel(const LmpcLoopDev L) { pack_observer<true>(L); }

// ... and of a loop with targets, behind the two above: T from the one map for the batch or the caller's per-instance array, both column-major
// [nu x nrhs]
__global__ __launch_bounds__(kPackThreads) void lmpc_loop_pack_target_kernel(const LmpcLoopDev L)
{
    const int nu = L.nu, nrhs = L.ny + L.ndu + L.nu;
    pack_block(L, kTargetMapBlock, [&](const size_t b, const int j, const int i) {
        return L.tmap_batch ? gin(L.tmap_batch)[(b * nrhs + j) * nu + i] : L.tmap[j * nu + i];
    });
}

inline int odd(int n) { return n | 1; }

// Which advance kernel a loop runs, on how many blocks of one wavefront, with how much dynamic LDS
struct AdvanceLaunch { LoopKernel kernel; unsigned grid; size_t lds; };
AdvanceLaunch advance_launch(const LmpcLoopDev &L)
{
    const unsigned tiles = (unsigned)lmpc_loop_tiles(L);
    if (L.ek) {                                   // an instance's row of operands, ipw of them
        const LoopKernel kernel = L.tgt ? lmpc_loop_advance_offset_free_target_kernel : L.dobs ? lmpc_loop_advance_offset_free_kernel : lmpc_loop_advance_observed_kernel;
        return {kernel, tiles, (size_t)L.ipw * L.so * sizeof(double)};
    }
    if (L.pk) return {lmpc_loop_advance_plants_kernel, tiles, (size_t)L.ipw * L.sv * sizeof(double)};      // [x | cmd | d] of ipw instances
    return {lmpc_loop_advance_kernel, (unsigned)((L.batch + kTile - 1) / kTile), (size_t)kTile * (2 * L.sx + L.su + L.sd) * sizeof(double)};   // x, cmd, d and x+ of 64
}

// blocks of a pack launch over n elements
dim3 pack_grid(const size_t n)
{
    const size_t blocks = (n + kPackThreads - 1) / kPackThreads;
    return dim3((unsigned)(blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks));
}

}  // namespace

// (nx <= 64: ipw >= 1 instances of nx lanes each fill, or nearly fill, the wavefront)
void lmpc_loop_plan_lds(LmpcLoopDev &L)
{
    L.sx = odd(L.nx); L.su = odd(L.nu); L.sd = L.ndu > 0 ? odd(L.ndu) : 0;
    L.ipw = L.nx < kTile ? kTile / L.nx : 1; L.sv = odd(L.nx + L.nu + L.ndu);
    L.so = odd(2 * L.nx + L.nu + L.ndu + L.ny + (L.dobs ? L.ndu : 0) + (L.tgt ? L.ny + L.ndu + L.nu : 0));
}

int lmpc_loop_prepare(const LmpcLoopDev &L)
{
    const AdvanceLaunch a = advance_launch(L);
    if (a.lds > lmpc_lds_limit()) return -2;
    if (a.lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(a.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds) != hipSuccess) return -3;
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
    const size_t n = L.pk ? lmpc_loop_block_len(L, kPlantBlock) : (size_t)L.batch * L.ndu;
    hipLaunchKernelGGL(lmpc_loop_pack_plants_kernel, pack_grid(n), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_pack_observer(const LmpcLoopDev &L, void *stream)
{
    if (!L.ek) return 0;
    size_t n = 0;                                 // the first kernel fills several blocks: a grid for the longest
    for (const LoopBlock b : {kEstimatorBlock, kMeasurementBlock, kDisturbanceGainBlock})
        if (lmpc_loop_block_buf(L, b).p && lmpc_loop_block_len(L, b) > n) n = lmpc_loop_block_len(L, b);
    const LoopKernel pack = L.dobs ? lmpc_loop_pack_offset_free_kernel : lmpc_loop_pack_observer_kernel;
    hipLaunchKernelGGL(pack, pack_grid(n), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    if (L.tgt)
        hipLaunchKernelGGL(lmpc_loop_pack_target_kernel, pack_grid(lmpc_loop_block_len(L, kTargetMapBlock)), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lmpc_loop_advance(const LmpcLoopDev &L, void *stream)
{
    const AdvanceLaunch a = advance_launch(L);
    hipLaunchKernelGGL(a.kernel, dim3(a.grid), dim3(kTile), a.lds, reinterpret_cast<hipStream_t>(stream), L);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mpcx
