// POD views of the device-resident controller handed to the HIP kernels.
//
// HBM layout (all doubles, zero padded; every leading dimension is even so a lane
// can fetch an element pair with one 16-byte load):
//   H, Kinv : nz columns x ldz rows, column-major (both symmetric)
//   Gr      : row r of G contiguous   [ldg x ldz]  -> G' v  (lanes own elements of nz)
//   Gc      : column j of G contiguous [ldz x ldg] -> G x   (lanes own rows of G)
//   Y       : [ldy x ldy], ldy = ldz + ldg, the dual Hessian N Hinv N' with N = [I; G];
//             unified index q: box variable e -> q = e, general row r -> q = ldz + r
// A vector of length n is held by a wavefront as element pairs: lane l owns elements
// 128*c + 2*l and 128*c + 2*l + 1 for c < CP (CP = ceil(n / 128)).
#pragma once

#include <atomic>
#include <cstdint>
#include <initializer_list>

namespace mpcx {

constexpr int kMaxActive = 28;          // working-set capacity of the in-kernel polish
constexpr int kSld = kMaxActive + 1;    // LDS row stride of the Schur complement
// the most rows a working set can hold and still be independent: nz of them, and every soft general row on top -- its 1 / rho on the diagonal of
// the dual Hessian keeps the Schur complement regular whatever else is in the set; never more than there are rows
__host__ __device__ inline int ws_limit(int nz, int mg, int n_soft) { return nz + (n_soft < mg ? n_soft : mg); }
// capacity of the fallback polish's working-set lists (indices, bounds, multipliers) for that limit; the Schur complement of a set of more than
// kMaxActive rows goes to a device buffer of one limit x limit slot per wavefront.  Without soft rows: nz, as it has always been
__host__ __device__ inline int ws_capacity(int limit) { return limit > kMaxActive ? limit : kMaxActive; }

// what a general row bounds (g_kind, f_kind; step and comp say where along the predicted trajectory)
// G_RATE: a bound on the input increment delta_i = v_{i+1} - v_i (the reference's delta-u rows, ProblemBuilder.hpp:768-793); step = i + 1
// G_LINEAR: row comp of the linear rows lo <= Fx x_i + Fu v_i <= hi (no counterpart in the reference), the scalar row's convention
enum GKind : int { G_STATE = 0, G_OUTPUT = 1, G_SCALAR = 2, G_RATE = 3, G_LINEAR = 4 };

struct LmpcDev {
    int nx, nu, ndu, ny, ph, ch, nf, nz, mg;
    int ldz, ldg, ldy;
    int m_ref, neq_ref, active_words;
    int has_dist, n_fixed;
    // solver parameters
    int max_iter, polish, check_every, polish_rounds0, polish_rounds;
    int cost_direct;                             // 1: cost from its definition (regularised Hessian), 0: from the multipliers
    int cond_status;                             // device-side condensing (lmpc_condense_models): 0 fine; bit 0: the condensed Hessian is not positive
                                                 // semidefinite; bit 1: the ADMM matrix is not positive definite; bit 2: a kept row of G is identically
                                                 // zero (the controller's constraint structure differs from controller 0's)
    int strict_infeasible;                       // 1: report INFEASIBLE / NaN; 0: behave as the reference does
    int n_soft;                                  // soft general rows (in what was padding: every other field keeps its offset)
    double alpha, sigma, eps_abs, eps_rel, eps_prim_inf;
    int adaptive_rho; double rho_user;            // LParameters::adaptive_rho / rho (the ADMM step sizes of the set-up).  adaptive_rho is a flag word: bit 0
                                                 // the parameter (MPCX_ADAPTIVE_RHO), bit 1 the terminal cost's presence (MPCX_HAS_TERMINAL), bits 2 .. 7 the number of
                                                 // linear rows (MPCX_LINEAR_NC) -- only the condensing kernel and the launch of the generic assemble kernel
                                                 // (its template parameters TERM and LIN) read those
    // per-wave LDS carve (in doubles)
    int stage_len, arena_len, lds_per_wave;
    int fast_slice;                              // per-wave LDS slice of the lean solve kernels (doubles)
    int wsld;                                    // per-instance workspace record (doubles): f | t0 | gt0 | lg | ug | c0, flag
    // model, column-major
    const double *A, *B, *C, *Bd, *Dd;
    const double *Wy, *Wu, *Wdu;                 // [(ph+1) x ny], [(ph+1) x nu], [ph x nu]; column = internal step.  Wy: then MPCX_TERMINAL, if present
    const double *yref_s, *uref_s, *duref_s, *dmeas_s;   // shared references [ph x n]
    // step-0 feasibility rows
    const double *lo0x, *hi0x, *lo0u, *hi0u, *lo0y, *hi0y, *sX, *sU;      // sX: then MPCX_LINEAR_F, if present
    double s0lo, s0hi;
    // condensed QP
    const double *H, *Kinv, *Gr, *Gc, *Y;
    const double *lw, *uw, *rho_b;               // [ldz]
    const double *lg0, *ug0, *rho_g;             // [ldg]; rho_g [2 ldg]: the step sizes, then MPCX_G_SOFT
    const int *g_kind, *g_step, *g_comp, *g_refrow;      // [ldg]
    const int *f_kind, *f_step, *f_comp; const double *f_lo, *f_hi;   // fixed rows [n_fixed]
    const int *boxrow_ptr, *boxrow_ref; const double *boxrow_lo, *boxrow_hi;
    const int *blk;                              // [ph+1]
    // stacked maps of the MFMA assemble kernel (see Condensed in lmpc_model.hpp)
    int kin, nxp, nup, nyp, ione, nz16, mg16, ns, ns16, kq16, rowsA, ldy16;
    const double *MA0, *MA1, *Ym, *slo, *shi;
    // the same maps as lmpc_solve_group takes them (lmpc_pack_mfma_tiles): a lane's A operands of four consecutive k-steps side by side, a wavefront's of
    // one row tile and k-step group 2 KB in a row -- the phase is bound by the vector memory pipe's instruction rate, not by bytes
    const double *MA0p, *MA1p, *Ymp;
    const double *Hp;                            // H the same way, nz16 x nz16 zero padded (lmpc_cost_mfma's operand; null unless cost_direct)
    // composed maps of the fused solve kernel: rows [t0; gt0 (ldy) | goff (ldg) | f (ldz) | feasibility rows (nsp) | Qc vin (kin)]
    int rowsF, nsp, fused_ok, group_ok;
    const double *MF0, *MF1;
};
// 1 / weight of a soft general row, 0 for a hard one and the padding, [ldg]: it rides behind the step sizes in rho_g's array.  The struct travels by
// value in lmpc_solve_group's kernel arguments, sixteen cache lines to the byte (kernarg_touch): it has room for an int, not for a pointer
#define MPCX_G_SOFT(M) ((M).rho_g + (M).ldg)
// The terminal cost rides the same way: its presence in bit 1 of the flag word adaptive_rho, its data behind the output weights in
// Wy's array, [Wy (ph + 1) ny | P nx nx | xT nx | Tx nx (ny + ndu)], all column-major; without the term the array ends with the weights
#define MPCX_ADAPTIVE_RHO(M) (((M).adaptive_rho & 1) != 0)
#define MPCX_HAS_TERMINAL(M) (((M).adaptive_rho & 2) != 0)
#define MPCX_TERMINAL(M) ((M).Wy + ((M).ph + 1) * (M).ny)
// The linear rows likewise: their number in bits 2 .. 7 of the flag word, their coefficients behind the scalar row's in sX's array,
// [sX nx | row c: Fx(c, :) nx, Fu(c, :) nu]; a zero-initialised struct has none.  Read by the condensing kernel and by the generic assemble kernel
// (its template parameter LIN, chosen by the launch)
#define MPCX_LINEAR_NC(M) (((M).adaptive_rho >> 2) & 63)
#define MPCX_LINEAR_F(M) ((M).sX + (M).nx)
__host__ __device__ inline int lmpc_terminal_len(int nx, int ny, int ndu) { return nx * nx + nx + nx * (ny + ndu); }

struct LmpcBatchDev {
    int batch;
    const double *x0, *u0;
    // reference accessors: value(b, k, a) = p[b*bs + k*ks + a]
    const double *yref; long yref_bs, yref_ks;
    const double *uref; long uref_bs, uref_ks;
    const double *duref; long duref_bs, duref_ks;
    const double *dmeas; long dmeas_bs, dmeas_ks;
    double *cmd, *cost;
    int32_t *status, *solver_status, *is_feasible, *iterations;
    uint32_t *active_lower, *active_upper;
    double *seq_state, *seq_output, *seq_input;
    int32_t *polish_rounds, *active_count;
    const uint32_t *warm_lower, *warm_upper;      // optional previous active sets (reference row numbering)
    int warm_shift;
    int fq_cap;                                   // entries the failure queue's list holds
    int fused;                                    // 0: record from the workspace; 1 / 2: lmpc_solve_fused with MF0 / MF1; 3 / 4: lmpc_solve_group with MA0 / MA1.  The kernels read this encoding; the host writes it in one place, LmpcPlan::fused (lmpc_launch copies it here)
    int *fq;                                      // failure queue (described below; lmpc_launch fills it in): the polish-first kernels list the instances they leave open, the fallback kernel serves the list.  Null when polish is switched off: the fallback then serves every instance
    int *pcounter;                                // work counter of the persistent fused kernel (lmpc_launch fills it in for the fused mat-vec form; null: one instance per launched wavefront)
    // heterogeneous batch (mpcx_lmpc_hetero_*): the kernels' model pointer is an array of n_models structs of identical dimensions and
    // constraint structure, instance b uses entry model_index[b] (null: entry b); 0 models = the one shared controller
    int n_models;
    const int32_t *model_index;
    long long *dbg_cycles;       // optional [B x 8] per-phase cycle counts (profiling aid)
};
// Both structs travel by value in lmpc_solve_group's kernel arguments, sixteen cache lines to the byte: a field added to either shows here first
static_assert(sizeof(LmpcDev) == 712 && sizeof(LmpcBatchDev) == 296, "LmpcDev / LmpcBatchDev changed size: see kernarg_touch (lmpc_fast.hip)");
// doubles of one wavefront's slot of the large-working-set buffer (LmpcScratch::pbuf)
__host__ __device__ inline size_t lmpc_slot_len(const LmpcDev &m) { const size_t n = (size_t)ws_limit(m.nz, m.mg, m.n_soft); return n * n; }
// which entry of the model array instance b uses
__host__ __device__ inline int lmpc_model_of(const LmpcBatchDev &Bt, int b) { return Bt.n_models <= 0 ? 0 : (Bt.model_index ? Bt.model_index[b] : b); }

// The failure queue, device resident, one per handle: [count, ticket, served_last, (pad) | list[cap]] ints.  A producer (lmpc_solve_group: once per
// workgroup; the other polish-first kernels: once per failing wavefront) takes `count` forward with one atomic and stores the indices of the instances
// it leaves open; one that leaves none touches nothing.  The fallback kernel returns at once when count is 0; otherwise wavefront w of W serves
// list[w], list[w + W], ..., every wavefront takes a ticket when it is through, and the last one files count under served_last and zeroes count
// and ticket.  Invariant: count == ticket == 0 between complete steps (a producer launched without the consumer behind it: lmpc_fallback_reset).
constexpr int kFqCount = 0, kFqTicket = 1, kFqServed = 2, kFqList = 4;
inline size_t lmpc_fallback_queue_bytes(size_t cap) { return (kFqList + cap) * sizeof(int); }
// wavefronts the fallback kernel launches after a polish pass (the largest count whose idle launch costs what the smallest does)
int lmpc_fallback_waves();
// stream-ordered zeroing of count and ticket
int lmpc_fallback_reset(int *fq, void *stream);

// LDS a workgroup of the current device may take (one CU's: gfx950 160 KB), asked of the runtime once per device -- implemented in lmpc_kernels.hip
size_t lmpc_lds_limit();
// implemented in lmpc_kernels.hip
int lmpc_kernel_variant(int ldz, int ldg);     // -1 if the dimensions are not covered
// One handle's scratch memory on the device, sized for batches of up to `cap` instances:
//   ws       per-instance workspace between assemble and solve, cap records of wsld doubles
//   fq       failure queue (above), a list of cap entries, count and ticket zeroed when allocated
//   pbuf     the fallback kernel's slots for working sets of more than kMaxActive rows, pslots (lmpc_fallback_slots) x limit x limit doubles (ws_limit); the
//            fallback's grid is capped at pslots wavefronts
//   pcounter work counters of the persistent fused kernel, eight ints (single-controller handles only; null in a bank)
struct LmpcScratch { double *ws; size_t cap; int *fq; double *pbuf; int pslots; int *pcounter; };
// grow-only: allocates anew when `batch` exceeds cap (not capturable in a graph: the first, plain solve of a batch size does it); the queue's header
// is zeroed in `stream`'s order.  with_pcounter: the counters come with the workspace, never later -- a launch under capture must not allocate.
// 0, or -3 (cap stays 0: the next call starts over)
int lmpc_scratch_reserve(LmpcScratch &s, const LmpcDev &m, int batch, bool with_pcounter, void *stream);
void lmpc_scratch_release(LmpcScratch &s);

// What one call launches, decided once by the caller (mpcx_capi.cpp: lmpc_plan) and only read by the launchers.
enum class LmpcAssemble { Generic, MfmaSharedYref, MfmaInstanceYref };      // roll-out kernel, or the MFMA kernel with a shared / per-instance-constant output reference
enum class LmpcForm { TwoKernels, FusedMatvec, Group };                     // assemble + lmpc_solve; lmpc_solve_fused / lmpc_solve_persistent; lmpc_solve_group
struct LmpcPlan {
    LmpcAssemble assemble;
    LmpcForm form;
    int fused;                                    // what LmpcBatchDev::fused is given: 0 for two kernels, 1 / 2 fused mat-vec, 3 / 4 group, the odd value for the shared reference
};
// which: bit 0 = assemble, bit 1 = polish-only solve, bit 2 = ADMM fallback (7 = the normal path; single bits are for per-kernel timing).
// The scratch must hold the batch (lmpc_scratch_reserve); without large-working-set slots such sets are left to ADMM.
int lmpc_launch(const LmpcDev &m, const LmpcDev *m_dev, const LmpcBatchDev &b, const LmpcScratch &scratch, void *stream, int which, const LmpcPlan &plan);
// slots of the large-working-set buffer (LmpcScratch::pbuf) to allocate for batches of up to `batch` instances: one per wavefront the fallback kernel launches (lmpc_fallback_waves,
// never more than instances), at most what fits in a fixed budget (at least one workgroup's)
int lmpc_fallback_slots(const LmpcDev &m, int batch);
int lmpc_lds_per_wave(const LmpcDev &m, int *stage_len, int *arena_len);
// src: rows x K column-major (rows a multiple of 16, K of 4) -> out[((t G + g) 64 + lane) 4 + e] = src[(4 (4 g + e) + kq) rows + 16 t + j] with lane = 16 kq + j,
// G = ceil(K / 16) k-step groups per row tile t (zero beyond K): what one wavefront's MFMA A operands of four k-steps look like in registers
void lmpc_pack_mfma_tiles(const double *src, int rows, int K, double *out);
inline size_t lmpc_packed_len(int rows, int K) { return (size_t)(rows / 16) * ((K + 15) / 16) * 256; }
int lmpc_fast_slice(const LmpcDev &m);          // needs wsld, kin, nx
size_t lmpc_group_lds_bytes(const LmpcDev &m);  // LDS block of lmpc_solve_group (0: no group form for the variant); needs fast_slice, kin, nz16, nu
// implemented in lmpc_fast.hip: the polish-first kernel of `form` on `stream`
int lmpc_launch_fast(const LmpcDev &m, const LmpcDev *m_dev, const LmpcBatchDev &b, double *ws, void *stream, LmpcForm form);
// testing aid (lmpc_fast.hip): in [nvec][64] -> out [nvec][4][64] = every lane of wave_sum, of wave_sum_full, and of the two-level sum (lanes l, l ^ 16,
// l ^ 32, l ^ 48) by __shfl_xor and by lane swaps; device pointers
int lmpc_debug_wave_reduce(const double *in, double *out, int nvec, void *stream);
// testing aid (lmpc_fast.hip): one working-set solve and update of the lean kernels (ws_solve_reg, one chunk) per wavefront, with the elimination by scalar
// lane reads and by DPP row broadcast: out [count][2][kWsProbeLen] = dep_at, lmax, lam [16], wv [64 lanes x 2], gw [64 lanes x 2] of each form (mpcx.h)
constexpr int kWsProbeLen = 2 + 16 + 128 + 128;
int lmpc_debug_ws_solve(const double *Y, int n, int ldy, int nz, const int *wsidx, const double *wsb, const int *na, const double *t0, double *out, int count,
                        void *stream);
// hipFuncAttributeMaxDynamicSharedMemorySize of `kernels` raised to `bytes` on the current device unless `cache` says it has been: one cache per
// set of kernels that are raised together, grow-only, an atomic per device (two host threads or two handles on different GPUs can neither skip
// nor tear the update).  0, or -3
struct LmpcLdsCache { std::atomic<size_t> bytes[64]; };
int lmpc_raise_dynamic_lds(LmpcLdsCache &cache, std::initializer_list<const void *> kernels, size_t bytes);
// implemented in lmpc_hetero.hip: the O(n^3) arrays of `count` model structs (device array) computed in place, one workgroup each;
// -2: the dimensions do not fit the kernel's LDS plan (the bank then condenses on the host)
size_t lmpc_condense_lds(const LmpcDev &m, int *NP_out, int *NQ_out, size_t *big_out = nullptr);
int lmpc_condense_launch(LmpcDev *models_d, const LmpcDev &m0, int count, void *stream);

// Sensitivities of a solved batch (lmpc_sens.hip).  All device pointers, laid out as mpcx_lmpc_sens documents them
struct LmpcSensArgs {
    int batch;
    bool jacobian;                                // the nu unit seeds on cmd; otherwise one seed per instance from seed_cmd / seed_input
    const uint32_t *active_lower, *active_upper;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    double *d_x0, *d_u0, *d_yref;
    int32_t *flags;
};
// the kernel's shared MFMA operand, the transpose of MF1's t0 rows packed by lmpc_pack_mfma_tiles: its length in doubles (out null), or filled in
size_t lmpc_sens_operand(int nz, int kin, int rowsF, const double *MF1, double *out);
// 0; -2: not even a working set of one row fits the LDS plan; -3: a launch or its configuration failed
int lmpc_sens_launch(const LmpcDev &m, const LmpcDev *m_dev, const double *T0p, const LmpcSensArgs &a, void *stream);

// The same for a bank (lmpc_bank_sens.hip): instance b on models[model_index[b]] (null map: entry b), as lmpc_model_of reads a batch
struct LmpcBankSensArgs {
    LmpcSensArgs s;
    const LmpcDev *models;                        // the bank's model structs (device array)
    const int32_t *model_index;
    int n_models;
};
// m: controller 0 (dimensions; the same for every controller of a bank).  0; -2: not even a working set of one row fits the LDS plan; -3: a launch
// or its configuration failed
int lmpc_bank_sens_launch(const LmpcDev &m, const LmpcBankSensArgs &a, void *stream);

// Gradients of a bank's solved batch with respect to the weights, the bounds and the model of each instance's controller (lmpc_bank_grad.hip,
// DESIGN.md 4.10b).  All device pointers; the references as LmpcBatchDev's accessors, a null array (bs = 0) being each controller's own.  One seed
// per instance.  d_*: [B x ..] per instance, laid out as LmpcParamSensArgs / LmpcModelSensArgs; c_*: [K x ..] per controller, row k the sum of the
// rows of controller k's instances whose flag is 0 in the order of group_order[group_offsets[k] .. group_offsets[k + 1]) (a second kernel that
// reads the d_* arrays: every c_* needs its d_*)
struct LmpcBankGradArgs {
    int batch;
    const uint32_t *active_lower, *active_upper;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    const double *u0, *seq_state, *seq_output, *seq_input;      // of the solved batch; seq_state only where a model output is asked for
    const double *yref; long yref_bs, yref_ks;
    const double *uref; long uref_bs, uref_ks;
    const double *duref; long duref_bs, duref_ks;
    const double *dmeas; long dmeas_bs, dmeas_ks;
    double *d_oweight, *d_uweight, *d_duweight, *d_lower, *d_upper;
    double *d_A, *d_B, *d_C, *d_Bd, *d_Dd;        // column-major; d_Bd / d_Dd (and c_Bd / c_Dd) are ignored without exogenous inputs
    int32_t *flags;
    const LmpcDev *models;                        // the bank's model structs (device array)
    const int32_t *model_index;
    int n_models;
    const int32_t *group_order, *group_offsets;   // [B], [n_models + 1]
    double *c_oweight, *c_uweight, *c_duweight, *c_lower, *c_upper, *c_A, *c_B, *c_C, *c_Bd, *c_Dd;
    int32_t *n_used;                              // [n_models]
};
// m: controller 0 (dimensions; the same for every controller of a bank).  0; -2: not even a working set of one row fits the LDS plan; -3: a launch
// or its configuration failed
int lmpc_bank_grad_launch(const LmpcDev &m, const LmpcBankGradArgs &a, void *stream);

// Parameter sensitivities of a solved batch (lmpc_param_sens.hip).  All device pointers; the references as LmpcBatchDev's accessors
struct LmpcParamSensArgs {
    int batch;
    bool reduce;                                  // the outputs summed over the batch (through `partials`) instead of one set per instance
    const uint32_t *active_lower, *active_upper;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    const double *u0, *seq_output, *seq_input;    // of the solved batch
    const double *yref; long yref_bs, yref_ks;
    const double *uref; long uref_bs, uref_ks;
    const double *duref; long duref_bs, duref_ks;
    double *d_oweight, *d_uweight, *d_duweight, *d_lower, *d_upper;
    int32_t *flags, *n_used;
    double *partials;                             // reduce: lmpc_param_sens_partials(m, batch) doubles
};
// Cq, the derivative of the outputs of the steps 1 .. ph with respect to the decision vector, [rows16 x nz] column-major (rows16 = ny ph rounded up to
// the MFMA row tile; what lmpc_pack_mfma_tiles takes): its length in doubles (out null), or filled in.  A, B, C column-major on the host
size_t lmpc_param_sens_cq(int nx, int nu, int ny, int ph, int nz, const double *A, const double *B, const double *C, const int *blk, double *out);
size_t lmpc_param_sens_partials(const LmpcDev &m, int batch);
// 0; -2: not even a working set of one row fits the LDS plan; -3: a launch or its configuration failed (reduce without partials among them)
int lmpc_param_sens_launch(const LmpcDev &m, const LmpcDev *m_dev, const double *Cqp, const LmpcParamSensArgs &a, void *stream);

// Model sensitivities of a solved batch (lmpc_model_sens.hip).  All device pointers; the references as LmpcBatchDev's accessors
struct LmpcModelSensArgs {
    int batch;
    bool reduce;                                  // the outputs summed over the batch (through `partials`) instead of one set per instance
    const uint32_t *active_lower, *active_upper;
    const int32_t *status;
    const double *seed_cmd, *seed_input;
    const double *u0, *seq_state, *seq_output, *seq_input;      // of the solved batch
    const double *yref; long yref_bs, yref_ks;
    const double *uref; long uref_bs, uref_ks;
    const double *duref; long duref_bs, duref_ks;
    const double *dmeas; long dmeas_bs, dmeas_ks;
    double *d_A, *d_B, *d_C, *d_Bd, *d_Dd;        // column-major, [B x ..] or one set (reduce); d_Bd / d_Dd are ignored without exogenous inputs
    int32_t *flags, *n_used;
    double *partials;                             // reduce: lmpc_model_sens_partials(m, batch) doubles
};
// Xq, the derivative of the states of the steps 1 .. ph with respect to the decision vector, [rows16 x nz] column-major (rows16 = nx ph rounded up to
// the MFMA row tile; what lmpc_pack_mfma_tiles takes): its length in doubles (out null), or filled in.  A, B column-major on the host
size_t lmpc_model_sens_xq(int nx, int nu, int ph, int nz, const double *A, const double *B, const int *blk, double *out);
size_t lmpc_model_sens_partials(const LmpcDev &m, int batch);
// 0; -2: not even a working set of one row fits the LDS plan; -3: a launch or its configuration failed (reduce without partials among them)
int lmpc_model_sens_launch(const LmpcDev &m, const LmpcDev *m_dev, const double *Xqp, const LmpcModelSensArgs &a, void *stream);

// The closed loop around the solve (lmpc_loop.hip): everything the advance kernel touches. All device pointers; the same struct at every tick.
// The packed blocks: per-instance coefficients in the order the advance kernels read them (lmpc_loop.hip, DESIGN 4.3b has the table)
enum LoopBlock : int {
    kPlantBlock,                                  // [A_p | B_p | Bd_p] of the instance's plant
    kEstimatorBlock,                              // [A | B | Bd | L] of the instance's controller
    kMeasurementBlock,                            // [C | Dd] of the instance's controller
    kDisturbanceGainBlock,                        // Ld of the instance's controller
    kTargetMapBlock,                              // T of the instance's controller
    kLoopBlocks
};
struct LoopBlockShape { int terms, rows; };       // a block is `terms` columns of `rows` coefficients per instance
struct LoopBlockBuf { double *p; long ts; };      // null: the loop has no such block; tile stride 0: one tile
struct LmpcLoopDev {
    int batch, ticks, nx, nu, ndu, ph, aw;        // aw: active-set words per instance
    int sx, su, sd;                               // LDS row strides of the state, command and exogenous-input tiles (lmpc_loop_plan_lds)
    const double *plant;                          // [A_p (nx x nx) | B_p (nx x nu) | Bd_p (nx x ndu)], each row-major: read by scalar loads
    // per-instance plants (pk null: the one plant above)
    int ipw, sv;                                  // instances per wavefront where a lane is an (instance, row), LDS stride of an instance's [x | cmd | d] (lmpc_loop_plan_lds)
    double *pk;                                   // the plant block with a tile per ipw instances, written by lmpc_loop_pack_plants
    const double *pk_src;                         // the caller's [B x nx (nx + nu + ndu)], A_b | B_b | Bd_b column-major; null: each instance's controller
    const LmpcDev *models;                        // a bank's model structs and its instance -> controller map (null map: instance b = controller b)
    const int32_t *model_index;
    double *d_own;                                // [B x ndu]: step 0 of each controller's own exogenous input (a bank's "shared" mode), or null
    const double *x0, *u0;                        // the caller's initial state and last input (read by lmpc_loop_begin)
    double *x, *u;                                // the loop's current state and last input: what the solve reads as x0 / u0
    const double *dmeas; long d_bs, d_tick;       // d_k of instance b, component a: dmeas[b * d_bs + k * d_tick + a]
    const double *noise;                          // [ticks x B x nx] or null
    // the solve's results of the tick ...
    const double *cmd, *cost;
    const int32_t *status, *solver_status, *iterations, *polish_rounds, *active_count;
    const uint32_t *active_lower, *active_upper;
    uint32_t *warm_lower, *warm_upper;            // ... its active sets copied here for the next solve (null: no carry)
    // ... logged tick-major; traj_x [(ticks + 1) x B x nx], traj_u [ticks x B x nu], the others [ticks x B] or null
    double *traj_x, *traj_u, *traj_cost;
    int32_t *traj_status, *traj_solver_status, *traj_iterations, *traj_polish_rounds, *traj_active_count;
    // preview references (yref, uref, duref, dmeas): source [B x (ticks + ph) x n], staging [B x ph x n]; null source: not a preview array
    const double *pv_src[4]; double *pv_dst[4]; int pv_n[4];
    int *state;                                   // [tick, blocks of the running advance kernel that are through]
    // observed loops (ek null: none): x above is then the estimate -- what the solve reads -- and xt the plant's true state.  The packed blocks
    // (LoopBlock above; reached by name here and through lmpc_loop_block_buf) are written by lmpc_loop_pack_observer; a tile stride of 0: one tile,
    // the same for every instance, read by every block of a launch
    int ny, so;                                   // outputs; LDS stride of an instance's [x | xhat | cmd | d | e] (lmpc_loop_plan_lds)
    double *xt;
    double *ok; long ok_ts;                       // the plant [A_p | B_p | Bd_p]: pk (a plant per instance; set with pk in every such loop), or one tile packed from `plant`
    double *ek; long ek_ts;                       // the estimator [A | B | Bd | L] of the instance's controller
    double *mk; long mk_ts;                       // the measurement [C | Dd] of the instance's controller
    const double *mA, *mB, *mBd, *mC, *mDd;       // a handle's model on the device, column-major (null in a bank: models / model_index)
    const double *gain, *gain_batch;              // [nx x ny] one gain for the batch, or [B x nx ny] a gain per instance; column-major
    const double *xhat0;                          // [B x nx] or null (= x0), read by lmpc_loop_begin
    const double *meas_noise;                     // [ticks x B x ny] or null
    double *traj_xhat, *traj_y;                   // [(ticks + 1) x B x nx], [ticks x B x ny], or null
    // offset-free loops (dobs 0: none): an observed loop whose estimator carries [xhat; dhat].  dmeas above is then the true disturbance, which drives
    // the plant and the measurement and which the controller does not see; the solve reads dhat as its per-instance exogenous input; gain and
    // gain_batch are [(nx + ndu) x ny], rows 0 .. nx - 1 the estimator block's L, the others Ld
    int dobs;                                     // (before lmpc_loop_plan_lds: so is then the stride of [x | xhat | cmd | dhat | e | d])
    double *dhat;                                 // [B x ndu]
    double *dk; long dk_ts;                       // Ld of the instance's controller
    const double *dhat0;                          // [B x ndu] or null (= 0), read by lmpc_loop_begin
    double *traj_dhat;                            // [(ticks + 1) x B x ndu] or null
    // steady-state targets (tgt 0: none; needs dobs): us = T [r; dhat; ubar] with T [nu x (ny + ndu + nu)] column-major is what the solve reads as its
    // per-instance uref.  r and ubar are step 0 of the tick's yref and uref: value(b, k, a) = src[b * bs + k * tick + a]; a null source is a bank's
    // "shared" mode, each controller's own (models / model_index)
    int tgt;                                      // (before lmpc_loop_plan_lds: so then also holds [r | dhat+ | ubar] of tick k + 1)
    double *us;                                   // [B x nu]
    double *tk; long tk_ts;                       // T of the instance's controller
    const double *tmap, *tmap_batch;              // one map for the batch (device copy), or the caller's [B x nu nrhs]
    const double *r_src; long r_bs, r_tick;
    const double *ub_src; long ub_bs, ub_tick;
    double *traj_us;                              // [(ticks + 1) x B x nu] or null
};
// The one description of a packed block; its length, its tile stride, the pack launches and what the kernels index with all derive from it
__host__ __device__ inline LoopBlockShape lmpc_loop_block_shape(const LmpcLoopDev &L, LoopBlock b)
{
    switch (b) {
    case kPlantBlock: return {L.nx + L.nu + L.ndu, L.nx};
    case kEstimatorBlock: return {L.nx + L.nu + L.ndu + L.ny, L.nx};
    case kMeasurementBlock: return {L.nx + L.ndu, L.ny};
    case kDisturbanceGainBlock: return {L.ny, L.ndu};
    default: return {L.ny + L.ndu + L.nu, L.nu};  // kTargetMapBlock
    }
}
// ... and where it lies.  The blocks keep a named pointer and stride each, where they have always been in the struct: the advance kernels hold most
// of it in scalar registers, and how many of those spill has followed every move of a field (profiles/loop_refactor.txt)
__host__ __device__ inline LoopBlockBuf lmpc_loop_block_buf(const LmpcLoopDev &L, LoopBlock b)
{
    switch (b) {
    case kPlantBlock: return {L.ok, L.ok_ts};
    case kEstimatorBlock: return {L.ek, L.ek_ts};
    case kMeasurementBlock: return {L.mk, L.mk_ts};
    case kDisturbanceGainBlock: return {L.dk, L.dk_ts};
    default: return {L.tk, L.tk_ts};              // kTargetMapBlock
    }
}
__host__ __device__ inline size_t lmpc_loop_tiles(const LmpcLoopDev &L) { return (size_t)((L.batch + L.ipw - 1) / L.ipw); }
// doubles of a tile (ipw instances, the last tile padded): the tile stride of a block that differs from instance to instance
__host__ __device__ inline size_t lmpc_loop_tile_len(const LmpcLoopDev &L, LoopBlock b)
{
    const LoopBlockShape s = lmpc_loop_block_shape(L, b);
    return (size_t)s.terms * L.ipw * s.rows;
}
// doubles of the block as its tile stride says: a tile per ipw instances, or one
__host__ __device__ inline size_t lmpc_loop_block_len(const LmpcLoopDev &L, LoopBlock b) { return (lmpc_loop_block_buf(L, b).ts ? lmpc_loop_tiles(L) : 1) * lmpc_loop_tile_len(L, b); }
void lmpc_loop_plan_lds(LmpcLoopDev &L);          // fills sx, su, sd, ipw, sv, so (ny, dobs and tgt before the call)
int lmpc_loop_prepare(const LmpcLoopDev &L);      // once per loop, outside any capture: 0, -2 (tiles larger than a CU's LDS), -3
int lmpc_loop_begin(const LmpcLoopDev &L, void *stream);
int lmpc_loop_pack_plants(const LmpcLoopDev &L, void *stream);   // head of every run, next to lmpc_loop_begin: fills a per-instance plant block and d_own (no launch without either)
int lmpc_loop_pack_observer(const LmpcLoopDev &L, void *stream);  // head of every run of an observed loop, behind lmpc_loop_pack_plants: fills every other block the loop has
int lmpc_loop_advance(const LmpcLoopDev &L, void *stream);

// The backward pass of a plain closed loop (lmpc_loop_grad.hip): everything its kernels touch.  All device pointers; the same
// struct at every backward tick.  The loop's own fields are copies of LmpcLoopDev's.
constexpr int kLoopGradSlots = 8;                 // d_oweight, d_uweight, d_duweight, d_A, d_B, d_C, d_Bd, d_Dd
struct LmpcLoopGradDev {
    int batch, ticks, nx, nu, ndu, ny, ph;
    int ipw, sg;                                  // instances per wavefront of the per-instance form; LDS stride of an instance's [lam | x | cmd | d | lam' | mu]
    const double *plant;                          // the one plant for the batch, row-major per matrix (read by scalar loads) ...
    const double *pk;                             // ... or the packed plant block of the loop's last run (null: the one plant)
    const double *traj_x, *traj_u, *u0;           // the loop's logged trajectories and the caller's last input
    const double *dmeas; long d_bs, d_tick;       // d_k as the loop reads it
    double *x, *u;                                // what the re-solve reads as x0 / u0: staged from the trajectories
    const double *pv_src[4]; double *pv_dst[4]; int pv_n[4];      // the loop's preview windows
    const double *seed_x, *seed_u;                // [(ticks + 1) x B x nx], [ticks x B x nu]; either may be null
    double *lam, *mu, *c;                         // lambda_{k+1} [B x nx], mu_{k+1} [B x nu], the cotangent on cmd_k [B x nu]
    const double *gx, *gu, *gy;                   // the tick's vector-Jacobian products [B x nx], [B x nu], [B x ny]
    const int32_t *tflags; int ntf;               // the tick's flags, [ntf x B]: one row per launch of the tick
    const double *tick_out[kLoopGradSlots];       // the tick's per-instance weight and model gradients [B x len] (null: not asked for) ...
    double *acc[kLoopGradSlots]; int len[kLoopGradSlots];         // ... and what they are added into
    double *a_yref, *a_plant;                     // [B x ny], [B x nx (nx + nu + ndu)] accumulators, or null
    double *d_noise, *d_x0, *d_u0;                // [ticks x B x nx], [B x nx], [B x nu], or null
    int32_t *flags;                               // [B]: the OR over the ticks
    int *state;                                   // [tick, blocks of the running adjoint kernel that are through]
};
// the reduced form's sums over the instances whose flag is 0: up to five arrays [B x len] -> partials [groups x plen] -> dst, the count last
struct LmpcLoopGradSum {
    const double *src[5]; double *dst[5]; int len[5];
    const int32_t *flags; int batch;
    double *part; int32_t *n_used;
};
constexpr int kLoopGradGroup = 64;                // instances a workgroup of the partial sums adds up
inline size_t lmpc_loop_grad_plen(const LmpcLoopGradSum &s) { size_t n = 1; for (int k = 0; k < 5; ++k) n += (size_t)s.len[k]; return n; }
inline size_t lmpc_loop_grad_groups(int batch) { return (size_t)((batch + kLoopGradGroup - 1) / kLoopGradGroup); }
void lmpc_loop_grad_plan_lds(LmpcLoopGradDev &G); // fills sg (nx, nu, ndu before the call)
int lmpc_loop_grad_prepare(const LmpcLoopGradDev &G);             // once per handle, outside any capture: 0, -2 (tiles larger than a CU's LDS), -3
int lmpc_loop_grad_begin(const LmpcLoopGradDev &G, void *stream);
int lmpc_loop_grad_adjoint(const LmpcLoopGradDev &G, void *stream);
int lmpc_loop_grad_finish(const LmpcLoopGradDev &G, void *stream);                 // d_x0, d_u0, and NaN for the flagged instances
int lmpc_loop_grad_sum(const LmpcLoopGradSum &s, void *stream);                     // 0, -3

// Steady-state target maps (target_kernels.hip): the KKT system of each instance's target, one instance per wavefront, and the product with a map
size_t target_map_lds_bytes(int nx, int nu, int ndu, int ny);         // the augmented matrix [K | rhs] of one instance
// 0; -2: the augmented matrix exceeds lds_limit; -3: a launch or its configuration failed
int target_map_launch(int nx, int nu, int ndu, int ny, int batch, const double *A, const double *B, const double *Bd, const double *C, const double *Dd,
                      double *map_u, double *map_x, int *flags, size_t lds_limit, void *stream);
int target_apply_launch(int nu, int ndu, int ny, int batch, const double *map_u, int map_per_instance, const double *r, const double *dhat,
                        const double *ubar, double *us, void *stream);

}  // namespace mpcx
