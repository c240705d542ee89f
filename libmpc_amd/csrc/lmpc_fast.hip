// Lean polish kernels of the batched LMPC solve (see the comment at solve_fast); launched by lmpc_launch (lmpc_kernels.hip)
// through lmpc_launch_fast.
#include "lmpc_solve_common.hpp"
#include <cstddef>
#include <cstdlib>
#include <utility>

namespace mpcx {

namespace {

// =====================================================================================
// solve, lean form: the polish-only path of lmpc_solve, one instance per wavefront
// =====================================================================================
// The polish-first solve (OSQP's polish promoted to the main iteration, a verified
// point is the exact optimum), rebuilt around what the round-2 profile showed: the kernel is bound by the number of
// instructions a wavefront issues per round and by the rounds of the slowest instances, not by arithmetic.
//   * repair rule: wrong-signed rows leave AND violated rows enter in the same round (drop-then-add doubled the rounds of the
//     hard instances); the first working set holds the rows violated at the unconstrained optimum by at least 0.3 x the
//     largest violation, later rounds add from 0.2 x.  tools/activeset_sim.py, config 2, 32768 instances: mean 5.1 -> 3.5
//     rounds, maximum 12 -> 8.
//   * the Schur system is solved by Gauss-Jordan elimination with the right-hand side as an extra column, lane i owning row i:
//     no forward / backward substitution, no transposition through LDS, no predication -- 3 instructions per eliminated entry
//     (two v_readlane, one fma) instead of 5 plus two substitutions.  On the Schur complements of config 2 / config 4 its error
//     is that of the Cholesky factorisation (6e-15 relative).
//   * rows of Y the update w = t0 - Y[:, A] lambda needs are requested together with the Schur entries, before the elimination -- all of
//     them for working sets of up to six rows (one trip to L2 per round), the first four for up to twelve, none beyond; the rest follows
//     the elimination, pipelined (round 9, below).  The multipliers reach the update by v_readlane or, in the classes where that wins, from LDS (round 10); the working-set
//     indices are wave-uniform and live in SGPRs (scalar row addresses).
//   * wave-wide maxima by DPP operations -- four within the rows of sixteen lanes, two across them -- and one v_readlane pair (the
//     ds_bpermute butterfly of __shfl_xor is a chain of six LDS round trips);
//   * what a round only reads -- t0, G t0, the linear term and the bounds -- stays in LDS: the wave's slice has the layout of the
//     workspace record (f | t0 | gt0 | lg | ug | c0, flag) followed by a small arena, the box bounds are shared by the
//     workgroup.  The one-chunk variant fits 128 VGPRs and 3.3 KB of LDS per wavefront: four wavefronts per SIMD, i.e. at the
//     benchmark batch every instance is resident at once (the dispatch order no longer matters).
//   * round 8: no register spilled inside the round loop.  The compiler used to carry 134-160 SGPRs through the rounds in lanes of two VGPRs (the model
//     struct's fields for the unpack behind the loop, sixteen 64-bit row bases of the Schur loads, the sixteen masks lane == k and the identity's entries
//     for every size class, formed ahead of the loop) and paid a v_writelane / v_readlane for each use: 358 of the loop's 4 124 vector instructions, a sixth
//     of the sixteen-row class.  Now the Schur entries and the rows of Y are loaded as one scalar base plus a 32-bit byte offset, the lane-dependent masks are
//     formed where they are used, the later rows' indices are read from LDS again, lmpc_solve_group reads its arguments through the kernel-argument
//     pointer and once more behind the loop (fast_finish), and the pad of the Schur matrix is two moves per column under one execution mask with the
//     pivot threshold from one more load instead of a select chain per column.  No floating-point operation changed; profiles/r08_round_isa_census.txt.
//   * round 9: fewer exposed trips and a leaner verify phase.  The six-row class requests all its rows ahead of the elimination.  Behind the
//     elimination the remaining rows come in batches of two with three batches in flight, each batch requested before the one ahead of it is waited
//     for: one fresh trip in the 8- and 10-row classes, two in the 12-row class, three in the 14- and 16-row classes (they were 1, 2, 2, 4, 4; the
//     eight rows in flight that would make it one or two everywhere do not fit 128 VGPRs without scratch), and no branch in the update any more.
//     The verify phase's multiplier signs are bit arithmetic instead of four exec-mask ladders, the wave maximum's DPP moves no longer copy their source,
//     and viol()'s contractions are written out.  What is still not straight-line code there: the NaN screen, the "solved" test and the choice between
//     the two repair rules are wave-uniform branches.  No floating-point operation changed; profiles/r09_round_isa_census.txt.
//   * round 10: the broadcasts of ws_solve_reg off the vector pipe, behind a switch per size class (MPCX_FAST_LDSMULT_CLASSES below; the crossbar form of (2)
//     had one of its own until round 12 removed the form), each kept where it wins on the GPU.  (1) The update's multipliers read back from lam[] in LDS at wave-uniform addresses, two per 16-byte read, each read
//     travelling with the rows of Y it multiplies, instead of a v_readlane pair per row: on in the 8- and 10-row classes.  Whole step, parent -> this:
//     0.03414 -> 0.03359 ms, 0.03280 -> 0.03220 ms at --steps 2000.  In the 4- and 6-row classes it is within the noise of the scalar reads; in the 12- to
//     16-row classes the pairs in flight beside three batches of rows do not fit 128 VGPRs (12 B of scratch) and the step is 0.7 us SLOWER.  (2) The
//     elimination's pivot row and right-hand side through the LDS crossbar (ds_swizzle_b32, broadcast mode): built, measured, and OFF in every class.  A step's
//     FMAs wait for the crossbar, whose result the next step's pivot row depends on -- sixteen LDS round trips on the dependent chain where v_readlane's are a
//     few cycles each: the elimination phase goes from 790 to 1030 cycles per round in the 4-row class and from 2077 to 3038 in the 16-row class, the step
//     from 0.0346 to 0.0386 ms with every class on it (fewer vector instructions, but it is the slowest chain that ends the launch, and that chain is latency).
//     The elimination's steps are instances of one lambda over the step number either way (the crossbar's lane is an immediate).  No floating-point operation
//     changed; profiles/r10_round_ab.txt, r10_round_isa_census.txt.
//   * round 11: what a step runs outside the rounds.  The wave-wide sums there still went through the ds_bpermute butterfly of wave_sum -- the cost's sum in
//     fast_finish (the last thing the slowest instance does), the cost constant's two levels in front of the barrier between lmpc_solve_group's products, the
//     deal's key and rank: 42 ds_bpermute_b32 in lmpc_solve_group<1, 1>, sixteen dependent LDS round trips on every step's critical path.  They are lane swaps
//     (v_permlane32_swap / v_permlane16_swap) and DPP moves now, wave_sum_full below: the butterfly's own pairing tree, so the cost keeps its bits; the deal's
//     key, whose bits reach no result, takes the cheapest tree.  Against the same source with MPCX_FAST_DPP_SUMS 0, whole step, three runs each: 0.03396 ->
//     0.03334 ms, 0.03242 -> 0.03180 ms at --steps 2000, every run below every run of the other.  Tried with it and not kept, each level with "off" on the
//     GPU: the sixteen-term sums of the cost constants on the last wavefront instead of wavefront 0 (which has a tile of the second product); the fallback
//     launch's queue pointer as a preloaded kernel argument (one trip to memory for the idle exit test instead of two).  profiles/r13_head_ab.txt,
//     r13_head_isa_census.txt.
//   * round 12: the elimination's pivot row and right-hand side by DPP row broadcast inside the FMA -- v_fmac_f64_dpp row_newbcast:K, one vector instruction
//     per eliminated entry where the scalar form has two v_readlane_b32 and the FMA, no SGPR on the dependent chain (fmac_row_bcast, gj_step below: the
//     latency of a lane read, not of LDS, which is what round 10's crossbar form lacked; that form is gone).  Behind MPCX_FAST_DPP_CLASSES, a bit per size
//     class; both forms stay compiled in the probe kernel at the end of this file (mpcx_lmpc_debug_ws_solve), which holds them to the same bits.  No
//     floating-point operation changed; profiles/r14_round_dpp_ab.txt, r14_round_isa_census.txt.
// Working sets of more than kFastCap rows are left to the fallback kernel (none in 32768 instances of config 2, none in 8192 of
// config 4).
// How deep a round reaches into memory ahead of its arithmetic (ws_solve_reg).  Rows of Y requested with the Schur entries, ahead of the elimination:
// every row in the size classes up to MPCX_FAST_PF_ALL rows, MPCX_FAST_PF rows in the classes up to MPCX_FAST_PF_MAXCAP, none beyond (their elimination
// needs the registers).  The rows behind them come in batches after the elimination: MPCX_FAST_RB_DEEP rows per batch and MPCX_FAST_NBUF batches in flight
// where a row is cheap in registers (a lane holds at most MPCX_FAST_DEEP_CHUNKS pairs of a row: the one- and two-chunk variants), one batch of
// MPCX_FAST_RB rows at a time and no deeper first trip in the four-chunk variant, where a row is 32 VGPRs.
#ifndef MPCX_FAST_PF_MAXCAP
#define MPCX_FAST_PF_MAXCAP 12
#endif
#ifndef MPCX_FAST_RB
#define MPCX_FAST_RB 4
#endif
#ifndef MPCX_FAST_PF
#define MPCX_FAST_PF 4
#endif
#ifndef MPCX_FAST_PF_ALL
#define MPCX_FAST_PF_ALL 6
#endif
#ifndef MPCX_FAST_NBUF
#define MPCX_FAST_NBUF 3
#endif
#ifndef MPCX_FAST_RB_DEEP
#define MPCX_FAST_RB_DEEP 2
#endif
#ifndef MPCX_FAST_DEEP_CHUNKS
#define MPCX_FAST_DEEP_CHUNKS 4
#endif
// Which size classes of ws_solve_reg take their broadcasts off the scalar lane reads (rounds 10 and 12 in the comment above), two switches per class, each
// decided by measurement (profiles/r10_round_ab.txt, r14_round_dpp_ab.txt), never by round number at run time.  Bit CAP / 2 stands for the class of at most
// CAP rows (4, 6, ..., 16: bits 2 to 8).  MPCX_FAST_DPP_CLASSES: the elimination's pivot row and right-hand side taken by the FMA itself as a DPP row
// broadcast (its parameter DP; the one- and two-chunk variants -- a lane holds at most MPCX_FAST_DPP_CHUNKS pairs of a row -- of the kernels that read the
// record: where the resource listing shows more scratch with it, see solve_fast, the scalar reads stay).  MPCX_FAST_LDSMULT_CLASSES: the
// update's multipliers read back from LDS (XL; not in the kernels that compute the record themselves -- lmpc_solve_fused, lmpc_solve_persistent: they sit at
// their register budgets, see solve_fast -- and only in the variants whose lane holds at most MPCX_FAST_LDSMULT_CHUNKS pairs of a row, as before).
#ifndef MPCX_FAST_DPP_CLASSES
#define MPCX_FAST_DPP_CLASSES 0x1FC
#endif
#ifndef MPCX_FAST_DPP_CHUNKS
#define MPCX_FAST_DPP_CHUNKS 4
#endif
#ifndef MPCX_FAST_LDSMULT_CLASSES
#define MPCX_FAST_LDSMULT_CLASSES 0x30
#endif
#ifndef MPCX_FAST_LDSMULT_CHUNKS
#define MPCX_FAST_LDSMULT_CHUNKS 4
#endif
constexpr bool fast_class_bit(unsigned mask, int cap) { return ((mask >> (cap / 2)) & 1u) != 0; }
// between the stages of the pipelined update: the instruction scheduler moves nothing across (a batch's loads stay ahead of the wait for the batch before it)
#ifndef MPCX_FAST_STAGE
#define MPCX_FAST_STAGE() __builtin_amdgcn_sched_barrier(0)
#endif
constexpr int kFastCap = 16;
#ifndef MPCX_FAST_ADD_THETA_LATE
#define MPCX_FAST_ADD_THETA_LATE 0.02       // ... and from the fourth round on (the instances still open then are the ones that set the launch time)
#endif
#ifndef MPCX_FAST_SAFE_AFTER
#define MPCX_FAST_SAFE_AFTER 12       // rounds of the block repair rule before the single-exchange rule takes over
#endif

template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v)
{
    // a move whose `old` operand is not its source (there is none: a lane without a source reads 0): the destination is a fresh register, so no copy
    // of the source has to be made in front of the move to keep the source alive
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// maximum over the wavefront of non-NaN values, the same in every lane
__device__ __forceinline__ double wave_max_dpp(double v)
{
    v = fmax(v, dpp_mov_d<0xB1>(v));     // quad_perm [1,0,3,2]
    v = fmax(v, dpp_mov_d<0x4E>(v));     // quad_perm [2,3,0,1]
    v = fmax(v, dpp_mov_d<0x141>(v));    // row_half_mirror
    v = fmax(v, dpp_mov_d<0x140>(v));    // row_mirror: every row of 16 lanes is uniform now
    // across the rows towards lane 63: row r takes in the last lane of row r - 1, then rows 2 and 3 the last lane of row 1.  Rows without a source
    // take in a 0 and hold values nobody reads; lane 63 holds the maximum of all four rows and is read back -- one pair of v_readlane instead of four
    v = fmax(v, dpp_mov_d<0x142>(v));    // row_bcast:15
    v = fmax(v, dpp_mov_d<0x143>(v));    // row_bcast:31
    return readlane_d(v, 63);
}
// Round 11: the sums on the critical path outside the rounds -- the cost in fast_finish, the cost constant, the deal's key and rank in lmpc_solve_group --
// without the ds_bpermute butterfly of wave_sum (kernel_common), behind one switch for the A/B builds (profiles/r13_head_ab.txt).
#ifndef MPCX_FAST_DPP_SUMS
#define MPCX_FAST_DPP_SUMS 1
#endif
// v[l] + v[l ^ 32] (ROW16 false) or v[l] + v[l ^ 16] (ROW16 true) in every lane, by gfx950's lane swaps: the instruction exchanges the upper half (the odd
// rows of sixteen) of its first operand with the lower half (the even rows) of its second, so with v in both the first comes back as the lower partner in
// every lane and the second as the upper one.  The lanes of the upper half add their pair in the other order than the butterfly did: IEEE addition is
// commutative, signed zeros included, so the bits are the butterfly's (a NaN stays a NaN).  Every lane has to be active.
template <bool ROW16>
__device__ __forceinline__ double lane_swap_pair_sum(double v)
{
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    if constexpr (ROW16) {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    } else {
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    }
}
template <bool ROW16>
__device__ __forceinline__ int lane_swap_pair_sum(int v)
{
    if constexpr (ROW16) { const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); return (int)(r[0] + r[1]); }
    else { const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); return (int)(r[0] + r[1]); }
}
// Sum over the wavefront, the same in every lane and bit for bit wave_sum's: the same pairing tree in the same order (xor 32, 16, 8, 4, 2, 1), each level a
// lane swap or DPP moves instead of two ds_bpermute_b32 -- no LDS round trip on the chain.  xor 8 is a rotation of the row by eight; xor 4 is a rotation by
// twelve for the banks 0 and 2 of a row and by four for the banks 1 and 3, two moves into one register under complementary bank masks; xor 2 and xor 1 are
// quad permutations.  EVERY LANE HAS TO BE ACTIVE (a DPP move or a lane swap reads an inactive lane's register as it stands, or 0): it is called from
// wave-uniform code only -- fast_finish, lmpc_solve_group's head, the debug kernel below.  Everything else keeps wave_sum.
__device__ __forceinline__ double wave_sum_full(double v)
{
    v = lane_swap_pair_sum<false>(v);
    v = lane_swap_pair_sum<true>(v);
    v += dpp_mov_d<0x128>(v);            // row_ror:8
    {
        int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x12C, 0xF, 0x5, true);      // row_ror:12, banks 0 and 2
        int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x12C, 0xF, 0x5, true);
        lo = __builtin_amdgcn_update_dpp(lo, __double2loint(v), 0x124, 0xF, 0xA, false);  // row_ror:4, banks 1 and 3
        hi = __builtin_amdgcn_update_dpp(hi, __double2hiint(v), 0x124, 0xF, 0xA, false);
        v += __hiloint2double(hi, lo);
    }
    v += dpp_mov_d<0x4E>(v);             // quad_perm [2,3,0,1]
    v += dpp_mov_d<0xB1>(v);             // quad_perm [1,0,3,2]
    return v;
}
// the two-level form of lmpc_solve_group's head: the sum over the four lanes l, l ^ 16, l ^ 32, l ^ 48, paired as the two __shfl_xor levels paired them
// (16, then 32).  Every lane active.
template <typename T>
__device__ __forceinline__ T wave_sum_rows_swap(T v)
{
    v = lane_swap_pair_sum<true>(v);
    return lane_swap_pair_sum<false>(v);
}
template <typename T>
__device__ __forceinline__ T wave_sum_rows_shfl(T v)
{
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum_rows(T v)
{
#if MPCX_FAST_DPP_SUMS
    return wave_sum_rows_swap(v);
#else
    return wave_sum_rows_shfl(v);
#endif
}
// a sum over the wavefront whose bits need not be wave_sum's (another tree: within the rows as wave_max_dpp's maximum, across them towards lane 63, a row
// without a source takes in a 0), the same in every lane and the same from run to run.  Every lane active.
__device__ __forceinline__ double wave_sum_any(double v)
{
#if MPCX_FAST_DPP_SUMS
    v += dpp_mov_d<0xB1>(v);
    v += dpp_mov_d<0x4E>(v);
    v += dpp_mov_d<0x141>(v);
    v += dpp_mov_d<0x140>(v);
    v += dpp_mov_d<0x142>(v);
    v += dpp_mov_d<0x143>(v);
    return readlane_d(v, 63);
#else
    return wave_sum(v);
#endif
}
// the sums of fast_finish: the cost's bits are the result's
__device__ __forceinline__ double wave_sum_cost(double v)
{
#if MPCX_FAST_DPP_SUMS
    return wave_sum_full(v);
#else
    return wave_sum(v);
#endif
}

// One solve of the working-set system and the update of the primal point, working set of at most CAP (<= 16) rows.
// In: wsidx / wsb in LDS (unified indices and bound values of the na working rows), t0s = [t0 (128 CPZ) | G t0] in LDS.
// Out: lam[0..na) in LDS, wv / gw = w and G w in registers, lmax = largest |multiplier|; returns the position of a linearly
// dependent row, or -1.
// profiling aid (tools/phase_cycles.py): cycles per phase of a round, compiled in with -DMPCX_PROFILE_ROUNDS only
#ifdef MPCX_PROFILE_ROUNDS
#define MPCX_LAP(k) do { const long long now_ = (long long)__builtin_readcyclecounter(); pacc[k] += now_ - plast; plast = now_; } while (0)
#define MPCX_LAP_WAIT(k) do { __builtin_amdgcn_s_waitcnt(0); MPCX_LAP(k); } while (0)
#define MPCX_PROF_ARGS , long long (&pacc)[6], long long &plast
#define MPCX_PROF_PASS , pacc, plast
#else
#define MPCX_LAP(k) do {} while (0)
#define MPCX_LAP_WAIT(k) do {} while (0)
#define MPCX_PROF_ARGS
#define MPCX_PROF_PASS
#endif

// Round 12: e[i] += nm * (lane K's e[i], of this lane's row of sixteen lanes), i < N, each ONE instruction: gfx950's DP-ALU takes the DPP control
// row_newbcast:K on 64-bit VOP2, so the FMA reads lane K's entry itself -- no v_readlane pair, no SGPR, no broadcast value held in a register.  A single
// rounding, as fma(nm, p, e).  EVERY LANE HAS TO BE ACTIVE (a DPP source lane that is switched off delivers nothing).
// One asm statement for all N entries of an elimination step.  The hazard recogniser does not see into it, so the statement opens with its own wait
// states: a DPP read of a VGPR needs two after the VALU instruction that wrote it (s_nop 1) -- here nm, or an entry the step before wrote.  The five wait
// states between a VALU write of EXEC and a DPP instruction are not padded: no v_cmpx stands in the elimination, and every step's nm hangs on the pivot's
// reciprocal (a v_rcp_f64 and four FMAs behind the step's first instruction).  An entry is read (by DPP) and written by the same instruction only, so
// nothing inside the statement needs a wait.  N <= 14: an asm statement takes thirty operands, a read-write one counts twice.
#define MPCX_DPP_L(i) "v_fmac_f64_dpp %[e" #i "], %[e" #i "], %[nm] row_newbcast:%c[k] row_mask:0xf bank_mask:0xf\n\t"
#define MPCX_DPP_O(i) [e##i] "+v"(e[i])
#define MPCX_DPP_L1 MPCX_DPP_L(0)
#define MPCX_DPP_L2 MPCX_DPP_L1 MPCX_DPP_L(1)
#define MPCX_DPP_L3 MPCX_DPP_L2 MPCX_DPP_L(2)
#define MPCX_DPP_L4 MPCX_DPP_L3 MPCX_DPP_L(3)
#define MPCX_DPP_L5 MPCX_DPP_L4 MPCX_DPP_L(4)
#define MPCX_DPP_L6 MPCX_DPP_L5 MPCX_DPP_L(5)
#define MPCX_DPP_L7 MPCX_DPP_L6 MPCX_DPP_L(6)
#define MPCX_DPP_L8 MPCX_DPP_L7 MPCX_DPP_L(7)
#define MPCX_DPP_L9 MPCX_DPP_L8 MPCX_DPP_L(8)
#define MPCX_DPP_L10 MPCX_DPP_L9 MPCX_DPP_L(9)
#define MPCX_DPP_L11 MPCX_DPP_L10 MPCX_DPP_L(10)
#define MPCX_DPP_L12 MPCX_DPP_L11 MPCX_DPP_L(11)
#define MPCX_DPP_L13 MPCX_DPP_L12 MPCX_DPP_L(12)
#define MPCX_DPP_L14 MPCX_DPP_L13 MPCX_DPP_L(13)
#define MPCX_DPP_O1 MPCX_DPP_O(0)
#define MPCX_DPP_O2 MPCX_DPP_O1, MPCX_DPP_O(1)
#define MPCX_DPP_O3 MPCX_DPP_O2, MPCX_DPP_O(2)
#define MPCX_DPP_O4 MPCX_DPP_O3, MPCX_DPP_O(3)
#define MPCX_DPP_O5 MPCX_DPP_O4, MPCX_DPP_O(4)
#define MPCX_DPP_O6 MPCX_DPP_O5, MPCX_DPP_O(5)
#define MPCX_DPP_O7 MPCX_DPP_O6, MPCX_DPP_O(6)
#define MPCX_DPP_O8 MPCX_DPP_O7, MPCX_DPP_O(7)
#define MPCX_DPP_O9 MPCX_DPP_O8, MPCX_DPP_O(8)
#define MPCX_DPP_O10 MPCX_DPP_O9, MPCX_DPP_O(9)
#define MPCX_DPP_O11 MPCX_DPP_O10, MPCX_DPP_O(10)
#define MPCX_DPP_O12 MPCX_DPP_O11, MPCX_DPP_O(11)
#define MPCX_DPP_O13 MPCX_DPP_O12, MPCX_DPP_O(12)
#define MPCX_DPP_O14 MPCX_DPP_O13, MPCX_DPP_O(13)
#define MPCX_DPP_CASE(n) if constexpr (N == n) asm volatile("s_nop 1\n\t" MPCX_DPP_L##n : MPCX_DPP_O##n : [nm] "v"(nm), [k] "i"(K))
constexpr int kDppBlock = 14;
template <int K, int N>
__device__ __forceinline__ void fmac_row_bcast(double (&e)[N], const double nm)
{
    static_assert(K >= 0 && K < 16 && N >= 1 && N <= kDppBlock, "a row of sixteen lanes, at most fourteen read-write operands");
    MPCX_DPP_CASE(1); MPCX_DPP_CASE(2); MPCX_DPP_CASE(3); MPCX_DPP_CASE(4); MPCX_DPP_CASE(5); MPCX_DPP_CASE(6); MPCX_DPP_CASE(7);
    MPCX_DPP_CASE(8); MPCX_DPP_CASE(9); MPCX_DPP_CASE(10); MPCX_DPP_CASE(11); MPCX_DPP_CASE(12); MPCX_DPP_CASE(13); MPCX_DPP_CASE(14);
}
template <int K>
__device__ __forceinline__ double fmac_row_bcast(double acc, const double nm)
{
    double e[1] = {acc};
    fmac_row_bcast<K, 1>(e, nm);
    return e[0];
}

template <int CAP, int NLO, int CPZ, int CPG, bool DP = false, bool XL = false>
__device__ __forceinline__ int ws_solve_reg(const gdp gY, const int ldy, const int ldz, const int na, const int lane_in,
                                            const int *wsidx, const double *wsb, const double *t0s, double *lam,
                                            const unsigned (&offz)[CPZ], const unsigned (&offg)[CPG],
                                            double (&wv)[2 * CPZ], double (&gw)[2 * CPG], double &lmax MPCX_PROF_ARGS)
{
    // offz / offg: this lane's element pairs within a row of Y, in bytes -- with the row's scalar base an addressing mode of the load, no vector address arithmetic
    // NLO <= na <= CAP: the size class (the caller's dispatch), so only the columns from NLO on can lie past the working set
    // rows of Y requested ahead of the elimination (none for the largest working sets: their elimination needs the registers, and a
    // spilled register is HBM traffic -- scratch is memory)
    // (round 9: the six-row class, where the mean working set falls, takes ALL its rows ahead -- no trip after the elimination; the same for the eight-row
    // class spills 104 B per lane, six rows ahead in the 8- to 12-row classes 60 B, so from there on four rows go ahead and the rest is pipelined below.
    // DEEP: see the macros above)
    constexpr bool DEEP = CPZ + CPG <= MPCX_FAST_DEEP_CHUNKS;
    constexpr int PF = CAP > MPCX_FAST_PF_MAXCAP ? 0 : (CAP <= (DEEP ? MPCX_FAST_PF_ALL : MPCX_FAST_PF) ? CAP : MPCX_FAST_PF);
    // the lane number as this round's own value: what depends on it (the masks lane == k of the elimination, the identity's entries) is then formed
    // where it is used, one compare each, instead of ahead of the round loop for every size class at once -- more than the register files hold
    int lane = lane_in;
    asm volatile("" : "+v"(lane));
    const bool real = lane < na;
    const int li = real ? lane : 0;
    const int qi = wsidx[li];
    int qc[CAP];                                    // wave-uniform: SGPRs
#pragma unroll
    for (int c = 0; c < CAP; ++c) qc[c] = __builtin_amdgcn_readfirstlane(wsidx[(c < NLO || c < na) ? c : 0]);
    double Sr[CAP];
    // one 64-bit base and a 32-bit element offset per entry (sixteen 64-bit scalar row bases were more than the SGPR file holds next to
    // the pivot row: they were spilled to VGPR lanes and read back, two vector instructions per entry)
    const unsigned rowoff = (unsigned)(qi * ldy) * 8u;       // in bytes: base + 32-bit offset is an addressing mode of the load
    const char MPCX_GAS *const gYb = reinterpret_cast<const char MPCX_GAS *>(gY);
    auto y_at = [&](unsigned off) { return *reinterpret_cast<gdp>(gYb + off); };
    auto row_ld2 = [&](int q, unsigned off) { return *reinterpret_cast<const d2 MPCX_GAS *>(gYb + (unsigned)(q * ldy) * 8u + off); };     // the pair at `off` of row q
#pragma unroll
    for (int c = 0; c < CAP; ++c) Sr[c] = y_at(rowoff + (unsigned)qc[c] * 8u);
    const double dg = y_at(rowoff + (unsigned)qi * 8u);    // this lane's own diagonal, for its pivot threshold: the same element as Sr[lane]
    d2 pz[PF > 0 ? PF : 1][CPZ], pg[PF > 0 ? PF : 1][CPG];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
#pragma unroll
        for (int c = 0; c < CPZ; ++c) pz[u][c] = row_ld2(qc[u], offz[c]);
#pragma unroll
        for (int c = 0; c < CPG; ++c) pg[u][c] = row_ld2(qc[u], offg[c]);
    }
    double y = real ? t0s[qi < ldz ? qi : qi - ldz + 128 * CPZ] - wsb[li] : 0.0;       // [t0 | G t0] by unified index (padded arrays)
    MPCX_LAP_WAIT(1);                              // 1: working set to registers + every load of the round answered
    // rows and columns past na: the identity (the elimination below is straight-line code over all CAP steps).  The lanes past na take their
    // whole rows under one execution mask; a column past na (wave-uniform, from NLO on only) is zero on the real lanes, which lie before it
    if (!real) {
#pragma unroll
        for (int c = 0; c < CAP; ++c) Sr[c] = 0.0;
    }
#pragma unroll
    for (int c = NLO; c < CAP; ++c) if (c >= na) Sr[c] = lane == c ? 1.0 : 0.0;
    const double pthr = 1e-11 * (real ? dg : 1.0);  // this lane's pivot threshold (relative to its original diagonal; the identity's is 1)
    double mydinv = 1.0;
    unsigned long long dep = 0ull;
    // Gauss-Jordan on [S | y], lane i = row i; a failed pivot test is recorded and looked at once, after the loop
    // (the step number is a template argument: the DPP form's source lane is an immediate of the instruction)
    auto gj_step = [&]<int K>() {
        dep |= __ballot(!(Sr[K] > pthr)) & (1ull << K);       // lane K's verdict on its pivot
        // the pivot itself is a scalar read in both forms: its reciprocal chain runs on a wave-uniform value
        const double rinv = pivot_rcp(readlane_d(Sr[K], K));
        if constexpr (DP) {
            // Round 12: the pivot row and the right-hand side by DPP row broadcast inside the FMA (fmac_row_bcast above), one instruction per entry where the
            // scalar form has two v_readlane_b32 and the FMA.  A DPP source lane has to be active, so there is NO execution mask around the FMAs -- every lane
            // is active here: ws_solve_reg is called from wave-uniform code, and the region `if (!real)` above closes before the elimination; keep it so --
            // and lane K, the source, takes the multiplier +0 instead of being masked off.  Why the bits are those of the scalar form:
            //   * lanes 0..15 are one DPP row and receive lane K's value, which is what v_readlane delivered, and -m is an exact negation: the operands of
            //     every FMA on the real lanes and on the identity padding below lane 16 are the old ones, and fma(-m, p, S) is S += (-m) p in one rounding;
            //   * lane K computes S + (+0) S, which is S for every finite S, both signed zeros included (the product has S's sign; x + (+-0) = x, and
            //     (+-0) + (+-0) of equal signs keeps the sign) -- tests/test_lmpc_round_dpp_probe_gpu.py holds the sign cases;
            //   * lanes 16..63 hold zero rows and receive lane 16 r + K's zeros instead of lane K's values.  Their own m is 0 x rinv either way, so their rows
            //     stay zero (or turn NaN where a pivot is not a positive finite number, as the padding in lanes 16..31 did: the dep test ends that solve).
            //     Nothing reads them: lam[] is written by the lanes below CAP, the ballot keeps bit K < 16, and the update takes no lane's y;
            //   * a non-finite entry in the pivot row turns lane K's row into NaN where it stayed +-inf.  Such an instance reaches the NaN screen in both
            //     forms and goes to the fallback (tests/test_lmpc_round_dpp_gpu.py, test_bad_neighbour_in_the_workgroup).
            if (lane == K) mydinv = rinv;
            const double nm = lane == K ? 0.0 : -(Sr[K] * rinv);
            constexpr int NE = CAP - K;              // the step's entries: columns K + 1 .. CAP - 1, then y
            auto block = [&]<int J0, int N>() {
                double e[N];
#pragma unroll
                for (int u = 0; u < N; ++u) e[u] = J0 + u < CAP ? Sr[J0 + u < CAP ? J0 + u : 0] : y;
                fmac_row_bcast<K, N>(e, nm);
#pragma unroll
                for (int u = 0; u < N; ++u) {
                    if (J0 + u < CAP) Sr[J0 + u < CAP ? J0 + u : 0] = e[u];
                    else y = e[u];
                }
            };
            if constexpr (NE <= kDppBlock) block.template operator()<K + 1, NE>();
            else {
                static_assert(NE <= 2 * kDppBlock, "two statements hold a step of the largest class");
                block.template operator()<K + 1, kDppBlock>();
                block.template operator()<K + 1 + kDppBlock, NE - kDppBlock>();
            }
        } else {
            double pj[CAP];
#pragma unroll
            for (int j = K + 1; j < CAP; ++j) pj[j] = readlane_d(Sr[j], K);
            const double py = readlane_d(y, K);
            if (lane == K) mydinv = rinv;
            else {
                const double m = Sr[K] * rinv;
#pragma unroll
                for (int j = K + 1; j < CAP; ++j) Sr[j] = fma(-m, pj[j], Sr[j]);
                y = fma(-m, py, y);
            }
        }
    };
    [&]<int... Ks>(std::integer_sequence<int, Ks...>) { (gj_step.template operator()<Ks>(), ...); }(std::make_integer_sequence<int, CAP>{});
    MPCX_LAP(2);                                   // 2: elimination
    if (dep != 0ull) return (int)__builtin_ctzll(dep);
    y *= mydinv;                                   // lanes >= na: 0
    // XL: the update reads the multipliers back from here, a pair per read, so the positions from na up to CAP hold their lanes' exact +0 too (the verify
    // phase looks up positions below na or the spare slot, as before)
    if (XL ? lane < CAP : real) lam[lane] = y;
    // wave-uniform addresses, two multipliers per 16-byte read.  The reads travel with the rows of Y they multiply: the first PF rows' here, next to t0, a later
    // batch's with the batch's loads (all CAP of them at once, live beside three batches of rows, spill: profiles/r10_resource_usage_lmpc.txt)
    auto lam_pair = [&](const int a, double (&l2)[2]) {
        const double2 v = *reinterpret_cast<const double2 *>(lam + a);
        l2[0] = v.x; l2[1] = v.y;
    };
    constexpr int NLP = XL && PF > 0 ? PF / 2 : 1;
    double lamp[NLP][2];
    if constexpr (XL) {
        static_assert(CAP % 2 == 0 && PF % 2 == 0 && kFastCap % 2 == 0, "multipliers are read back in pairs");
        wave_sync();                               // the multipliers are written by other lanes
#pragma unroll
        for (int p = 0; p < PF / 2; ++p) lam_pair(2 * p, lamp[p]);
    }
    // w = t0 - Y[:, A] lambda
#pragma unroll
    for (int c = 0; c < CPZ; ++c) {
        const double2 v = *reinterpret_cast<const double2 *>(t0s + 128 * c + 2 * lane);
        wv[2 * c] = v.x; wv[2 * c + 1] = v.y;
    }
#pragma unroll
    for (int c = 0; c < CPG; ++c) {
        const double2 v = *reinterpret_cast<const double2 *>(t0s + 128 * CPZ + 128 * c + 2 * lane);
        gw[2 * c] = v.x; gw[2 * c + 1] = v.y;
    }
    double lm = 0.0;
    // one row of Y applied: rows in ascending working-set position, whichever batch brought them (a row past na is a copy of row 0 with multiplier 0)
    // (lds: the multiplier as read back from lam[a].  The update runs on all 64 lanes, so a 32-lane crossbar broadcast does not serve here)
    auto apply_row = [&](const int a, const double lds, const d2 (&rz)[CPZ], const d2 (&rg)[CPG]) {
        const double la = XL ? lds : readlane_d(y, a);
        lm = fmax(lm, fabs(la));
#pragma unroll
        for (int c = 0; c < CPZ; ++c) { wv[2 * c] = fma(-la, rz[c].x, wv[2 * c]); wv[2 * c + 1] = fma(-la, rz[c].y, wv[2 * c + 1]); }
#pragma unroll
        for (int c = 0; c < CPG; ++c) { gw[2 * c] = fma(-la, rg[c].x, gw[2 * c]); gw[2 * c + 1] = fma(-la, rg[c].y, gw[2 * c + 1]); }
    };
    if constexpr (CAP == PF) {
#pragma unroll
        for (int a = 0; a < PF; ++a) apply_row(a, lamp[XL ? a / 2 : 0][a % 2], pz[a], pg[a]);
    } else {
        // round 9: the rows behind the first PF in batches of RB, software-pipelined over NBUF buffers -- the first NBUF batches are requested together,
        // batch k + NBUF as soon as batch k's FMAs are issued (its registers are free then), i.e. always ahead of the wait for batch k + 1.  The requests
        // follow the FMAs of the rows that came ahead of the elimination, whose registers they take over (requested before them, the two sets are live
        // together and the kernels spill).  Every batch starts before the class's smallest working set ends (a0 < NLO: the size classes are two rows
        // wide), so nothing here is under a branch.  Rows are still applied in ascending working-set position.
        constexpr int RB0 = DEEP ? MPCX_FAST_RB_DEEP : MPCX_FAST_RB, RB = CAP - PF < RB0 ? CAP - PF : RB0;      // rows of Y per later batch
        constexpr int NB = (CAP - PF + RB - 1) / RB, NBUF = DEEP ? MPCX_FAST_NBUF : 1;
        static_assert(PF + (NB - 1) * RB < NLO, "a later batch would start past the class's smallest working set");
        // the later rows' indices come from LDS once more: sixteen of them do not stay in SGPRs through the elimination beside its pivot row, and they
        // were spilled to VGPR lanes.  (An offset the compiler cannot see through makes these loads of their own, not the first ones' registers kept.)
        int again = 0;
        asm volatile("" : "+s"(again));
        const int *wsidx_again = wsidx + again;
        static_assert(!XL || RB % 2 == 0, "multipliers are read back in pairs");
        d2 mz[NBUF][RB][CPZ], mgv[NBUF][RB][CPG];
        double ml[NBUF][XL ? RB / 2 : 1][2];
        auto request = [&](const int k, d2 (&bz)[RB][CPZ], d2 (&bg)[RB][CPG], double (&bl)[XL ? RB / 2 : 1][2]) {
            if constexpr (XL) {
#pragma unroll
                for (int u = 0; u < RB; u += 2)
                    if (PF + k * RB + u < CAP) lam_pair(PF + k * RB + u, bl[u / 2]);
            }
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int cu = PF + k * RB + u < CAP ? PF + k * RB + u : 0;
                const int q = __builtin_amdgcn_readfirstlane(wsidx_again[(cu < NLO || cu < na) ? cu : 0]);
#pragma unroll
                for (int c = 0; c < CPZ; ++c) bz[u][c] = row_ld2(q, offz[c]);
#pragma unroll
                for (int c = 0; c < CPG; ++c) bg[u][c] = row_ld2(q, offg[c]);
            }
        };
#pragma unroll
        for (int a = 0; a < PF; ++a) apply_row(a, lamp[XL ? a / 2 : 0][a % 2], pz[a], pg[a]);
#pragma unroll
        for (int k = 0; k < NBUF && k < NB; ++k) request(k, mz[k], mgv[k], ml[k]);
        MPCX_FAST_STAGE();
#pragma unroll
        for (int k = 0; k < NB; ++k) {
#pragma unroll
            for (int u = 0; u < RB; ++u)
                if (PF + k * RB + u < CAP) apply_row(PF + k * RB + u, ml[k % NBUF][XL ? u / 2 : 0][u % 2], mz[k % NBUF][u], mgv[k % NBUF][u]);
            if (k + NBUF < NB) { request(k + NBUF, mz[k % NBUF], mgv[k % NBUF], ml[k % NBUF]); MPCX_FAST_STAGE(); }
        }
    }
    lmax = lm;
    return -1;
}

// the pads of a slice (written once per wavefront: nothing ever overwrites them except the solution w, whose pads are 0 too)
template <int CPZ, int CPG>
__device__ __forceinline__ void fast_init_pads(double *slice, const int ldz, const int ldg, const int lane)
{
    constexpr int ZP = 128 * CPZ, GPD = 128 * CPG;
    const double INF = __builtin_huge_val();
    double *t0s = slice, *gt0s = t0s + ZP, *lgs = gt0s + GPD, *ugs = lgs + GPD, *fs = ugs + GPD, *lam = fs + ZP + 2;
#pragma unroll
    for (int c = 0; c < CPZ; ++c) {
        const int e = 128 * c + 2 * lane;
        if (e >= ldz) { *reinterpret_cast<double2 *>(t0s + e) = make_double2(0.0, 0.0); *reinterpret_cast<double2 *>(fs + e) = make_double2(0.0, 0.0); }
    }
#pragma unroll
    for (int c = 0; c < CPG; ++c) {
        const int r = 128 * c + 2 * lane;
        if (r >= ldg) {
            *reinterpret_cast<double2 *>(gt0s + r) = make_double2(0.0, 0.0);
            *reinterpret_cast<double2 *>(lgs + r) = make_double2(-INF, -INF);
            *reinterpret_cast<double2 *>(ugs + r) = make_double2(INF, INF);
        }
    }
    if (lane == 0) { lam[kFastCap] = 0.0; lam[kFastCap + 1] = 0.0; }      // where the rows outside the working set look their multiplier up
}

// this wavefront's LDS slice (doubles), ZP = 128 CPZ, GPD = 128 CPG -- every array padded to whole lane pairs so that no lane needs a
// range predicate: t0 pads 0, bounds pad -inf / +inf (a padded row is never violated, never active):
//   t0 [ZP] | gt0 [GPD] | lg [GPD] | ug [GPD] | f, later w [ZP] | c0, flag | lam [kFastCap + 2] | wsb [kFastCap + 2] | wsidx (ints) | scratch
// lwuw: the workgroup's copy of the box bounds [lw (ZP) | uw (ZP)], padded the same way
template <int CPZ, int CPG> constexpr int fast_slice_fixed() { return 2 * 128 * CPZ + 3 * 128 * CPG + 2 + 2 * (kFastCap + 2) + (kFastCap + 2) / 2 + 1; }

// =====================================================================================
// the record of one instance without the workspace: ProblemBuilder::get as ONE mat-vec
// =====================================================================================
// Everything the solve needs of an instance -- f, t0 = -Hinv f, G t0, the row offsets, the feasibility rows and the cost
// constant -- is MF * vin with vin = [x0 | lastU | yref | 1] (lmpc_model.cpp: compose_fused_maps).  The wavefront computes it
// into its own LDS slice, in the layout of the workspace record (f | t0 | gt0 | lg | ug | c0, flag), and solve_fast reads it
// from there: no assemble kernel, no 2.7 KB per instance written to HBM and read back.  MF streams from L2 (87 KB at N = 20).
constexpr int kCpFused = 3;            // rows of MF per lane pair: up to 384
// where the pieces of the record go (the lean kernels keep them in padded LDS arrays)
struct RecPtrs { double *f, *t0, *gt0, *lg, *ug, *tail; };
// (__forceinline__: as a real call the lean kernels' fused form faulted on its by-reference arguments)
__device__ __forceinline__ void fused_record(const LmpcDev &M, const LmpcBatchDev &Bt, const int b, const int lane, double *stage,
                                             const RecPtrs &rp, const double *mf_lds)
{
    const int nx = M.nx, nu = M.nu, ny = M.ny, kin = M.kin;
    const int ldz = M.ldz, ldg = M.ldg, ldy = M.ldy, rowsF = M.rowsF;
    const int variant = Bt.fused - 1;
    // vin: the same k -> (x0 | lastU | yref | 1) map as lmpc_assemble_mfma (kin may exceed the 64 lanes: nx + nu + ny past 60)
    for (int k = lane; k < kin; k += 64) {
        double v = 0.0;
        if (k < M.nxp) { if (k < nx) v = gl(Bt.x0)[(size_t)b * nx + k]; }
        else if (k < M.nxp + M.nup) { const int c = k - M.nxp; if (c < nu) v = gl(Bt.u0)[(size_t)b * nu + c]; }
        else if (k < M.ione) { const int c = k - M.nxp - M.nup; if (variant && c < ny) v = gl(Bt.yref)[(size_t)b * Bt.yref_bs + c]; }
        else if (k == M.ione) v = 1.0;
        stage[k] = v;
    }
    wave_sync();
    double acc[2 * kCpFused];
#pragma unroll
    for (int s = 0; s < 2 * kCpFused; ++s) acc[s] = 0.0;
    if (mf_lds) {
        // the composed map sits in this workgroup's LDS (lmpc_solve_persistent loaded it once): sixteen-byte reads, lanes on
        // consecutive rows (no bank conflicts), four columns in flight
        int off[kCpFused];
#pragma unroll
        for (int c = 0; c < kCpFused; ++c) { const int e = 128 * c + 2 * lane; off[c] = e < rowsF ? e : 0; }
        for (int j = 0; j < kin; j += 4) {
            double2 m[4][kCpFused];
            double xj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double *col = mf_lds + (size_t)(j + u) * rowsF;
#pragma unroll
                for (int c = 0; c < kCpFused; ++c) m[u][c] = *reinterpret_cast<const double2 *>(col + off[c]);
                xj[u] = stage[j + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int c = 0; c < kCpFused; ++c) {
                    acc[2 * c] = fma(m[u][c].x, xj[u], acc[2 * c]);
                    acc[2 * c + 1] = fma(m[u][c].y, xj[u], acc[2 * c + 1]);
                }
            }
        }
    } else {
        // from L2, two columns per batch: the stream is bandwidth-bound there -- every wavefront of the launch reads the same
        // 87 KB -- and deeper batches only made the burst worse (146 us against 122 us for the launch at the benchmark batch)
        matvec_acc<kCpFused>(gl(variant ? M.MF1 : M.MF0), rowsF, rowsF, kin, stage, acc, lane);
    }
    const int r_goff = ldy, r_f = r_goff + ldg, r_s = r_f + ldz, r_q = r_s + M.nsp;
    double c0p = 0.0;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < kCpFused; ++c) {
        const int e = 128 * c + 2 * lane;          // block boundaries are even: a pair never straddles two blocks
        if (e >= rowsF) continue;
        const double a0 = acc[2 * c], a1 = acc[2 * c + 1];
        if (e < ldz) {                             // t0
            *reinterpret_cast<double2 *>(rp.t0 + e) = make_double2(a0, a1);
        } else if (e < r_goff) {                   // gt0
            *reinterpret_cast<double2 *>(rp.gt0 + (e - ldz)) = make_double2(a0, a1);
        } else if (e < r_f) {                      // row offsets -> bounds of this instance
            const int r = e - r_goff;
            const d2 l0 = ld2(GP(lg0) + r), u0 = ld2(GP(ug0) + r);
            *reinterpret_cast<double2 *>(rp.lg + r) = make_double2(l0.x - a0, l0.y - a1);
            *reinterpret_cast<double2 *>(rp.ug + r) = make_double2(u0.x - a0, u0.y - a1);
        } else if (e < r_s) {                      // linear term
            *reinterpret_cast<double2 *>(rp.f + (e - r_f)) = make_double2(a0, a1);
        } else if (e < r_q) {                      // rows that do not see the inputs: pure feasibility conditions on (x0, lastU)
            const int r = e - r_s;
            if (r < M.ns) bad |= violates(a0, GP(slo)[r], GP(shi)[r], M.eps_abs, M.eps_rel);
            if (r + 1 < M.ns) bad |= violates(a1, GP(slo)[r + 1], GP(shi)[r + 1], M.eps_abs, M.eps_rel);
        } else {                                   // cost constant: vin' Qc vin / 2
            const int k = e - r_q;
            c0p = fma(0.5 * stage[k], a0, c0p);
            c0p = fma(0.5 * stage[k + 1], a1, c0p);
        }
    }
    c0p = wave_sum(c0p);
    const bool anybad = wave_any(bad);
    if (lane == 0) *reinterpret_cast<double2 *>(rp.tail) = make_double2(c0p, anybad ? 1.0 : 0.0);
    wave_sync();
}

// lmpc_solve_group's kernel arguments as they lie in the kernel-argument segment.  The kernel reads them through the segment pointer, not through
// its by-value parameters: a by-value struct has every field loaded at the kernel's entry and kept in SGPRs until its last use, and what the unpack
// behind the round loop reads was spilled to VGPR lanes across the loop -- writelane / readlane pairs on the issue slots the rounds are bound by.
struct GroupArgs { LmpcDev M; LmpcBatchDev Bt; double *wsbase; int variant; };
typedef const GroupArgs __attribute__((address_space(4))) *group_args_p;
static_assert(offsetof(GroupArgs, Bt) == sizeof(LmpcDev) && offsetof(GroupArgs, wsbase) == sizeof(LmpcDev) + sizeof(LmpcBatchDev), "GroupArgs mirrors lmpc_solve_group's parameter list");

// What follows the rounds of solve_fast: the instance goes to the fallback kernel, or its solution is unpacked and written out
// (LOptimizer.hpp:305-347).  A function of its own so that lmpc_solve_group can hand it the kernel arguments re-read behind the round loop.
template <int CPZ, int CPG, int SRC>
__device__ __forceinline__ void fast_finish(const LmpcDev &M, const LmpcBatchDev &Bt, const int b, const int lane, double *slice, const double *lwuw, gdw ws, double *outs,
                                            const bool infeasible, const bool solved, const bool fixed_violation,
                                            const double (&wv)[2 * CPZ], const int (&actb)[2 * CPZ], const int (&actg)[2 * CPG], const int (&posb)[2 * CPZ],
                                            const int (&posg)[2 * CPG], const double dtol_last, const int na_last, const int rounds_total,
                                            const long long ts0, const long long ts1, const long long ts2 MPCX_PROF_ARGS)
{
    constexpr int NZS = 2 * CPZ, NGS = 2 * CPG, ZP = 128 * CPZ, GPD = 128 * CPG;
    constexpr bool FUSED = SRC != 0;
    const int nu = M.nu, nz = M.nz, mg = M.mg, ldz = M.ldz, ldg = M.ldg, ldy = M.ldy;
    double *t0s = slice, *gt0s = t0s + ZP, *lgs = gt0s + GPD, *ugs = lgs + GPD, *fs = ugs + GPD, *tail = fs + ZP;
    double *lam = tail + 2, *wsb = lam + (kFastCap + 2);
    double *scratch = wsb + (kFastCap + 2) + (kFastCap + 2) / 2 + 1;
    const double *lws = lwuw, *uws = lwuw + ZP;
    const double c0 = tail[0], flag0 = tail[1];     // (read again rather than carried through the rounds in registers)
    long long ts3 = 0;
    auto stamp = [&](long long &t) { if (Bt.dbg_cycles) t = (long long)__builtin_readcyclecounter(); };

    if (!infeasible && !solved) {
        // left for the fallback kernel (flag stays 0 / 1), which reads the workspace record
        if constexpr (FUSED) {
#pragma unroll
            for (int c = 0; c < CPZ; ++c) {
                const int e = 128 * c + 2 * lane;
                if (e < ldz) {
                    const double2 vf = *reinterpret_cast<const double2 *>(fs + e), vt = *reinterpret_cast<const double2 *>(t0s + e);
                    st2(ws + e, vf.x, vf.y); st2(ws + ldz + e, vt.x, vt.y);
                }
            }
#pragma unroll
            for (int c = 0; c < CPG; ++c) {
                const int r = 128 * c + 2 * lane;
                if (r < ldg) {
                    const double2 vt = *reinterpret_cast<const double2 *>(gt0s + r), vl = *reinterpret_cast<const double2 *>(lgs + r),
                                  vu = *reinterpret_cast<const double2 *>(ugs + r);
                    st2(ws + ldz + ldz + r, vt.x, vt.y);
                    st2(ws + ldz + ldy + r, vl.x, vl.y);
                    st2(ws + ldz + ldy + ldg + r, vu.x, vu.y);
                }
            }
            if (lane == 0) st2(ws + ldz + ldy + 2 * ldg, c0, flag0);
        }
        if (outs && lane == 0) outs[7] = 0.0;
        if constexpr (SRC != 2) { if (Bt.fq && lane == 0) fallback_append(Bt.fq, Bt.fq_cap, b); }      // (lmpc_solve_group files its workgroup's failures together)
        return;
    }
    const int solver_status = infeasible ? -3 : (fixed_violation ? -2 : 1);

    // ---- unpack (LOptimizer.hpp:305-347)
    double w[NZS], f[NZS];
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < CPZ; ++c) {
        const double2 vf = *reinterpret_cast<const double2 *>(fs + 128 * c + 2 * lane);
        f[2 * c] = vf.x; f[2 * c + 1] = vf.y;
    }
#pragma unroll
    for (int s = 0; s < NZS; ++s) w[s] = infeasible ? qnan : ((128 * (s >> 1) + 2 * lane + (s & 1) < nz) ? wv[s] : 0.0);
    double *stage = fs;                              // the solution replaces the linear term
    double cost;
    bool cost_pending = false;
    wave_sync();
#pragma unroll
    for (int c = 0; c < CPZ; ++c) *reinterpret_cast<double2 *>(stage + 128 * c + 2 * lane) = make_double2(w[2 * c], w[2 * c + 1]);
    wave_sync();
    // this lane's share of the soft rows' penalty at the verified point: the slack of a working row is lambda / rho.  Only the
    // branches that take the cost from its definition add it; the multiplier identity below holds with the penalty in it
    auto soft_penalty = [&]() {
        double pen = 0.0;
#pragma unroll
        for (int s = 0; s < NGS; ++s) {
            const int r = 128 * (s >> 1) + 2 * lane + (s & 1);
            if (r < mg && actg[s] != 0) { const double l = lam[posg[s]]; pen = fma(0.5 * gl(MPCX_G_SOFT(M))[r] * l, l, pen); }
        }
        return pen;
    };
    if (infeasible) {
        cost = 1e30;
    } else if (!M.cost_direct) {
        // cost from the multipliers: at the verified point H w + f + N_A' lambda = 0 and N_A w = b_A, hence w'Hw/2 + f'w = (f'w - lambda'b_A)/2 -- no
        // pass over H (the single largest read of an instance), and the products involve the bounded solution w, not the possibly huge unconstrained optimum
        double j = 0;
#pragma unroll
        for (int s = 0; s < NZS; ++s) j = fma(f[s], w[s], j);
        if (lane < na_last) j = fma(-lam[lane], wsb[lane], j);
        cost = 0.5 * wave_sum_cost(j) + c0;
    } else if (!FUSED && Bt.n_models <= 0) {
        // cost from its definition by lmpc_cost_mfma: the solution goes to the workspace in t0's place
#pragma unroll
        for (int c = 0; c < CPZ; ++c) {
            const int e = 128 * c + 2 * lane;
            if (e < ldz) st2(ws + ldz + e, w[2 * c], w[2 * c + 1]);
        }
        if (M.n_soft > 0) {                         // lmpc_cost_mfma adds the record's constant: the penalty rides in it
            const double pen = wave_sum_cost(soft_penalty());
            if (lane == 0) ws[ldz + ldy + 2 * ldg] = c0 + pen;
        }
        cost = 0.0;
        cost_pending = true;
    } else if (SRC == 2 && CPZ == 2 && Bt.n_models <= 0) {
        // lmpc_solve_group<2, 2>: the workgroup takes these costs from their definition together, behind its solves, by lmpc_cost_mfma's own
        // arithmetic (group_cost_mfma) -- the two-kernel form's bits.  Here only what that kernel reads from the record: the constant, with the penalty in it
        cost = M.n_soft > 0 ? c0 + wave_sum_cost(soft_penalty()) : c0;
        cost_pending = true;
    } else {
        double hw[NZS];
#pragma unroll
        for (int s = 0; s < NZS; ++s) hw[s] = 0;
        matvec_acc<CPZ>(GP(H), ldz, ldz, nz, stage, hw, lane);
        double j = 0;
#pragma unroll
        for (int s = 0; s < NZS; ++s) j += w[s] * (0.5 * hw[s] + f[s]);
        if constexpr (SRC != 1) { if (M.n_soft > 0) j += soft_penalty(); }      // (the fused mat-vec form is never taken with cost_direct: fused_ok)
        cost = wave_sum_cost(j) + c0;
    }
#pragma unroll
    for (int s = 0; s < NZS; ++s) {
        const int e = 128 * (s >> 1) + 2 * lane + (s & 1);
        if (e < nu) { if (outs) outs[8 + e] = w[s]; else glw(Bt.cmd)[(size_t)b * nu + e] = w[s]; }
    }
    if (outs) {
        if (lane == 0) {
            outs[0] = cost; outs[1] = ref_status(solver_status); outs[2] = solver_status;
            outs[3] = ref_feasible(solver_status); outs[4] = cost_pending ? 1.0 : 0.0; outs[5] = rounds_total; outs[6] = infeasible ? 0 : na_last; outs[7] = 2.0;
        }
    } else if (lane == 0) {
        store_scalars(Bt, b, !cost_pending, cost, solver_status, 0, rounds_total, infeasible ? 0 : na_last);
    }

    if (Bt.active_lower && Bt.active_upper) {
        // a working row is active where its multiplier is not zero; t0's place in LDS is free for the words
        const ActiveBits bits(M, t0s, lane);
        if (!infeasible) {
#pragma unroll
            for (int s = 0; s < NZS; ++s) {
                const int e = 128 * (s >> 1) + 2 * lane + (s & 1);
                if (e >= nz || actb[s] == 0) continue;
                const double l = lam[posb[s]];
                if (!(fabs(l) > dtol_last)) continue;
                bits.mark_box(e, l < 0 ? -1 : 1, lws[e], uws[e]);
            }
#pragma unroll
            for (int s = 0; s < NGS; ++s) {
                const int r = 128 * (s >> 1) + 2 * lane + (s & 1);
                if (r >= mg || actg[s] == 0) continue;
                const double l = lam[posg[s]];
                if (!(fabs(l) > dtol_last)) continue;
                bits.mark_row(r, l < 0 ? -1 : 1);
            }
        }
        bits.store(Bt, b, lane);
    }

    sequence_rollout(M, Bt, b, lane, stage, scratch, infeasible);
    wave_sync();
    if (lane == 0 && !outs) ws[ldz + ldy + 2 * ldg + 1] = cost_pending ? 3.0 : 2.0;     // 2: done, the fallback kernel skips it; 3: lmpc_cost_mfma first
    stamp(ts3);   // 3: unpacked
    if (Bt.dbg_cycles && lane == 0)
    {
        long long *o = Bt.dbg_cycles + (size_t)b * 8;
#ifdef MPCX_PROFILE_ROUNDS
        o[0] = ts1 - ts0; o[1] = ts2 - ts1;                    // load, solve, six phases
        for (int k = 0; k < 6; ++k) o[2 + k] = pacc[k];
#else
        o[0] = ts0; o[1] = ts1; o[2] = ts2; o[3] = ts3;        // (slots 4..6: lmpc_solve_group's own stamps)
#endif
    }
}

// SRC: where the instance's record comes from -- 0 the workspace (two-kernel path), 1 computed here by fused_record (one mat-vec
// with the composed maps), 2 already in the slice (lmpc_solve_group: the workgroup's MFMA assemble phase put it there)
template <int CPZ, int CPG, int SRC = 0>
__device__ __forceinline__ void solve_fast(const LmpcDev &M, const LmpcBatchDev &Bt, const int b, const int lane,
                           double *slice, const double *lwuw, gdw ws, const double *mf_lds = nullptr, double *outs = nullptr, const int eqbits = 0)
{
    // eqbits (SRC = 2, lmpc_solve_group): bit s = this lane's general row s is an equality (lg0 == ug0), looked up by the caller with its other loads
    // outs (lmpc_solve_group): the instance's scalar results and its command go to this LDS record [cost, status, solver status,
    // feasible, iterations, rounds, active rows, done | cmd (nu)] instead of to HBM; the workgroup writes sixteen of them coalesced
    constexpr int NZS = 2 * CPZ, NGS = 2 * CPG, ZP = 128 * CPZ, GPD = 128 * CPG;
    const int nz = M.nz, mg = M.mg, ldz = M.ldz, ldg = M.ldg, ldy = M.ldy;
    const gdp gY = GP(Y);
    double *t0s = slice, *gt0s = t0s + ZP, *lgs = gt0s + GPD, *ugs = lgs + GPD, *fs = ugs + GPD, *tail = fs + ZP;
    double *lam = tail + 2, *wsb = lam + (kFastCap + 2);
    int *wsidx = reinterpret_cast<int *>(wsb + (kFastCap + 2));
    double *scratch = wsb + (kFastCap + 2) + (kFastCap + 2) / 2 + 1;
    const double *lws = lwuw, *uws = lwuw + ZP;
    const double INF = __builtin_huge_val();

    long long ts0 = 0, ts1 = 0, ts2 = 0;                   // profiling aid: start, loaded, solved (Bt.dbg_cycles; fast_finish stamps the unpack)
#ifdef MPCX_PROFILE_ROUNDS
    long long pacc[6] = {0, 0, 0, 0, 0, 0}, plast = 0;
#endif
    auto stamp = [&](long long &t) { if (Bt.dbg_cycles) t = (long long)__builtin_readcyclecounter(); };
    stamp(ts0);

    // offsets of this lane's element pairs into the rows of Y (clamped: lanes past the end re-read pair 0, their results are never used)
    int offz[CPZ], offg[CPG];
#pragma unroll
    for (int c = 0; c < CPZ; ++c) { const int e = 128 * c + 2 * lane; offz[c] = e < ldz ? e : 0; }
#pragma unroll
    for (int c = 0; c < CPG; ++c) { const int r = 128 * c + 2 * lane; offg[c] = ldz + (r < ldg ? r : 0); }
    unsigned boffz[CPZ], boffg[CPG];                 // the same in bytes, as ws_solve_reg takes them
#pragma unroll
    for (int c = 0; c < CPZ; ++c) boffz[c] = (unsigned)offz[c] * 8u;
#pragma unroll
    for (int c = 0; c < CPG; ++c) boffg[c] = (unsigned)offg[c] * 8u;

    // ---- the assembled problem: the workspace record the assemble kernel left, copied into the slice, or computed in place
    if constexpr (SRC != 2) fast_init_pads<CPZ, CPG>(slice, ldz, ldg, lane);
    if constexpr (SRC == 2) {
        // nothing to do: the record is in place
    } else if constexpr (SRC == 1) {
        RecPtrs rp{fs, t0s, gt0s, lgs, ugs, tail};
        fused_record(M, Bt, b, lane, scratch, rp, mf_lds);
    } else {
#pragma unroll
        for (int c = 0; c < CPZ; ++c) {
            const int e = 128 * c + 2 * lane;
            if (e < ldz) {
                const d2 vf = ld2(ws + e), vt = ld2(ws + ldz + e);
                *reinterpret_cast<double2 *>(fs + e) = make_double2(vf.x, vf.y);
                *reinterpret_cast<double2 *>(t0s + e) = make_double2(vt.x, vt.y);
            }
        }
#pragma unroll
        for (int c = 0; c < CPG; ++c) {
            const int r = 128 * c + 2 * lane;
            if (r < ldg) {
                const d2 vt = ld2(ws + 2 * ldz + r), vl = ld2(ws + ldz + ldy + r), vu = ld2(ws + ldz + ldy + ldg + r);
                *reinterpret_cast<double2 *>(gt0s + r) = make_double2(vt.x, vt.y);
                *reinterpret_cast<double2 *>(lgs + r) = make_double2(vl.x, vl.y);
                *reinterpret_cast<double2 *>(ugs + r) = make_double2(vu.x, vu.y);
            }
        }
        if (lane == 0) { const d2 t = ld2(ws + ldz + ldy + 2 * ldg); *reinterpret_cast<double2 *>(tail) = make_double2(t.x, t.y); }
        wave_sync();
    }
    const double flag0 = tail[1];
    // a violated step-0 / input-independent row: see admm_solve_one (lmpc_kernels.hip)
    const bool fixed_violation = flag0 == 1.0;
    const bool infeasible = fixed_violation && M.strict_infeasible;

    // working-set state of this lane's rows: 0 free, -1 / +1 at the lower / upper bound, 2 equality row (always in, never shed)
    int actb[NZS], actg[NGS];
    const double ptol = 1e-8;
    // by how much v lies outside [lo, hi] widened by ptol max(1, |bound|), with the contractions written out: the low side's bound is widened first and v
    // subtracted from it, the high side subtracts first and widens the difference (what the compiler made of lo - ptol m - v and v - hi - ptol m)
    auto viol = [&](double v, double lo, double hi) {
        const double lo_wide = fma(-ptol, fmax(1.0, fabs(lo)), lo), hi_scale = fmax(1.0, fabs(hi));
        return fmax(fmax(lo_wide - v, fma(-ptol, hi_scale, v - hi)), 0.0);
    };
    // a working row's multiplier as "how wrong": lm at the lower bound (act = -1), -lm at the upper (act = 1), 0 for a free or an equality row (0, 2).
    // Bit arithmetic on the high word, no select and no branch: (act + 1) << 30 is the sign bit for act = 1 and nothing for act = -1, bit 0 of act
    // says whether the row counts at all.  -lm is the exact negation (the sign bit flipped), the 0 is +0.
    auto wrong_signed = [](double lm, int act) {
        const int in = -(act & 1);
        const int hi = (__double2hiint(lm) ^ (int)((unsigned)(act + 1) << 30)) & in;
        return __hiloint2double(hi, __double2loint(lm) & in);
    };
    {
        // first working set: equalities, and the rows the unconstrained optimum violates by >= MPCX_INIT_THETA x the largest violation
        double vb[NZS], vg[NGS], vinit = 0.0;
        bool lowb[NZS], lowg[NGS];
#pragma unroll
        for (int c = 0; c < CPZ; ++c) {
            const int e = 128 * c + 2 * lane;
            const double2 l = *reinterpret_cast<const double2 *>(lws + e), u = *reinterpret_cast<const double2 *>(uws + e);
            const double2 t = *reinterpret_cast<const double2 *>(t0s + e);
            vb[2 * c] = viol(t.x, l.x, u.x); vb[2 * c + 1] = viol(t.y, l.y, u.y);
            lowb[2 * c] = t.x < l.x; lowb[2 * c + 1] = t.y < l.y;
            actb[2 * c] = l.x == u.x ? 2 : 0; actb[2 * c + 1] = l.y == u.y ? 2 : 0;
            vinit = fmax(vinit, fmax(vb[2 * c], vb[2 * c + 1]));
        }
#pragma unroll
        for (int c = 0; c < CPG; ++c) {
            const int r = 128 * c + 2 * lane;
            const double2 l = *reinterpret_cast<const double2 *>(lgs + r), u = *reinterpret_cast<const double2 *>(ugs + r);
            const double2 t = *reinterpret_cast<const double2 *>(gt0s + r);
            vg[2 * c] = viol(t.x, l.x, u.x); vg[2 * c + 1] = viol(t.y, l.y, u.y);
            lowg[2 * c] = t.x < l.x; lowg[2 * c + 1] = t.y < l.y;
            if constexpr (SRC == 2) {
                actg[2 * c] = ((eqbits >> (2 * c)) & 1) ? 2 : 0; actg[2 * c + 1] = ((eqbits >> (2 * c + 1)) & 1) ? 2 : 0;
            } else {
                const d2 l0 = ld2(GP(lg0) + (offg[c] - ldz)), u0 = ld2(GP(ug0) + (offg[c] - ldz));
                const bool ok = r < ldg;
                actg[2 * c] = (ok && l0.x == u0.x) ? 2 : 0; actg[2 * c + 1] = (ok && l0.y == u0.y) ? 2 : 0;
            }
            vinit = fmax(vinit, fmax(vg[2 * c], vg[2 * c + 1]));
        }
        const double thr0 = MPCX_INIT_THETA * wave_max_dpp(vinit);
#pragma unroll
        for (int s = 0; s < NZS; ++s) actb[s] = (actb[s] == 0 && vb[s] > 0.0 && vb[s] >= thr0) ? (lowb[s] ? -1 : 1) : actb[s];
#pragma unroll
        for (int s = 0; s < NGS; ++s) actg[s] = (actg[s] == 0 && vg[s] > 0.0 && vg[s] >= thr0) ? (lowg[s] ? -1 : 1) : actg[s];
    }
    stamp(ts1);   // 1: loaded

    if (Bt.warm_lower) {
        // the first working set is the previous solve's active set; an equality row (2) stays in whatever the bits say
        const WarmStart warm(M, Bt, b);
#pragma unroll
        for (int s = 0; s < NZS; ++s) {
            const int e = 128 * (s >> 1) + 2 * lane + (s & 1);
            if (e < nz && actb[s] != 2) actb[s] = warm.box_side(e, lws[e], uws[e]);
        }
#pragma unroll
        for (int s = 0; s < NGS; ++s) {
            const int r = 128 * (s >> 1) + 2 * lane + (s & 1);
            if (r < mg && actg[s] != 2) actg[s] = warm.row_side(r);
        }
    }

    double wv[NZS], gw[NGS];
    int posb[NZS], posg[NGS];                        // position in the working set (kFastCap: not in it)
    double dtol_last = 0;
    int na_last = 0, rounds_total = 0;
    bool solved = false;

    if (!infeasible && M.polish) {
        const int rounds = M.polish_rounds0;
        for (int rd = 0; rd < rounds; ++rd) {
            ++rounds_total;
#ifdef MPCX_PROFILE_ROUNDS
            plast = (long long)__builtin_readcyclecounter();
#endif
            // A launch lasts as long as its slowest instance, and the slow ones are those that need many rounds: from the fourth
            // round on a wavefront asks the instruction arbiter for precedence over its three neighbours on the SIMD.
            if (rd == 3) __builtin_amdgcn_s_setprio(1);
            else if (rd == 5) __builtin_amdgcn_s_setprio(2);
            else if (rd == 7) __builtin_amdgcn_s_setprio(3);
            // ---- the working set, in row order, to LDS: unified index and bound value per row.  Straight-line code: a row that
            // is not in the set writes to the spare slot kFastCap (so does a row past the capacity, which ends the solve below).
            int na = 0;
#pragma unroll
            for (int c = 0; c < CPZ; ++c) {
                const int e = 128 * c + 2 * lane;
                const double2 l = *reinterpret_cast<const double2 *>(lws + e), u = *reinterpret_cast<const double2 *>(uws + e);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int s = 2 * c + h;
                    const bool act = actb[s] != 0;
                    const unsigned long long mk = __ballot(act);
                    int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, (unsigned)na));      // (na as the count's addend)
                    pos = (act && pos < kFastCap) ? pos : kFastCap;
                    posb[s] = pos;
                    wsidx[pos] = e + h;
                    wsb[pos] = actb[s] < 0 ? (h ? l.y : l.x) : (h ? u.y : u.x);
                    na += __popcll(mk);
                }
            }
#pragma unroll
            for (int c = 0; c < CPG; ++c) {
                const int r = 128 * c + 2 * lane;
                const double2 l = *reinterpret_cast<const double2 *>(lgs + r), u = *reinterpret_cast<const double2 *>(ugs + r);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int s = 2 * c + h;
                    const bool act = actg[s] != 0;
                    const unsigned long long mk = __ballot(act);
                    int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, (unsigned)na));      // (na as the count's addend)
                    pos = (act && pos < kFastCap) ? pos : kFastCap;
                    posg[s] = pos;
                    wsidx[pos] = ldz + r + h;
                    wsb[pos] = actg[s] < 0 ? (h ? l.y : l.x) : (h ? u.y : u.x);
                    na += __popcll(mk);
                }
            }
            if (na > kFastCap) break;                // left to the fallback kernel
            na_last = na;
            wave_sync();
            MPCX_LAP_WAIT(0);                        // 0: working set built and in LDS
            int dep_at = -1;
            double lmax = 0.0;
            // (SRC = 1, the kernels that compute the record themselves, keep the update's scalar reads: at 128 and 168 VGPRs every multiplier kept in a VGPR spills
            // there.  The elimination's DPP form holds no broadcast value in a register, and the resource listing decides where it goes
            // (profiles/r14_resource_usage_lmpc.txt): with it lmpc_solve_persistent<1, 1> goes from 188 to 204 B of scratch per lane, and lmpc_solve_fused
            // -- 124 VGPRs and no scratch either way -- is the same instantiation of this function, so SRC = 1 keeps the scalar reads; the four-chunk
            // variants go from 132 to 172 B of scratch and keep them too)
            constexpr auto dp = [](int cap) { return SRC != 1 && CPZ + CPG <= MPCX_FAST_DPP_CHUNKS && fast_class_bit(MPCX_FAST_DPP_CLASSES, cap); };
            constexpr auto xl = [](int cap) { return SRC != 1 && CPZ + CPG <= MPCX_FAST_LDSMULT_CHUNKS && fast_class_bit(MPCX_FAST_LDSMULT_CLASSES, cap); };
            if (na == 0) {
#pragma unroll
                for (int c = 0; c < CPZ; ++c) { const double2 v = *reinterpret_cast<const double2 *>(t0s + 128 * c + 2 * lane); wv[2 * c] = v.x; wv[2 * c + 1] = v.y; }
#pragma unroll
                for (int c = 0; c < CPG; ++c) { const double2 v = *reinterpret_cast<const double2 *>(gt0s + 128 * c + 2 * lane); gw[2 * c] = v.x; gw[2 * c + 1] = v.y; }
            } else if (na <= 4) dep_at = ws_solve_reg<4, 1, CPZ, CPG, dp(4), xl(4)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            else if (na <= 6) dep_at = ws_solve_reg<6, 5, CPZ, CPG, dp(6), xl(6)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            else if (na <= 8) dep_at = ws_solve_reg<8, 7, CPZ, CPG, dp(8), xl(8)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            else if (na <= 10) dep_at = ws_solve_reg<10, 9, CPZ, CPG, dp(10), xl(10)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            else if (na <= 12) dep_at = ws_solve_reg<12, 11, CPZ, CPG, dp(12), xl(12)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            else if (na <= 14) dep_at = ws_solve_reg<14, 13, CPZ, CPG, dp(14), xl(14)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            else dep_at = ws_solve_reg<kFastCap, 15, CPZ, CPG, dp(kFastCap), xl(kFastCap)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
            if (dep_at >= 0) {
                // linearly dependent working set: drop the offending row and try again
                row_leaves(wsidx[dep_at], ldz, lane, actb, actg);
                wave_sync();
                continue;
            }
            wave_sync();                             // lam is in LDS
            MPCX_LAP_WAIT(3);                        // 3: w = t0 - Y[:, A] lambda, multipliers in LDS
            const double dtol = 1e-9 * lmax + 1e-300;
            dtol_last = dtol;
            // ---- how wrong is each working row's multiplier (> dtol: wrong sign), how violated each free row: straight-line code,
            // every slot looks a multiplier up (0 in the spare slot) and measures a violation; a select (violation) and the state's bits (multiplier) decide which one counts
            double badb[NZS], badg[NGS], vb[NZS], vg[NGS], vm = 0.0, bm = 0.0, chk = 0.0;
            bool lowb[NZS], lowg[NGS];
            double lmb[NZS], lmg[NGS];
#pragma unroll
            for (int s = 0; s < NZS; ++s) lmb[s] = lam[posb[s]];
#pragma unroll
            for (int s = 0; s < NGS; ++s) lmg[s] = lam[posg[s]];
#pragma unroll
            for (int c = 0; c < CPZ; ++c) {
                const int e = 128 * c + 2 * lane;
                const double2 l = *reinterpret_cast<const double2 *>(lws + e), u = *reinterpret_cast<const double2 *>(uws + e);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int s = 2 * c + h;
                    const double lo = h ? l.y : l.x, hi = h ? u.y : u.x;
                    chk += wv[s];
                    lowb[s] = wv[s] < lo;
                    const double v = viol(wv[s], lo, hi);
                    vb[s] = actb[s] == 0 ? v : 0.0;
                    badb[s] = wrong_signed(lmb[s], actb[s]);
                    vm = fmax(vm, vb[s]); bm = fmax(bm, badb[s]);
                }
            }
#pragma unroll
            for (int c = 0; c < CPG; ++c) {
                const int r = 128 * c + 2 * lane;
                const double2 l = *reinterpret_cast<const double2 *>(lgs + r), u = *reinterpret_cast<const double2 *>(ugs + r);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int s = 2 * c + h;
                    const double lo = h ? l.y : l.x, hi = h ? u.y : u.x;
                    chk += gw[s];
                    lowg[s] = gw[s] < lo;
                    const double v = viol(gw[s], lo, hi);
                    vg[s] = actg[s] == 0 ? v : 0.0;
                    badg[s] = wrong_signed(lmg[s], actg[s]);
                    vm = fmax(vm, vg[s]); bm = fmax(bm, badg[s]);
                }
            }
            if (wave_any(!(chk - chk == 0.0))) break;       // a NaN or an infinity in the point: left to the fallback kernel
            MPCX_LAP(4);                             // 4: multipliers and violations
            const bool any_bad = wave_any(bm > dtol), any_viol = wave_any(vm > 0.0);
            if (!any_bad && !any_viol) { solved = true; break; }
            if (rd < MPCX_FAST_SAFE_AFTER) {
                // every wrong-signed row leaves, and the rows violated by at least MPCX_FAST_ADD_THETA x the largest violation enter
                const double thr = any_viol ? (rd < 3 ? MPCX_FAST_ADD_THETA : MPCX_FAST_ADD_THETA_LATE) * wave_max_dpp(vm) : INF;
#pragma unroll
                for (int s = 0; s < NZS; ++s) actb[s] = badb[s] > dtol ? 0 : ((vb[s] > 0.0 && vb[s] >= thr) ? (lowb[s] ? -1 : 1) : actb[s]);
#pragma unroll
                for (int s = 0; s < NGS; ++s) actg[s] = badg[s] > dtol ? 0 : ((vg[s] > 0.0 && vg[s] >= thr) ? (lowg[s] ? -1 : 1) : actg[s]);
            } else {
                // an instance that is still here (none in 40 000 of the benchmark workloads: the rule above may cycle in principle) goes
                // on with one exchange per round: the most wrong multiplier leaves, else the most violated row enters
                const double mx = wave_max_dpp(any_bad ? bm : vm);
                int slot = -1;
#pragma unroll
                for (int s = 0; s < NZS; ++s) if (slot < 0 && (any_bad ? badb[s] : vb[s]) == mx) slot = s;
#pragma unroll
                for (int s = 0; s < NGS; ++s) if (slot < 0 && (any_bad ? badg[s] : vg[s]) == mx) slot = NZS + s;
                const unsigned long long mk = __ballot(slot >= 0);
                if (slot >= 0 && lane == (int)__builtin_ctzll(mk)) {
#pragma unroll
                    for (int s = 0; s < NZS; ++s) if (slot == s) actb[s] = any_bad ? 0 : (lowb[s] ? -1 : 1);
#pragma unroll
                    for (int s = 0; s < NGS; ++s) if (slot == NZS + s) actg[s] = any_bad ? 0 : (lowg[s] ? -1 : 1);
                }
            }
            wave_sync();
            MPCX_LAP(5);                             // 5: repair
        }
    }
    __builtin_amdgcn_s_setprio(0);
    stamp(ts2);   // 2: solved

    // lmpc_solve_group re-reads its kernel arguments here (see GroupArgs): the empty asm keeps the compiler from loading a field the finish needs
    // ahead of the rounds and carrying it through them
    if constexpr (SRC == 2) {
        group_args_p ka = (group_args_p)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        fast_finish<CPZ, CPG, SRC>((const LmpcDev &)ka->M, (const LmpcBatchDev &)ka->Bt, b, lane, slice, lwuw, ws, outs, infeasible, solved, fixed_violation,
                                   wv, actb, actg, posb, posg, dtol_last, na_last, rounds_total, ts0, ts1, ts2 MPCX_PROF_PASS);
    } else {
        fast_finish<CPZ, CPG, SRC>(M, Bt, b, lane, slice, lwuw, ws, outs, infeasible, solved, fixed_violation,
                                   wv, actb, actg, posb, posg, dtol_last, na_last, rounds_total, ts0, ts1, ts2 MPCX_PROF_PASS);
    }
}

// waves per SIMD the lean kernels are compiled for: the one-chunk variant fits 128 VGPRs
#ifndef MPCX_FAST_WAVES1
#define MPCX_FAST_WAVES1 4
#endif
#ifndef MPCX_FAST_WAVES2
#define MPCX_FAST_WAVES2 2
#endif
template <int CPZ> constexpr int fast_waves() { return CPZ == 1 ? MPCX_FAST_WAVES1 : (CPZ == 2 ? MPCX_FAST_WAVES2 : 2); }     // (CPZ = 2 at three per SIMD: 7 % faster at config 4, but 20 spilled VGPRs = 74 MB of scratch writes per 32 768)

// LDS of the lean kernels: [lw | uw] of the workgroup (padded to whole lane pairs), then one slice per wavefront (M.fast_slice doubles)
template <int CPZ>
__device__ __forceinline__ void fast_load_box(const LmpcDev &M, double *lwuw)
{
    constexpr int ZP = 128 * CPZ;
    const double INF = __builtin_huge_val();
    for (int e = 2 * (int)threadIdx.x; e < ZP; e += 2 * (int)blockDim.x) {
        const bool ok = e < M.ldz;
        const d2 vl = ld2(GP(lw) + (ok ? e : 0)), vu = ld2(GP(uw) + (ok ? e : 0));
        *reinterpret_cast<double2 *>(lwuw + e) = ok ? make_double2(vl.x, vl.y) : make_double2(-INF, -INF);
        *reinterpret_cast<double2 *>(lwuw + ZP + e) = ok ? make_double2(vu.x, vu.y) : make_double2(INF, INF);
    }
    __syncthreads();
}

template <int CPZ, int CPG>
__global__ __launch_bounds__(kWavesPerBlock * 64, fast_waves<CPZ>()) void lmpc_solve(const LmpcDev *__restrict__ Mp, const LmpcBatchDev Bt, double *wsbase)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform, and known to be: the instance number and what is addressed with it stay scalar)
    constexpr int ZP = 128 * CPZ;
    const int wpb = blockDim.x >> 6;
    double *rec = smem + 2 * ZP + (size_t)wave * M.fast_slice;
    fast_load_box<CPZ>(M, smem);
    // one instance per wavefront, no loop over instances: the grid covers the batch (a loop makes the compiler hoist the per-lane
    // addresses of every input and output array out of it and keep them alive -- in scratch, i.e. in HBM -- across the whole solve)
    const int i = blockIdx.x * wpb + wave;
    if (i < Bt.batch) solve_fast<CPZ, CPG, 0>(M, Bt, i, lane, rec, smem, glw(wsbase) + (size_t)i * M.wsld);
}

// The same for a heterogeneous batch (mpcx_lmpc_hetero_*): every instance its own model struct, so every wavefront keeps its own
// copy of the box bounds (after the slices).  A kernel of its own: the shared-model kernel above keeps its register allocation.
template <int CPZ, int CPG>
__global__ __launch_bounds__(kWavesPerBlock * 64, fast_waves<CPZ>()) void lmpc_solve_hetero(const LmpcDev *__restrict__ Mp, const LmpcBatchDev Bt, double *wsbase)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform, and known to be: the instance number and what is addressed with it stay scalar)
    constexpr int ZP = 128 * CPZ;
    const int wpb = blockDim.x >> 6;
    double *rec = smem + 2 * ZP + (size_t)wave * M.fast_slice;
    double *box = smem + 2 * ZP + (size_t)wpb * M.fast_slice + (size_t)wave * 2 * ZP;
    const double INF = __builtin_huge_val();
    const int i = blockIdx.x * wpb + wave;
    if (i < Bt.batch) {
        const LmpcDev &Mi = Mp[lmpc_model_of(Bt, i)];
#pragma unroll
        for (int c = 0; c < CPZ; ++c) {
            const int e = 128 * c + 2 * lane;
            const bool ok = e < Mi.ldz;
            const d2 vl = ld2(gl(Mi.lw) + (ok ? e : 0)), vu = ld2(gl(Mi.uw) + (ok ? e : 0));
            *reinterpret_cast<double2 *>(box + e) = ok ? make_double2(vl.x, vl.y) : make_double2(-INF, -INF);
            *reinterpret_cast<double2 *>(box + ZP + e) = ok ? make_double2(vu.x, vu.y) : make_double2(INF, INF);
        }
        wave_sync();
        solve_fast<CPZ, CPG, 0>(Mi, Bt, i, lane, rec, box, glw(wsbase) + (size_t)i * M.wsld);
        wave_sync();
    }
}

// The same with the record computed in place (no assemble kernel, no workspace traffic): instances in batch order
template <int CPZ, int CPG>
__global__ __launch_bounds__(kWavesPerBlock * 64, fast_waves<CPZ>()) void lmpc_solve_fused(const LmpcDev *__restrict__ Mp, const LmpcBatchDev Bt, double *wsbase)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform, and known to be: the instance number and what is addressed with it stay scalar)
    fast_load_box<CPZ>(M, smem);
    double *rec = smem + 2 * 128 * CPZ + (size_t)wave * M.fast_slice;
    const int wpb = blockDim.x >> 6;
    const int b = blockIdx.x * wpb + wave;
    if (b < Bt.batch) solve_fast<CPZ, CPG, 1>(M, Bt, b, lane, rec, smem, glw(wsbase) + (size_t)b * M.wsld);
}

// The fused form as a persistent kernel: one workgroup of kPersistWaves wavefronts per CU loads the composed map into LDS once
// (87.5 KB at N = 20; with twelve 5.6 KB slices 157 of the 160 KB of a CU), then every wavefront pulls instances from a device
// counter until the batch is exhausted -- the record of an instance costs one pass over LDS instead of a round trip through
// HBM, nobody waits for a neighbour, and an early finisher simply takes the next instance.
constexpr int kPersistWaves = 12;
template <int CPZ, int CPG>
__global__ __launch_bounds__(kPersistWaves * 64) void lmpc_solve_persistent(const LmpcDev *__restrict__ Mp, const LmpcBatchDev Bt, double *wsbase,
                                                                             int *counter)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LmpcDev &M = *Mp;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform, and known to be: the instance number and what is addressed with it stay scalar)
    const int nmf = M.rowsF * M.kin;                  // even
    {
        const gdp src = gl(Bt.fused == 2 ? M.MF1 : M.MF0);
        for (int k = 2 * (int)threadIdx.x; k < nmf; k += 2 * (int)blockDim.x) {
            const d2 v = ld2(src + k);
            *reinterpret_cast<double2 *>(smem + k) = make_double2(v.x, v.y);
        }
    }
    double *lwuw = smem + nmf;
    fast_load_box<CPZ>(M, lwuw);
    double *rec = lwuw + 2 * 128 * CPZ + (size_t)wave * M.fast_slice;
    // The first instance of a wavefront is its own number; the rest of the batch is handed out by eight counters (one per
    // residue of the workgroup number, i.e. per XCD under the usual placement), each over every eighth instance: a single
    // device-scope counter serves about 88 pulls per microsecond, which thousands of wavefronts starting together would queue on.
    const int nwaves = gridDim.x * kPersistWaves, shard = blockIdx.x & 7;
    int b = blockIdx.x * kPersistWaves + wave;
    while (b < Bt.batch) {
        solve_fast<CPZ, CPG, 1>(M, Bt, b, lane, rec, lwuw, glw(wsbase) + (size_t)b * M.wsld, smem);
        int n = 0;
        if (lane == 0) n = atomicAdd(counter + shard, 1);
        n = __builtin_amdgcn_readfirstlane(n);
        b = nwaves + shard + 8 * n;
    }
}

// =====================================================================================
// assemble + solve in one workgroup: sixteen instances per workgroup of sixteen wavefronts
// =====================================================================================
// Phase 1 is lmpc_assemble_mfma (lmpc_kernels.hip) on sixteen wavefronts instead of four: ProblemBuilder::get for sixteen instances
// as two small GEMMs on v_mfma_f64_16x16x4_f64 (instances = the N dimension), every row tile written straight into the LDS slice
// of its instance.  Phase 2: wavefront w solves instance w from its slice (solve_fast, SRC = 2).  No workspace record, no second
// launch: the only HBM traffic of a solve is its inputs and outputs.  One workgroup per CU; at the benchmark batch the launch is
// one workgroup deep.  A workgroup moves on when its slowest instance is done, so long batches use the two-kernel path instead.
// Round 5: the two-chunk variant too (CPZ = CPG = 2: up to 256 condensed variables -- config 4's N = 50).  Its slices are 10.9 KB, so a workgroup
// holds EIGHT instances on eight wavefronts (eight of the sixteen MFMA columns carry an instance, the others repeat the last one and store
// nothing); such a controller's cost comes from its definition: behind the solves, H times the workgroup's solutions on the matrix pipe, by the arithmetic of
// lmpc_cost_mfma step for step, so that the cost is the two-kernel form's bit for bit (round 11; it was one product with H per instance inside solve_fast, whose
// summation agreed with the other form's to 6e-12 only).
// The kernel arguments are a kilobyte here (the model struct by value) and the compiler fetches each field where it is first used: a dozen scalar
// loads on different cache lines, each a miss, one after the other.  Touch every 64-byte line of the segment at once instead (one dword each, all
// requested before the one wait), after which the compiler's own loads hit the scalar cache.
template <size_t BYTES>
__device__ __forceinline__ void kernarg_touch()
{
    static_assert(BYTES <= 16 * 64 && BYTES > 15 * 64, "kernarg_touch covers sixteen lines, the sixteenth must exist");
    const auto ka = __builtin_amdgcn_kernarg_segment_ptr();
    int t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11, t12, t13, t14, t15;
    asm volatile("s_load_dword %0, %16, 0x0\n\ts_load_dword %1, %16, 0x40\n\ts_load_dword %2, %16, 0x80\n\ts_load_dword %3, %16, 0xc0\n\t"
                 "s_load_dword %4, %16, 0x100\n\ts_load_dword %5, %16, 0x140\n\ts_load_dword %6, %16, 0x180\n\ts_load_dword %7, %16, 0x1c0\n\t"
                 "s_load_dword %8, %16, 0x200\n\ts_load_dword %9, %16, 0x240\n\ts_load_dword %10, %16, 0x280\n\ts_load_dword %11, %16, 0x2c0\n\t"
                 "s_load_dword %12, %16, 0x300\n\ts_load_dword %13, %16, 0x340\n\ts_load_dword %14, %16, 0x380\n\ts_load_dword %15, %16, 0x3c0\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3), "=&s"(t4), "=&s"(t5), "=&s"(t6), "=&s"(t7), "=&s"(t8), "=&s"(t9), "=&s"(t10), "=&s"(t11),
                   "=&s"(t12), "=&s"(t13), "=&s"(t14), "=&s"(t15)
                 : "s"(ka)
                 : "memory");
}
#ifndef MPCX_GROUP_BALANCE
#define MPCX_GROUP_BALANCE 1
#endif

template <int CPZ> constexpr int kGroupWavesOf = CPZ == 1 ? 16 : 8;
constexpr int kGroupG2 = 5;               // groups of four MFMA k-steps of the second product whose A operands are in flight together (the whole of N = 20's)
constexpr int kGroupG1 = 2;               // ... of the first product (kin = 32: the whole of it for up to 12 states, 4 inputs and 12 outputs)
// Round 6: the phase's trips to memory side by side.  A launch starts with cold caches (the controller's factors come from the memory side once per
// XCD and launch) and the phase used to chain its first-touch loads: the model struct, the box bounds, the inputs, the first product's operands,
// the row bounds of its epilogue, the second product's operands, the bounds again at the head of the solve -- seven dependent trips of 1.5-2 us
// each before the first round.  Now the model struct travels in the kernel arguments and every wavefront requests ALL of what the phase will
// touch before it waits for any of it: one trip.  The products take their operands in the old order (the same bits), from copies of the maps laid
// out as the MFMA wants them (LmpcDev::MA0p / MA1p / Ymp: a lane's operands of four k-steps are 32 contiguous bytes, a wavefront's 2 KB): the phase
// was bound by the instruction rate of the vector memory pipe -- forty-odd 8-byte loads per lane, 64 lanes on four rows each -- not by its bytes.
// Measured by cutting the kernel short (tools/group_cut.py; quadrotor N = 20, 4096 instances, us per step with the idle fallback launch): empty
// 6.9, inputs staged 7.6, first product 10.6, second product 15.3, whole 49.0 before the packed copies.
template <int CPZ, int CPG>
__global__ __launch_bounds__(kGroupWavesOf<CPZ> * 64) void lmpc_solve_group(const LmpcDev Mv, const LmpcBatchDev Btv, double *wsbasev, const int variantv)
{
    constexpr int kGroupWaves = kGroupWavesOf<CPZ>;
    extern __shared__ __attribute__((aligned(16))) double smem[];
#if defined(MPCX_GROUP_CUT) && MPCX_GROUP_CUT == 0
    { return; }                                   // (timing experiment, tools/group_cut.sh: what a launch costs up to here)
#endif
    kernarg_touch<sizeof(LmpcDev) + sizeof(LmpcBatchDev) + sizeof(double *) + sizeof(int)>();
    const group_args_p ka = (group_args_p)__builtin_amdgcn_kernarg_segment_ptr();      // (see GroupArgs)
    const LmpcDev &M = (const LmpcDev &)ka->M;
    const LmpcBatchDev &Bt = (const LmpcBatchDev &)ka->Bt;
    double *const wsbase = ka->wsbase;
    const int variant = ka->variant;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int nx = M.nx, nu = M.nu, ny = M.ny;
    const int kin4 = M.kin >> 2, nz4 = M.nz16 >> 2;
    const int ldz = M.ldz, ldg = M.ldg, ldy = M.ldy;
    constexpr int ZP = 128 * CPZ, GPD = 128 * CPG;
    double *lwuw = smem;
    double *slices = lwuw + 2 * ZP;
    double *Bv = slices + (size_t)kGroupWaves * M.fast_slice;      // [kin4][64]   vin as MFMA B operands
    double *Bf = Bv + (size_t)kin4 * 64;                           // [nz4][64]    f as MFMA B operands
    double *c0s = Bf + (size_t)nz4 * 64;                           // [16 wavefronts][16 instances]
    unsigned *bad = reinterpret_cast<unsigned *>(c0s + kGroupWaves * 16);   // [16]
    const int outld = 8 + ((nu + 1) & ~1);
    double *outs = c0s + kGroupWaves * 16 + 16;                             // [16][8 + nu]: results of the sixteen instances
    double *mine = slices + (size_t)wave * M.fast_slice;
    const gdp MAp = gl(variant ? M.MA1p : M.MA0p), Ymp = GP(Ymp);
    const int ntile1 = M.rowsA >> 4, tg = M.nz16 >> 4, ts = tg + (M.mg16 >> 4), tq = ts + (M.ns16 >> 4);
    const int ntile2 = M.ldy16 >> 4;
    const int G1 = (kin4 + 3) >> 2, G2 = (nz4 + 3) >> 2;          // k-step groups per row tile of the packed maps
    auto ld4 = [](gdp p) -> v4d { return *reinterpret_cast<const v4d MPCX_GAS *>(p); };
    // the slice of instance j (this lane's MFMA column; a column beyond the workgroup's instances computes a copy and stores nothing)
    const bool jlive = j < kGroupWaves;
    double *sj = slices + (size_t)(jlive ? j : 0) * M.fast_slice;
    double *t0j = sj, *gt0j = sj + ZP, *lgj = gt0j + GPD, *ugj = lgj + GPD, *fj = ugj + GPD;

    const int b0 = blockIdx.x * kGroupWaves;    // one batch of sixteen (eight) per workgroup, no loop (see lmpc_solve)
    const int bj = b0 + (jlive ? j : kGroupWaves - 1);
    const int bc = bj < Bt.batch ? bj : Bt.batch - 1;
    // profiling aid: when the wavefront started, when the first product was done, when the records were complete
    auto gstamp = [&](int k) { if (Bt.dbg_cycles && lane == 0 && b0 + wave < Bt.batch) Bt.dbg_cycles[(size_t)(b0 + wave) * 8 + k] = (long long)__builtin_readcyclecounter(); };
    gstamp(4);

    // ---- every first-touch load of the phase, requested before anything waits
    // vin operands: k-step kb holds rows 4 kb + kq of instance j (one predicated load per lane: the branches only choose the address)
    auto vin_at = [&](int kb) -> double {
        const int k = 4 * kb + kq;
        gdp src = gl(Bt.x0);
        bool ld = false;
        if (k < M.nxp) { ld = k < nx; src = gl(Bt.x0) + ((size_t)bc * nx + k); }
        else if (k < M.nxp + M.nup) { const int c = k - M.nxp; ld = c < nu; src = gl(Bt.u0) + ((size_t)bc * nu + c); }
        else if (k < M.ione) { const int c = k - M.nxp - M.nup; ld = variant && c < ny; src = gl(Bt.yref) + ((size_t)bc * Bt.yref_bs + c); }
        double v = k == M.ione ? 1.0 : 0.0;
        if (ld) v = *src;
        return v;
    };
    const double vin0 = wave < kin4 ? vin_at(wave) : 0.0;
    // the box bounds (the workgroup's copy: the first ZP / 2 threads hold a pair each)
    const int ebx = 2 * (int)threadIdx.x;
    const bool boxok = ebx < ldz;
    d2 bxl = {0.0, 0.0}, bxu = {0.0, 0.0};
    if (ebx < ZP) { bxl = ld2(GP(lw) + (boxok ? ebx : 0)); bxu = ld2(GP(uw) + (boxok ? ebx : 0)); }
    // first product: the operands of this wavefront's first tile (a wavefront without one requests the last tile's: no divergence, nothing used)
    const int t1 = wave < ntile1 ? wave : ntile1 - 1;
    v4d a1[kGroupG1];
#pragma unroll
    for (int g = 0; g < kGroupG1; ++g) a1[g] = ld4(MAp + (((size_t)t1 * G1 + (g < G1 ? g : 0)) * 64 + lane) * 4);
    // ... and what its epilogue compares with or subtracts from: four rows of (lg0, ug0) or of (slo, shi)
    double eblo[4], ebhi[4];
    {
        const bool ing = t1 >= tg && t1 < ts, ins = t1 >= ts && t1 < tq;
        const gdp plo = ing ? GP(lg0) + 16 * (t1 - tg) : GP(slo) + 16 * (ins ? t1 - ts : 0);
        const gdp phi = ing ? GP(ug0) + 16 * (t1 - tg) : GP(shi) + 16 * (ins ? t1 - ts : 0);
        const int lim = ing ? ldg - 16 * (t1 - tg) : (ins ? M.ns - 16 * (t1 - ts) : 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + kq;
            eblo[r] = 0.0; ebhi[r] = 0.0;
            if (row < lim) { eblo[r] = plo[row]; ebhi[r] = phi[row]; }
        }
    }
    // second product: the operands of this wavefront's first tile
    const int t2 = wave < ntile2 ? wave : ntile2 - 1;
    v4d a2[kGroupG2];
#pragma unroll
    for (int g = 0; g < kGroupG2; ++g) a2[g] = ld4(Ymp + (((size_t)t2 * G2 + (g < G2 ? g : 0)) * 64 + lane) * 4);
    // the solve's first look at the general rows -- which are equalities (lg0 == ug0) -- is the same for every instance: the last wavefront looks
    d2 eql[CPG], equ[CPG];
#pragma unroll
    for (int c = 0; c < CPG; ++c) {
        const int r = 128 * c + 2 * lane;
        eql[c] = d2{0.0, 0.0}; equ[c] = d2{1.0, 1.0};
        if (wave == kGroupWaves - 1) { eql[c] = ld2(GP(lg0) + (r < ldg ? r : 0)); equ[c] = ld2(GP(ug0) + (r < ldg ? r : 0)); }
    }

    fast_init_pads<CPZ, CPG>(mine, ldz, ldg, lane);      // (the previous instance's active-set bitmaps may have run over them)
    if (wave < kin4) Bv[wave * 64 + lane] = vin0;
    for (int kb = wave + kGroupWaves; kb < kin4; kb += kGroupWaves) Bv[kb * 64 + lane] = vin_at(kb);
    if (ebx < ZP) {
        const double INF = __builtin_huge_val();
        *reinterpret_cast<double2 *>(lwuw + ebx) = boxok ? make_double2(bxl.x, bxl.y) : make_double2(-INF, -INF);
        *reinterpret_cast<double2 *>(lwuw + ZP + ebx) = boxok ? make_double2(bxu.x, bxu.y) : make_double2(INF, INF);
    }
    if (threadIdx.x < 16) bad[threadIdx.x] = 0u;
    __syncthreads();
    gstamp(7);
#if defined(MPCX_GROUP_CUT) && MPCX_GROUP_CUT == 1
    { return; }
#endif

    {
        double c0p = 0.0;
        bool badl = false;
        auto tile1 = [&]<bool PRE>(const int t) {
            v4d acc = {0.0, 0.0, 0.0, 0.0};
            for (int g0 = 0; g0 < G1; g0 += kGroupG1) {
                v4d a[kGroupG1];
#pragma unroll
                for (int g = 0; g < kGroupG1; ++g) a[g] = (PRE && g0 == 0) ? a1[g] : ld4(MAp + (((size_t)t * G1 + (g0 + g < G1 ? g0 + g : g0)) * 64 + lane) * 4);
#pragma unroll
                for (int g = 0; g < kGroupG1; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kb = 4 * (g0 + g) + e;
                        if (kb < kin4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g][e], Bv[kb * 64 + lane], acc, 0, 0, 0);      // (kb is wave-uniform)
                    }
            }
            if (t < tg) {
                // linear term: operand of the second product, and the instance's f
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    Bf[(4 * t + r) * 64 + lane] = acc[r];
                    const int row = 16 * t + 4 * r + kq;
                    if (jlive && row < ldz) fj[row] = acc[r];
                }
            } else if (t < ts) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * (t - tg) + 4 * r + kq;
                    if (jlive && row < ldg) {
                        const double l0 = PRE ? eblo[r] : GP(lg0)[row], u0 = PRE ? ebhi[r] : GP(ug0)[row];
                        lgj[row] = l0 - acc[r]; ugj[row] = u0 - acc[r];
                    }
                }
            } else if (t < tq) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * (t - ts) + 4 * r + kq;
                    if (row < M.ns) badl |= violates(acc[r], PRE ? eblo[r] : GP(slo)[row], PRE ? ebhi[r] : GP(shi)[row], M.eps_abs, M.eps_rel);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kb2 = 4 * (t - tq) + r;
                    if (kb2 < kin4) c0p = fma(0.5 * Bv[kb2 * 64 + lane], acc[r], c0p);
                }
            }
        };
        int *eqb = reinterpret_cast<int *>(outs + kGroupWaves * outld);      // [64] the equality flags of the general rows, for every wavefront's solve
        if (wave < ntile1) tile1.template operator()<true>(wave);
        for (int t = wave + kGroupWaves; t < ntile1; t += kGroupWaves) tile1.template operator()<false>(t);
        if (badl && jlive) atomicOr(&bad[j], 1u);
        // this wavefront's share of the cost constant of instance j (no atomics: the sum must not depend on arrival order)
        c0p = wave_sum_rows(c0p);
        if (kq == 0) c0s[wave * 16 + j] = c0p;
        __syncthreads();
        gstamp(5);
#if defined(MPCX_GROUP_CUT) && MPCX_GROUP_CUT == 2
        { return; }
#endif

        auto tile2 = [&]<bool PRE>(const int t) {
            v4d acc = {0.0, 0.0, 0.0, 0.0};
            for (int g0 = 0; g0 < G2; g0 += kGroupG2) {
                v4d a[kGroupG2];
#pragma unroll
                for (int g = 0; g < kGroupG2; ++g) a[g] = (PRE && g0 == 0) ? a2[g] : ld4(Ymp + (((size_t)t * G2 + (g0 + g < G2 ? g0 + g : g0)) * 64 + lane) * 4);
#pragma unroll
                for (int g = 0; g < kGroupG2; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kb = 4 * (g0 + g) + e;
                        if (kb < nz4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g][e], Bf[kb * 64 + lane], acc, 0, 0, 0);
                    }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * r + kq;
                if (!jlive) continue;
                if (row < ldz) t0j[row] = acc[r];
                else if (row < ldy) gt0j[row - ldz] = acc[r];
            }
        };
        if (wave < ntile2) tile2.template operator()<true>(wave);
        for (int t = wave + kGroupWaves; t < ntile2; t += kGroupWaves) tile2.template operator()<false>(t);
        if (wave == kGroupWaves - 1) {                          // (a wavefront without a tile of the second product at the benchmark's sizes)
            int bits = 0;
#pragma unroll
            for (int c = 0; c < CPG; ++c) {
                const bool ok = 128 * c + 2 * lane < ldg;
                bits |= ((ok && eql[c].x == equ[c].x) ? 1 : 0) << (2 * c) | ((ok && eql[c].y == equ[c].y) ? 1 : 0) << (2 * c + 1);
            }
            eqb[lane] = bits;
        }
        // (round 11 moved this section to the last wavefront, which has no tile of the second product at the benchmark's sizes: no gain, not kept)
        if (threadIdx.x < kGroupWaves) {
            double *tl = slices + (size_t)threadIdx.x * M.fast_slice + 2 * ZP + 3 * GPD;
            double c0 = 0.0;
            for (int w = 0; w < kGroupWaves; ++w) c0 += c0s[w * 16 + threadIdx.x];
            tl[0] = c0;
            tl[1] = bad[threadIdx.x] ? 1.0 : 0.0;
        }
        __syncthreads();
        const int eqbits = eqb[lane];
        // ---- which wavefront solves which instance.  A launch of the benchmark batch holds every instance at once, four wavefronts on every SIMD, and it
        // ends when the busiest SIMD has issued the rounds of its four: the time of the launch is that SIMD's work (tools/group_phases.py: solves of six
        // rounds took 45 k cycles at the median and 78 k where the three neighbours were long ones too -- 25 rounds on the worst SIMD of the batch against
        // 14 on average; asking the arbiter for precedence changes nothing, measured).  How many rounds an instance will need is not known, but how far its
        // unconstrained optimum lies outside the bounds says a good deal about it (the sum of the violations correlates 0.83 with the rounds over the
        // benchmark batch, their number 0.76: tools/activeset_sim.py), and the slices are in LDS: the instances are dealt to the wavefronts in the order of
        // that sum, back and forth over the four SIMDs (wavefront w runs on SIMD w mod 4) -- the worst SIMD's rounds 25 -> 22 in the simulation (19 with the
        // rounds known beforehand, 18.2 = a quarter of the worst workgroup's), the step 0.0460 -> 0.0408 ms on the GPU (dealt by the number: 0.0425).
        int inst = wave;
#if MPCX_GROUP_BALANCE
        if (b0 + kGroupWaves <= Bt.batch) {
            const double *t0m = mine, *gt0m = mine + ZP, *lgm = gt0m + GPD, *ugm = lgm + GPD;
            auto over = [](double v, double lo, double hi) { return fmax(fmax(lo - v, v - hi), 0.0); };
            double sv = 0.0;
#pragma unroll
            for (int c = 0; c < CPZ; ++c) {
                const int e = 128 * c + 2 * lane;
                const double2 l = *reinterpret_cast<const double2 *>(lwuw + e), u = *reinterpret_cast<const double2 *>(lwuw + ZP + e), t = *reinterpret_cast<const double2 *>(t0m + e);
                sv += over(t.x, l.x, u.x) + over(t.y, l.y, u.y);
            }
#pragma unroll
            for (int c = 0; c < CPG; ++c) {
                const int r = 128 * c + 2 * lane;
                const double2 l = *reinterpret_cast<const double2 *>(lgm + r), u = *reinterpret_cast<const double2 *>(ugm + r), t = *reinterpret_cast<const double2 *>(gt0m + r);
                sv += over(t.x, l.x, u.x) + over(t.y, l.y, u.y);
            }
            // (the key's bits reach no result: a changed key can only change which wavefront solves which instance, never what the solve of an instance
            // computes -- so the cheapest deterministic sum serves, not wave_sum's tree)
            sv = wave_sum_any(sv);
            double *keys = reinterpret_cast<double *>(bad);      // (the flags were read before the barrier above; sixteen doubles are theirs)
            if (lane == 0) keys[wave] = sv;
            __syncthreads();
            // (the rank of instance `me`: the sixteen comparisons as four per lane, lane (me, part) against keys 4 part .. 4 part + 3, the parts added up by two
            // lane exchanges -- a quarter of the vector instructions of sixteen broadcasts per lane, in a kernel that is bound by them)
            const int me = lane & (kGroupWaves - 1), part = lane >> 4;
            const double ki = keys[me];
            int rank = 0;
#pragma unroll
            for (int q = 0; q < kGroupWaves / 4; ++q) {
                const int jj = (kGroupWaves / 4) * part + q;
                const double kj = keys[jj];
                rank += (kj > ki || (kj == ki && jj < me)) ? 1 : 0;
            }
            rank = wave_sum_rows(rank);
            const int q = rank >> 2, sd = (q & 1) ? 3 - (rank & 3) : (rank & 3);
            inst = (int)__builtin_ctzll(__ballot(lane < kGroupWaves && 4 * q + sd == wave));      // (a permutation: exactly one lane answers)
        }
#endif
        double *const slice_i = slices + (size_t)inst * M.fast_slice;
        const int b = b0 + inst;
        gstamp(6);
#if defined(MPCX_GROUP_CUT) && MPCX_GROUP_CUT == 3
        { return; }
#endif
        if (b < Bt.batch) solve_fast<CPZ, CPG, 2>(M, Bt, b, lane, slice_i, lwuw, glw(wsbase) + (size_t)b * M.wsld, nullptr, outs + inst * outld, eqbits);
        __syncthreads();
        if constexpr (CPZ == 2) {
            // The two-chunk controller's cost comes from its definition.  The solves left the constant in their result records and marked them; the products
            // with H are taken here for the workgroup's instances together, on the matrix pipe, by the arithmetic of lmpc_cost_mfma (lmpc_kernels.hip) step for
            // step -- its four wavefronts' shares of the row tiles, its order within a share, its two-level sum over a column's four lanes, its pairing of the
            // four shares -- so that the group form and the two-kernel form return the same bits (tests/test_lmpc_group_head_gpu.py).  A column is an instance
            // and no product mixes columns: what another column holds (an open instance's linear term, an infeasible one's NaNs) reaches nobody's cost.
            // Operands: the solution from the instance's slice (fast_finish put it in f's place, zero from nz on), f from the first product's staging block Bf,
            // which nothing has written since (lane (j, kq) of k-step 4 t + r holds f[16 t + 4 r + kq] of instance j: the layout this sum walks).
            if (M.cost_direct && Bt.n_models <= 0) {
                double *cs = c0s;                    // [4 shares][16 instances]: the head's partials were read in front of its last barrier
                if (wave < 4) {
                    const int ntile = M.nz16 >> 4;
                    const gdp H = GP(H), Hp = GP(Hp);
                    constexpr int kCostGB = 4;
                    double part = 0.0;
                    for (int tl = wave; tl < ntile; tl += 4) {
                        v4d acc = {0.0, 0.0, 0.0, 0.0};
                        auto wop = [&](const int kb) { const int k = 4 * kb + kq; return k < M.nz ? fj[k] : 0.0; };
                        if (Hp) {
                            for (int g0 = 0; g0 < G2; g0 += kCostGB) {
                                v4d a[kCostGB];
#pragma unroll
                                for (int g = 0; g < kCostGB; ++g) if (g0 + g < G2) a[g] = ld4(Hp + (((size_t)tl * G2 + g0 + g) * 64 + lane) * 4);
#pragma unroll
                                for (int g = 0; g < kCostGB; ++g)
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        const int kb = 4 * (g0 + g) + e;
                                        if (kb < nz4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g][e], wop(kb), acc, 0, 0, 0);
                                    }
                            }
                        } else {
                            const int rowa = 16 * tl + j;
                            const gdp Ht = H + (rowa < ldz ? rowa : 0);
                            for (int kb = 0; kb < nz4; ++kb) {
                                const int col = 4 * kb + kq;
                                const double a = (col < M.nz && rowa < ldz) ? Ht[(size_t)col * ldz] : 0.0;
                                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wop(kb), acc, 0, 0, 0);
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * tl + 4 * r + kq;
                            const double w = wop(4 * tl + r);
                            const double fr = row < M.nz ? Bf[(4 * tl + r) * 64 + lane] : 0.0;
                            part = fma(w, 0.5 * acc[r] + fr, part);
                        }
                    }
                    part = wave_sum_rows(part);
                    if (kq == 0) cs[wave * 16 + j] = part;      // one slot per share, added up in a fixed order
                }
                __syncthreads();
                if (threadIdx.x < kGroupWaves) {
                    double *o = outs + threadIdx.x * outld;
                    const int t = threadIdx.x;
                    if (o[7] == 2.0 && o[4] == 1.0) o[0] = ((cs[t] + cs[16 + t]) + (cs[32 + t] + cs[48 + t])) + o[0];
                }
                __syncthreads();
            }
        }
        // the sixteen instances' results, written by neighbouring lanes: one transaction per array and workgroup instead of sixteen
        {
            const int t = threadIdx.x;
            if (t < kGroupWaves && b0 + t < Bt.batch) {
                const double *o = outs + t * outld;
                const int bb = b0 + t;
                if (o[7] == 2.0) {
                    if (Bt.cost) glw(Bt.cost)[bb] = o[0];
                    if (Bt.status) glw(Bt.status)[bb] = (int)o[1];
                    if (Bt.solver_status) glw(Bt.solver_status)[bb] = (int)o[2];
                    if (Bt.is_feasible) glw(Bt.is_feasible)[bb] = (int)o[3];
                    if (Bt.iterations) glw(Bt.iterations)[bb] = 0;
                    if (Bt.polish_rounds) glw(Bt.polish_rounds)[bb] = (int)o[5];
                    if (Bt.active_count) glw(Bt.active_count)[bb] = (int)o[6];
                }
            }
            for (int e = t; e < kGroupWaves * nu; e += blockDim.x) {
                const int ti = e / nu, jj = e - ti * nu;
                if (b0 + ti < Bt.batch && outs[ti * outld + 7] == 2.0) glw(Bt.cmd)[(size_t)(b0 + ti) * nu + jj] = outs[ti * outld + 8 + jj];
            }
            // the instances left open go to the failure queue: one atomic per workgroup that has any, nothing at all otherwise
            if (Bt.fq && t < 64) {
                const bool open = t < kGroupWaves && b0 + t < Bt.batch && outs[t * outld + 7] != 2.0;
                const unsigned long long om = __ballot(open);
                if (om) {
                    int base = 0;
                    if (t == 0) base = atomicAdd(Bt.fq + kFqCount, (int)__builtin_popcountll(om));
                    base = __builtin_amdgcn_readfirstlane(base);
                    const int at = base + (int)__builtin_popcountll(om & ((1ull << t) - 1ull));
                    if (open && at >= 0 && at < Bt.fq_cap) glw(Bt.fq)[kFqList + at] = b0 + t;
                }
            }
        }
    }
}

}  // namespace
size_t lmpc_group_lds_bytes(const LmpcDev &m);
namespace {

template <int CPZ, int CPG>
int launch_fast_variant(const LmpcDev &m, const LmpcDev *m_dev, const LmpcBatchDev &b, double *ws, hipStream_t stream, const LmpcForm form)
{
    size_t ldsf = ((size_t)2 * 128 * CPZ + (size_t)kWavesPerBlock * m.fast_slice + (b.n_models > 0 ? (size_t)kWavesPerBlock * 2 * 128 * CPZ : 0)) * sizeof(double);
    static const size_t dbg_pad = [] { const char *pad = getenv("MPCX_DBG_LDS_PAD"); return pad ? (size_t)atoi(pad) : (size_t)0; }();      // (occupancy experiments; read once)
    ldsf += dbg_pad;
    const size_t lds_max = lmpc_lds_limit();
    if (ldsf > lds_max) return -2;
    auto k2 = lmpc_solve<CPZ, CPG>;
    auto k2h = lmpc_solve_hetero<CPZ, CPG>;
    // the fused forms serve the one-chunk variant only (fused_record: up to 384 rows of the composed map)
    auto k4 = lmpc_solve_fused<1, 1>;
    auto k5 = lmpc_solve_persistent<1, 1>;
    static LmpcLdsCache configured;
    if (lmpc_raise_dynamic_lds(configured, {reinterpret_cast<const void *>(k2), reinterpret_cast<const void *>(k2h), reinterpret_cast<const void *>(k4)}, ldsf) != 0) return -3;
    int blocks = (b.batch + kWavesPerBlock - 1) / kWavesPerBlock;      // one wavefront per instance: the grid covers the batch
    if (blocks < 1) blocks = 1;
    if (form == LmpcForm::Group) {
        if constexpr (CPZ <= 2 && CPZ == CPG) {
            // assemble + solve in one workgroup of sixteen (two-chunk variant: eight) wavefronts, one per CU
            constexpr int NW = kGroupWavesOf<CPZ>;
            const size_t ldsg = lmpc_group_lds_bytes(m);
            if (ldsg == 0 || ldsg > lds_max) return -2;
            static LmpcLdsCache gconf;
            if (lmpc_raise_dynamic_lds(gconf, {reinterpret_cast<const void *>(lmpc_solve_group<CPZ, CPG>)}, lds_max) != 0) return -3;
            const int wgs = (b.batch + NW - 1) / NW;
            hipLaunchKernelGGL((lmpc_solve_group<CPZ, CPG>), dim3(wgs), dim3(NW * 64), ldsg, stream, m, b, ws, b.fused - 3);      // (the model struct by value: see the kernel)
            return hipGetLastError() == hipSuccess ? 0 : -3;
        }
        return -2;      // (no group form for the four-chunk variant: lmpc_group_lds_bytes is 0 there, no plan names it)
    }
    const bool fused = form == LmpcForm::FusedMatvec;
    // persistent form: the composed map, the box bounds and kPersistWaves slices must fit one CU's LDS, and the batch must be worth
    // the prologue of every workgroup (the composed map: 87 KB at N = 20)
    const size_t ldsp = ((size_t)m.rowsF * m.kin + 2 * (size_t)128 + kPersistWaves * (size_t)m.fast_slice) * sizeof(double);
    if (fused && b.pcounter && ldsp <= lds_max && b.batch >= 1024) {
        static LmpcLdsCache pconf;
        if (lmpc_raise_dynamic_lds(pconf, {reinterpret_cast<const void *>(k5)}, lds_max) != 0) return -3;
        (void)hipMemsetAsync(b.pcounter, 0, 8 * sizeof(int), stream);
        int wgs = (b.batch + kPersistWaves - 1) / kPersistWaves;
        if (wgs > 256) wgs = 256;
        hipLaunchKernelGGL(k5, dim3(wgs), dim3(kPersistWaves * 64), ldsp, stream, m_dev, b, ws, b.pcounter);
    } else if (fused) hipLaunchKernelGGL(k4, dim3(blocks), dim3(kWavesPerBlock * 64), ldsf, stream, m_dev, b, ws);
    else if (b.n_models > 0) hipLaunchKernelGGL(k2h, dim3(blocks), dim3(kWavesPerBlock * 64), ldsf, stream, m_dev, b, ws);
    else hipLaunchKernelGGL(k2, dim3(blocks), dim3(kWavesPerBlock * 64), ldsf, stream, m_dev, b, ws);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int lmpc_fast_slice(const LmpcDev &m)
{
    const int cp = lmpc_kernel_variant(m.ldz, m.ldg);
    if (cp < 1) return 0;
    const int fixed = cp == 1 ? fast_slice_fixed<1, 1>() : (cp == 2 ? fast_slice_fixed<2, 2>() : fast_slice_fixed<4, 4>());
    const int scratch = m.kin > 2 * m.nx ? m.kin : 2 * m.nx;    // vin of the fused record / ping-pong state of the sequence roll-out
    int n = (fixed + scratch + 1) / 2 * 2;
    while (n % 16 != 2) n += 2;                                 // slices 2 doubles apart modulo the 32 LDS banks x 4 bytes
    return n;
}

// LDS block of lmpc_solve_group for this controller (0: no group form for its variant): two box-bound vectors, a slice per instance, the staged
// MFMA operands, the cost constants and flags, the result records, the equality flags of the general rows
size_t lmpc_group_lds_bytes(const LmpcDev &m)
{
    const int cp = lmpc_kernel_variant(m.ldz, m.ldg);
    if (cp != 1 && cp != 2) return 0;
    const int nw = cp == 1 ? 16 : 8;
    return ((size_t)2 * 128 * cp + (size_t)nw * m.fast_slice + (size_t)(m.kin / 4 + m.nz16 / 4) * 64 + (size_t)nw * 16 + 16 + (size_t)nw * (8 + ((m.nu + 1) & ~1)) + 32) * sizeof(double);
}

namespace {
// testing aid: one wavefront per vector of 64 values; all 64 lanes of the butterfly's sum, of wave_sum_full's, and of the two forms of the two-level sum
__global__ __launch_bounds__(64) void lmpc_wave_reduce_probe(const double *in, double *out)
{
    const int lane = threadIdx.x;
    const double x = in[(size_t)blockIdx.x * 64 + lane];
    double *o = out + (size_t)blockIdx.x * 256;
    o[lane] = wave_sum(x);
    o[64 + lane] = wave_sum_full(x);
    o[128 + lane] = wave_sum_rows_shfl(x);
    o[192 + lane] = wave_sum_rows_swap(x);
}

// testing aid: ws_solve_reg<CAP, NLO, 1, 1> of the class that na selects (the update's multipliers as the one-chunk product kernels take them), one
// wavefront per problem, with the elimination in form DP.  o [kWsProbeLen]: dep_at, lmax, lam [16], wv of the 64 lanes [128], gw [128]; what a solve that
// ends at a dependent row leaves unwritten stays 0
template <bool DP>
__device__ __forceinline__ void ws_probe_form(const gdp gY, const int ldy, const int ldz, const int na, const int lane, const int *wsidx, const double *wsb,
                                              const double *t0s, double *lam, const unsigned (&boffz)[1], const unsigned (&boffg)[1], double *o)
{
    double wv[2] = {0.0, 0.0}, gw[2] = {0.0, 0.0}, lmax = 0.0;
    int dep_at = -1;
#ifdef MPCX_PROFILE_ROUNDS
    long long pacc[6] = {0, 0, 0, 0, 0, 0}, plast = 0;
#endif
    if (lane < kFastCap + 2) lam[lane] = 0.0;
    wave_sync();
    constexpr auto xl = [](int cap) { return 2 <= MPCX_FAST_LDSMULT_CHUNKS && fast_class_bit(MPCX_FAST_LDSMULT_CLASSES, cap); };
    if (na <= 4) dep_at = ws_solve_reg<4, 1, 1, 1, DP, xl(4)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    else if (na <= 6) dep_at = ws_solve_reg<6, 5, 1, 1, DP, xl(6)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    else if (na <= 8) dep_at = ws_solve_reg<8, 7, 1, 1, DP, xl(8)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    else if (na <= 10) dep_at = ws_solve_reg<10, 9, 1, 1, DP, xl(10)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    else if (na <= 12) dep_at = ws_solve_reg<12, 11, 1, 1, DP, xl(12)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    else if (na <= 14) dep_at = ws_solve_reg<14, 13, 1, 1, DP, xl(14)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    else dep_at = ws_solve_reg<kFastCap, 15, 1, 1, DP, xl(kFastCap)>(gY, ldy, ldz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, wv, gw, lmax MPCX_PROF_PASS);
    wave_sync();
    if (lane == 0) { o[0] = (double)dep_at; o[1] = lmax; }
    if (lane < kFastCap) o[2 + lane] = lam[lane];
    o[2 + kFastCap + 2 * lane] = wv[0]; o[2 + kFastCap + 2 * lane + 1] = wv[1];
    o[2 + kFastCap + 128 + 2 * lane] = gw[0]; o[2 + kFastCap + 128 + 2 * lane + 1] = gw[1];
    wave_sync();
}
// problem p = blockIdx.x: Y + p n ldy (symmetric, n x n, rows 0 .. nz - 1 the z rows and the rest the general rows of the unified index), wsidx / wsb + 16 p,
// na[p], t0 + p n = [t0 | G t0] by unified index.  Indices are clamped to the matrix, a problem whose na is not in 1 .. 16 is left alone.
__global__ __launch_bounds__(64) void lmpc_ws_solve_probe(const double *Y, const int n, const int ldy, const int nz, const int *wsidx_in, const double *wsb_in,
                                                          const int *na_in, const double *t0_in, double *out)
{
    __shared__ double t0s[256], lam[kFastCap + 2], wsb[kFastCap + 2];
    __shared__ int wsidx[kFastCap + 2];
    const int lane = threadIdx.x, p = blockIdx.x;
    const int na = __builtin_amdgcn_readfirstlane(na_in[p]);
    if (na < 1 || na > kFastCap) return;
    const int ng = n - nz;
    for (int e = lane; e < 256; e += 64) t0s[e] = e < nz ? t0_in[(size_t)p * n + e] : (e >= 128 && e - 128 < ng ? t0_in[(size_t)p * n + nz + e - 128] : 0.0);
    if (lane < kFastCap + 2) {
        const int q = lane < kFastCap ? wsidx_in[(size_t)p * kFastCap + lane] : 0;
        wsidx[lane] = q < 0 ? 0 : (q < n ? q : n - 1);
        wsb[lane] = lane < kFastCap ? wsb_in[(size_t)p * kFastCap + lane] : 0.0;
    }
    wave_sync();
    const unsigned boffz[1] = {(unsigned)(2 * lane < nz ? 2 * lane : 0) * 8u}, boffg[1] = {(unsigned)(nz + (2 * lane < ng ? 2 * lane : 0)) * 8u};
    const gdp gY = gl(Y + (size_t)p * n * ldy);
    double *o = out + (size_t)p * 2 * kWsProbeLen;
    ws_probe_form<false>(gY, ldy, nz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, o);
    ws_probe_form<true>(gY, ldy, nz, na, lane, wsidx, wsb, t0s, lam, boffz, boffg, o + kWsProbeLen);
}
}  // namespace

int lmpc_debug_ws_solve(const double *Y, int n, int ldy, int nz, const int *wsidx, const double *wsb, const int *na, const double *t0, double *out, int count,
                        void *stream)
{
    // one chunk: at most 128 z rows and 128 general rows, at least one lane pair of each (a lane without a pair re-reads pair 0), a row of Y in whole pairs
    if (n < 4 || nz < 2 || n - nz < 2 || nz > 128 || n - nz > 128 || nz % 2 != 0 || (n - nz) % 2 != 0 || ldy < n || ldy % 2 != 0) return -2;
    if (count <= 0) return 0;
    hipLaunchKernelGGL(lmpc_ws_solve_probe, dim3(count), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), Y, n, ldy, nz, wsidx, wsb, na, t0, out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int lmpc_debug_wave_reduce(const double *in, double *out, int nvec, void *stream)
{
    if (nvec <= 0) return 0;
    hipLaunchKernelGGL(lmpc_wave_reduce_probe, dim3(nvec), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), in, out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int lmpc_launch_fast(const LmpcDev &m, const LmpcDev *m_dev, const LmpcBatchDev &b, double *ws, void *stream, LmpcForm form)
{
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (lmpc_kernel_variant(m.ldz, m.ldg)) {
    case 1: return launch_fast_variant<1, 1>(m, m_dev, b, ws, s, form);
#ifndef MPCX_FAST_ONLY_CP1
    case 2: return launch_fast_variant<2, 2>(m, m_dev, b, ws, s, form);
    case 4: return launch_fast_variant<4, 4>(m, m_dev, b, ws, s, form);
#endif
    default: return -2;
    }
}

}  // namespace mpcx
