// What the two LMPC solve kernels -- the lean kernels of lmpc_fast.hip (solve_fast, fast_finish) and the ADMM fallback of lmpc_kernels.hip
// (admm_solve_one) -- do outside their rounds: the front end that reads the reference's constraint numbering, the back end that writes the
// reference's result layout.  A kind of row is wired into the warm start and the active bits here, once.  The rounds themselves are each kernel's own.
#pragma once
#include "lmpc_kernel_common.hpp"

namespace mpcx {

namespace {

// Warm start: the first working set is the previous solve's active set, bits over the reference's rows (ProblemBuilder.hpp:814-822:
// equalities | box on [x; x_u] | outputs | delta-u | scalar | linear).  With warm_shift the row looked up is the same constraint one step later:
// the previous tick's step i+1 is this tick's step i.  The callers walk their lanes' slots, skip the equality rows and pass the bound values in.
struct WarmStart {
    const LmpcDev &M;
    const unsigned MPCX_GAS *wl, *wu;
    const bool shift;
    int na, n1, b_out, b_du, b_sc;        // rows of one step's box block, steps, where the output / delta-u / scalar blocks start
    __device__ __forceinline__ WarmStart(const LmpcDev &M_, const LmpcBatchDev &Bt, const int b)
        : M(M_), wl(gl(Bt.warm_lower) + (size_t)b * M_.active_words), wu(gl(Bt.warm_upper) + (size_t)b * M_.active_words), shift(Bt.warm_shift)
    {
        na = M.nx + M.nu; n1 = M.ph + 1;
        const int b_box = M.neq_ref;
        b_out = b_box + n1 * na; b_du = b_out + n1 * M.ny; b_sc = b_du + M.ph * M.nu;
    }
    __device__ __forceinline__ int look(int rr) const
    {
        if (!shift) return rr;
        if (rr < b_out) return rr + na < b_out ? rr + na : rr;
        if (rr < b_du) return rr + M.ny < b_du ? rr + M.ny : rr;
        if (rr < b_sc) return rr + M.nu < b_sc ? rr + M.nu : rr;
        const int sh = rr < b_sc + n1 ? 1 : MPCX_LINEAR_NC(M);      // (a linear row, DESIGN.md 3.4: the same row one step later is nc rows on)
        return rr + sh < M.m_ref ? rr + sh : rr;
    }
    // -1 / 0 / +1: box variable e, whose bounds are lo and hi now, starts at its lower / at no / at its upper bound (a reference row counts where
    // its own bound is the binding one)
    __device__ __forceinline__ int box_side(int e, double lo, double hi) const
    {
        int side = 0;
        for (int p = GP(boxrow_ptr)[e]; p < GP(boxrow_ptr)[e + 1]; ++p) {
            const int rr = look(GP(boxrow_ref)[p]);
            if (((wl[rr >> 5] >> (rr & 31)) & 1u) && GP(boxrow_lo)[p] == lo) side = -1;
            if (((wu[rr >> 5] >> (rr & 31)) & 1u) && GP(boxrow_hi)[p] == hi) side = 1;
        }
        return side;
    }
    // the same for general row r
    __device__ __forceinline__ int row_side(int r) const
    {
        const int rr = look(GP(g_refrow)[r]);
        return ((wl[rr >> 5] >> (rr & 31)) & 1u) ? -1 : (((wu[rr >> 5] >> (rr & 31)) & 1u) ? 1 : 0);
    }
};

// Active bits over the reference's rows: assembled in LDS (2 active_words words at `buf`, which the caller no longer needs), written out as whole
// words.  Which side of a row is active is the caller's rule.
struct ActiveBits {
    const LmpcDev &M;
    unsigned *bl, *bu;
    __device__ __forceinline__ ActiveBits(const LmpcDev &M_, double *buf, const int lane) : M(M_), bl(reinterpret_cast<unsigned *>(buf)), bu(bl + M_.active_words)
    {
        wave_sync();
        for (int wd = lane; wd < 2 * M.active_words; wd += 64) bl[wd] = 0u;
        wave_sync();
    }
    // box variable e at its lower (side < 0) or upper (side > 0) bound lo / hi: every reference row whose own bound is that one
    __device__ __forceinline__ void mark_box(int e, int side, double lo, double hi) const
    {
        for (int p = GP(boxrow_ptr)[e]; p < GP(boxrow_ptr)[e + 1]; ++p) {
            const int rr = GP(boxrow_ref)[p];
            if (side < 0 && GP(boxrow_lo)[p] == lo) atomicOr(&bl[rr >> 5], 1u << (rr & 31));
            if (side > 0 && GP(boxrow_hi)[p] == hi) atomicOr(&bu[rr >> 5], 1u << (rr & 31));
        }
    }
    __device__ __forceinline__ void mark_row(int r, int side) const
    {
        const int rr = GP(g_refrow)[r];
        if (side < 0) atomicOr(&bl[rr >> 5], 1u << (rr & 31));
        else atomicOr(&bu[rr >> 5], 1u << (rr & 31));
    }
    __device__ __forceinline__ void store(const LmpcBatchDev &Bt, const int b, const int lane) const
    {
        wave_sync();
        for (int wd = lane; wd < M.active_words; wd += 64) {
            glw(Bt.active_lower)[(size_t)b * M.active_words + wd] = bl[wd];
            glw(Bt.active_upper)[(size_t)b * M.active_words + wd] = bu[wd];
        }
        wave_sync();
    }
};

// OptSequence (LOptimizer.hpp:305-338): roll the model forward with the optimal inputs, staged in `stage`; xs holds 2 nx doubles
__device__ __forceinline__ void sequence_rollout(const LmpcDev &M, const LmpcBatchDev &Bt, const int b, const int lane, const double *stage, double *xs,
                                                 const bool infeasible)
{
    if (!(Bt.seq_state || Bt.seq_input || Bt.seq_output)) return;
    wave_sync();
    const int nx = M.nx, nu = M.nu, ny = M.ny, ndu = M.ndu, ph = M.ph;
    const gdp gA = GP(A), gB = GP(B), gC = GP(C), gBd = GP(Bd), gDd = GP(Dd), gdm = gl(Bt.dmeas ? Bt.dmeas : M.dmeas_s);
    const gip gblk = GP(blk);
    auto dm = [&](int k, int dd) -> double { return ref_at(gdm, Bt.dmeas_bs, Bt.dmeas_ks, b, k, dd); };
    double *xs0 = xs, *xs1 = xs + nx;      // ping-pong state
    if (lane < nx) xs0[lane] = infeasible ? __builtin_nan("") : gl(Bt.x0)[(size_t)b * nx + lane];
    wave_sync();
    for (int i = 0; i <= ph; ++i) {
        const double *xc = (i & 1) ? xs1 : xs0;
        double *xn = (i & 1) ? xs0 : xs1;
        const int k = i > 0 ? i - 1 : 0;
        if (Bt.seq_state && lane < nx) glw(Bt.seq_state)[((size_t)b * (ph + 1) + i) * nx + lane] = xc[lane];
        if (Bt.seq_input && lane < nu) {
            const int ii = (i + 1 <= ph) ? i + 1 : ph;
            glw(Bt.seq_input)[((size_t)b * (ph + 1) + i) * nu + lane] = stage[gblk[ii] * nu + lane];
        }
        if (Bt.seq_output && lane < ny) {
            double yv = 0;
            for (int c = 0; c < nx; ++c) yv = fma(gC[lane + c * ny], xc[c], yv);
            if (M.has_dist) for (int dd = 0; dd < ndu; ++dd) yv = fma(gDd[lane + dd * ny], dm(k, dd), yv);
            glw(Bt.seq_output)[((size_t)b * (ph + 1) + i) * ny + lane] = yv;
        }
        if (i < ph && lane < nx) {
            double s = 0;
            for (int c = 0; c < nx; ++c) s = fma(gA[lane + c * nx], xc[c], s);
            for (int c = 0; c < nu; ++c) s = fma(gB[lane + c * nx], stage[gblk[i + 1] * nu + c], s);
            if (M.has_dist) for (int dd = 0; dd < ndu; ++dd) s = fma(gBd[lane + dd * nx], dm(i, dd), s);
            xn[lane] = s;
        }
        wave_sync();
    }
}

// The scalar results.  The solver's status (OSQP's numbering: 1 solved, 2 solved inaccurate, -2 iterations ran out, -3 infeasible) as the reference's
// status and feasibility flag (LOptimizer.hpp:386-415)
__device__ __forceinline__ int ref_status(int solver_status)
{
    return (solver_status == 1 || solver_status == 2) ? 0 : (solver_status == -2 ? 1 : (solver_status == -3 ? 2 : 4));
}
__device__ __forceinline__ int ref_feasible(int solver_status) { return (solver_status == 1 || solver_status == 2 || solver_status == -2) ? 1 : 0; }
// one lane writes instance b's record (with_cost false: another kernel writes the cost)
__device__ __forceinline__ void store_scalars(const LmpcBatchDev &Bt, const int b, bool with_cost, double cost, int solver_status, int iterations, int rounds, int active)
{
    if (Bt.cost && with_cost) glw(Bt.cost)[b] = cost;
    if (Bt.solver_status) glw(Bt.solver_status)[b] = solver_status;
    if (Bt.status) glw(Bt.status)[b] = ref_status(solver_status);
    if (Bt.is_feasible) glw(Bt.is_feasible)[b] = ref_feasible(solver_status);
    if (Bt.iterations) glw(Bt.iterations)[b] = iterations;
    if (Bt.polish_rounds) glw(Bt.polish_rounds)[b] = rounds;
    if (Bt.active_count) glw(Bt.active_count)[b] = active;
}

// A linearly dependent working set: row q (unified index: box rows, then ldz + general row) leaves it
template <int NZS, int NGS>
__device__ __forceinline__ void row_leaves(const int q, const int ldz, const int lane, int (&actb)[NZS], int (&actg)[NGS])
{
#pragma unroll
    for (int s = 0; s < NZS; ++s)
        if (128 * (s >> 1) + 2 * lane + (s & 1) == q) actb[s] = 0;
#pragma unroll
    for (int s = 0; s < NGS; ++s)
        if (ldz + 128 * (s >> 1) + 2 * lane + (s & 1) == q) actg[s] = 0;
}

}  // namespace

}  // namespace mpcx
