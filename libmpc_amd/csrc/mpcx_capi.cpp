// extern "C" boundary of the batched LMPC engine (include/mpcx.h).
// Host code only: owns the controller state, runs the one-time condensing, keeps the
// condensed model resident in HBM, and launches the HIP kernel.  There is no CPU solve
// path here: without a usable HIP device every solve call fails with MPCX_E_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/mpcx.h"
#include "lmpc_device.hpp"
#include "lmpc_model.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

}  // namespace

namespace mpcx {
int capi_fail(int code, const std::string &msg) { return fail(code, msg); }   // shared with nlmpc_capi.cpp
}

struct mpcx_lmpc {
    mpcx::LmpcController ctl;
    int device = 0;
    bool host_only = false;
    bool dirty = true;                  // controller changed: condense again, rebuild the device-resident model
    bool refs_dirty = false;            // only references / exogenous inputs changed: refresh what depends on them, in place
    mpcx::Condensed cond;
    mpcx::LmpcDev dev{};
    mpcx::LmpcDev *dev_d = nullptr;     // the same struct, resident in HBM for the kernel
    std::vector<void *> allocs;
    long long *dbg_cycles = nullptr;
    bool force_generic = false;
    bool strict_infeasible = false;
    int dbg_rounds0 = 30, dbg_check_every = 10;      // experiment knobs (mpcx_lmpc_debug_set_rounds)
    // Fused forms (lmpc_solve_fused / lmpc_solve_persistent): the instance's record is computed inside the solve kernel instead of
    // being handed over through the HBM workspace (3 MB instead of 25 MB of traffic per 4096 instances), but the hardest-first
    // dispatch order of the two-kernel path is lost -- worth 22 us of its 70 us at 4096 instances, nothing at large batches.
    // Measured (quadrotor N = 20, ms per step, two kernels / fused): 4096: 0.097 / 0.125; 16384: 0.309 / 0.300; 65536: 1.10 / 1.00.
    // -1 = automatic (lmpc_solve_group up to group_max instances, assemble + solve as two kernels beyond; the fused / persistent mat-vec forms
    // only on request), 0 = always two kernels, 1 = the fused form wherever the dimensions allow, 2 = the group form (mpcx_lmpc_debug_use_fused)
    int use_fused = -1;
    int group_max = 4096;               // automatic mode: batches up to this size take lmpc_solve_group (assemble + solve in one workgroup)
    int total_batch = 0;                // mpcx_lmpc_set_total_batch: this handle solves shards of a batch of that size (0: every call is a whole batch)
    // staging of mpcx_lmpc_solve_host (kept between calls) and the active sets it carries from one call to the next
    double *stage_d = nullptr; int32_t *stage_i = nullptr; uint32_t *stage_act = nullptr;
    size_t stage_cap = 0;               // instances
    int warm_batch = 0;                 // batch size whose active sets are in stage_act (0: none)
    int n_full_setups = 0, n_ref_refreshes = 0;      // how often each kind of set-up ran (mpcx_lmpc_debug_setup_counts)
    mpcx::LmpcScratch scratch{};        // workspace, failure queue, large-working-set slots, persistent kernel's counters (lmpc_device.hpp)
    const double *sens_t0p = nullptr;   // the sensitivity kernel's shared MFMA operand (lmpc_sens_operand), uploaded with the model
    double *sens_stage = nullptr; size_t sens_stage_cap = 0;      // outputs of mpcx_lmpc_sensitivity_host on the device (kept between calls), instances
    int sens_batch = 0;                 // batch size of the last mpcx_lmpc_solve_host whose active sets and status are still in the staging buffers (0: none)
    // parameter sensitivities (lmpc_param_sens.hip): Cq on the host and packed on the device, built at first use after a set-up; the partials of the
    // batch reduction (mpcx_lmpc_param_sens_reserve; grow-only); the host form's outputs on the device; whether the last mpcx_lmpc_solve_host kept its sequences
    std::vector<double> param_cq; const double *param_cqp = nullptr;
    double *param_part = nullptr; size_t param_part_cap = 0;
    double *param_stage = nullptr; size_t param_stage_cap = 0;      // (capacity in doubles: a set-up may change m_ref, and with it the length per instance)
    bool sens_has_seq = false;
    // model sensitivities (lmpc_model_sens.hip): Xq likewise, built by mpcx_lmpc_model_sens_reserve or the first launch after a set-up -- a controller
    // that never asks pays nothing; its partials and the host form's staging
    std::vector<double> model_xq; const double *model_xqp = nullptr;
    double *model_part = nullptr; size_t model_part_cap = 0;
    double *model_stage = nullptr; size_t model_stage_cap = 0;
    int solved_full = -1, solved_refs = -1;          // n_full_setups / n_ref_refreshes when mpcx_lmpc_solve_batch last launched: the set-up a solved batch belongs to
    explicit mpcx_lmpc(const mpcx_dims &d) : ctl(d) {}

    void release()
    {
        for (void *p : allocs) (void)hipFree(p);
        allocs.clear();
        mpcx::lmpc_scratch_release(scratch);
        warm_batch = 0;                 // row numbering may have changed with the model
        sens_batch = 0;
        param_cqp = nullptr;            // (it was one of allocs)
        model_xqp = nullptr;
    }
    void release_staging()
    {
        if (stage_d) (void)hipFree(stage_d);
        if (stage_i) (void)hipFree(stage_i);
        if (stage_act) (void)hipFree(stage_act);
        if (sens_stage) (void)hipFree(sens_stage);
        if (param_stage) (void)hipFree(param_stage);
        if (param_part) (void)hipFree(param_part);
        param_stage = nullptr; param_stage_cap = 0; param_part = nullptr; param_part_cap = 0;
        if (model_stage) (void)hipFree(model_stage);
        if (model_part) (void)hipFree(model_part);
        model_stage = nullptr; model_stage_cap = 0; model_part = nullptr; model_part_cap = 0;
        stage_d = nullptr; stage_i = nullptr; stage_act = nullptr; stage_cap = 0; warm_batch = 0;
        sens_stage = nullptr; sens_stage_cap = 0; sens_batch = 0;
    }
    // copy into a buffer this handle already owns on the device (same size as at set-up)
    template <typename T>
    bool reup(const T *dst, const std::vector<T> &v)
    {
        return v.empty() || hipMemcpy(const_cast<T *>(dst), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    }
    // the O(n^3) arrays (H, Kinv, Gr, Gc, Y): for a single controller they are uploaded like everything else
    template <typename T> const T *up_big(const std::vector<T> &v, int &rc) { return up(v, rc); }
    const double *reserve_big(size_t) { return nullptr; }         // (banks only)
    template <typename T>
    const T *up(const std::vector<T> &v, int &rc)
    {
        size_t n = v.size() ? v.size() : 1;
        void *p = nullptr;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) { rc = MPCX_E_DEVICE; return nullptr; }
        allocs.push_back(p);
        if (v.size() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) rc = MPCX_E_DEVICE;
        return static_cast<const T *>(p);
    }
};

// The device view of one condensed controller: scalars ...
static void fill_dev_scalars(const mpcx_lmpc *h, const mpcx::LmpcController &c, const mpcx::Condensed &o, mpcx::LmpcDev &D)
{
    D = mpcx::LmpcDev{};
    D.nx = c.d.nx; D.nu = c.d.nu; D.ndu = c.d.ndu; D.ny = c.d.ny; D.ph = c.d.ph; D.ch = c.d.ch;
    D.nf = o.nf; D.nz = o.nz; D.mg = o.mg; D.ldz = o.ldz; D.ldg = o.ldg; D.ldy = o.ldy;
    D.m_ref = o.m_ref; D.neq_ref = o.neq_ref; D.active_words = o.active_words;
    D.has_dist = o.has_dist ? 1 : 0;
    D.n_fixed = (int)o.fixed_rows.size();
    D.n_soft = o.n_soft;                 // (before lmpc_lds_per_wave: the working-set lists are sized by it)
    D.max_iter = c.prm.maximum_iteration; D.polish = c.prm.polish ? 1 : 0;
    D.strict_infeasible = h->strict_infeasible ? 1 : 0;
    D.cost_direct = (o.h_regularised || o.inverse_residual > 1e-9) ? 1 : 0;
    D.check_every = h->dbg_check_every; D.polish_rounds0 = h->dbg_rounds0; D.polish_rounds = 10;
    D.alpha = c.prm.alpha; D.sigma = 1e-6;
    D.adaptive_rho = (c.prm.adaptive_rho ? 1 : 0) | (c.have_terminal ? 2 : 0) | (c.linear_rows_live() << 2); D.rho_user = c.prm.rho;      // (a flag word: MPCX_HAS_TERMINAL, MPCX_LINEAR_NC, before lmpc_lds_per_wave)
    D.eps_abs = c.prm.eps_abs; D.eps_rel = c.prm.eps_rel; D.eps_prim_inf = c.prm.eps_prim_inf;
    D.lds_per_wave = mpcx::lmpc_lds_per_wave(D, &D.stage_len, &D.arena_len);
    D.wsld = D.ldz + D.ldy + 2 * D.ldg + 2;
    // (a soft step-0 row is a general row, not a feasibility condition: Condensed::g_soft)
    const bool soft0 = std::isfinite(c.softS[0]);
    D.s0lo = soft0 ? -mpcx::kInf : c.sMin[0]; D.s0hi = soft0 ? mpcx::kInf : c.sMax[0];
}

// ... and arrays, through an uploader (one hipMalloc per array for a single controller, offsets into one slab for a bank of them)
template <class Uploader>
static void fill_dev_arrays(const mpcx_lmpc *h, const mpcx::LmpcController &c, const mpcx::Condensed &o, mpcx::LmpcDev &D, Uploader &U, int &rc)
{
    D.A = U.up(c.A.a, rc); D.B = U.up(c.B.a, rc); D.C = U.up(c.C.a, rc);
    D.Bd = U.up(c.Bd.a, rc); D.Dd = U.up(c.Dd.a, rc);
    {
        // the terminal cost's [P | xT | Tx] rides behind the output weights (MPCX_TERMINAL)
        std::vector<double> wy(c.wOutput.a);
        const std::vector<double> term = c.terminal_block();
        wy.insert(wy.end(), term.begin(), term.end());
        D.Wy = U.up(wy, rc);
    }
    D.Wu = U.up(c.wU.a, rc); D.Wdu = U.up(c.wDeltaU.a, rc);
    D.yref_s = U.up(c.yRef.a, rc); D.uref_s = U.up(c.uRef.a, rc);
    D.duref_s = U.up(c.duRef.a, rc); D.dmeas_s = U.up(c.dMeas.a, rc);
    {
        std::vector<double> lo0x(c.d.nx), hi0x(c.d.nx), lo0u(c.d.nu), hi0u(c.d.nu), lo0y(c.d.ny), hi0y(c.d.ny);
        for (int j = 0; j < c.d.nx; j++) { const bool soft = std::isfinite(c.softX(j, 0)); lo0x[j] = soft ? -mpcx::kInf : c.minX(j, 0); hi0x[j] = soft ? mpcx::kInf : c.maxX(j, 0); }
        for (int j = 0; j < c.d.nu; j++) { lo0u[j] = c.minU(j, 0); hi0u[j] = c.maxU(j, 0); }
        for (int j = 0; j < c.d.ny; j++) { const bool soft = std::isfinite(c.softY(j, 0)); lo0y[j] = soft ? -mpcx::kInf : c.minY(j, 0); hi0y[j] = soft ? mpcx::kInf : c.maxY(j, 0); }
        D.lo0x = U.up(lo0x, rc); D.hi0x = U.up(hi0x, rc); D.lo0u = U.up(lo0u, rc); D.hi0u = U.up(hi0u, rc);
        D.lo0y = U.up(lo0y, rc); D.hi0y = U.up(hi0y, rc);
        D.sX = U.up(c.scalar_linear_block(), rc); D.sU = U.up(c.sU, rc);      // (the linear rows' coefficients ride behind sX: MPCX_LINEAR_F)
    }
    if (o.big_n[0]) {          // structure-only condensing: room for what the device kernel computes
        D.H = U.reserve_big(o.big_n[0]); D.Kinv = U.reserve_big(o.big_n[1]); D.Gr = U.reserve_big(o.big_n[2]); D.Gc = U.reserve_big(o.big_n[3]); D.Y = U.reserve_big(o.big_n[4]);
    } else {
        D.H = U.up_big(o.H, rc); D.Kinv = U.up_big(o.Kinv, rc); D.Gr = U.up_big(o.Gr, rc); D.Gc = U.up_big(o.Gc, rc); D.Y = U.up_big(o.Y, rc);
    }
    D.lw = U.up(o.lw, rc); D.uw = U.up(o.uw, rc); D.rho_b = U.up(o.rho_b, rc);
    D.lg0 = U.up(o.lg0, rc); D.ug0 = U.up(o.ug0, rc); D.rho_g = U.up(o.rho_g_device(), rc);
    D.g_kind = U.up(o.g_kind, rc); D.g_step = U.up(o.g_step, rc); D.g_comp = U.up(o.g_comp, rc); D.g_refrow = U.up(o.g_refrow, rc);
    {
        std::vector<int> fk, fs, fc; std::vector<double> fl, fh;
        for (auto &r : o.fixed_rows) { fk.push_back(r.kind); fs.push_back(r.step); fc.push_back(r.comp); fl.push_back(r.lo); fh.push_back(r.hi); }
        D.f_kind = U.up(fk, rc); D.f_step = U.up(fs, rc); D.f_comp = U.up(fc, rc); D.f_lo = U.up(fl, rc); D.f_hi = U.up(fh, rc);
    }
    D.boxrow_ptr = U.up(o.boxrow_ptr, rc); D.boxrow_ref = U.up(o.boxrow_ref, rc);
    D.boxrow_lo = U.up(o.boxrow_lo, rc); D.boxrow_hi = U.up(o.boxrow_hi, rc);
    D.blk = U.up(o.blk, rc);
    D.kin = o.kin; D.nxp = o.nxp; D.nup = o.nup; D.nyp = o.nyp; D.ione = o.ione;
    D.nz16 = o.nz16; D.mg16 = o.mg16; D.ns = o.ns; D.ns16 = o.ns16; D.kq16 = o.kq16; D.rowsA = o.rowsA; D.ldy16 = o.ldy16;
    D.fast_slice = mpcx::lmpc_fast_slice(D);
    D.MA0 = U.up(o.MA[0], rc); D.MA1 = U.up(o.MA[1], rc); D.Ym = U.up(o.Ym, rc);
    {
        std::vector<double> pk;
        auto packed = [&](const std::vector<double> &v, int rows, int K) -> const std::vector<double> & {
            pk.clear();
            if (!v.empty()) { pk.resize(mpcx::lmpc_packed_len(rows, K)); mpcx::lmpc_pack_mfma_tiles(v.data(), rows, K, pk.data()); }
            return pk;
        };
        D.MA0p = U.up(packed(o.MA[0], o.rowsA, o.kin), rc); D.MA1p = U.up(packed(o.MA[1], o.rowsA, o.kin), rc); D.Ymp = U.up(packed(o.Ym, o.ldy16, o.nz16), rc);
        std::vector<double> hpad;
        if (D.cost_direct && !o.MA[0].empty() && !o.H.empty()) {          // (a controller that takes lmpc_cost_mfma: the shared-model path with the cost from its definition)
            hpad.assign((size_t)o.nz16 * o.nz16, 0.0);
            for (int c = 0; c < o.nz; ++c)
                for (int r = 0; r < o.nz; ++r) hpad[(size_t)c * o.nz16 + r] = o.H[(size_t)c * o.ldz + r];
        }
        D.Hp = hpad.empty() ? nullptr : U.up(packed(hpad, o.nz16, o.nz16), rc);
    }
    D.MF0 = U.up(o.MF[0], rc); D.MF1 = U.up(o.MF[1], rc); D.rowsF = o.rowsF; D.nsp = o.nsp;
    // the fused kernel serves the one-chunk variant while the composed map stays small enough to stream from L2 per instance
    // (and the cost comes from the multipliers: otherwise the two-kernel path's batched cost kernel is the better one)
    D.fused_ok = (h->use_fused != 0 && mpcx::lmpc_kernel_variant(o.ldz, o.ldg) == 1 && o.rowsF <= 384 && !D.cost_direct) ? 1 : 0;
    // assemble + solve in one workgroup (lmpc_solve_group): the one-chunk variant, cost from the multipliers
    // lmpc_solve_group's LDS block: two box-bound vectors, sixteen per-instance slices, the staged operands, the result records -- one CU's worth at most
    // (otherwise the two-kernel path, which handled such a controller before the group form existed, takes it)
    // Round 5: the two-chunk variant as well (config 4's N = 50: eight instances per workgroup, the cost from its definition inside the solve);
    // there it is taken on request only (mpcx_lmpc_debug_use_fused(h, 2)): measured no faster than the two-kernel path
    const size_t ldsg = mpcx::lmpc_group_lds_bytes(D);
    const int cpv = mpcx::lmpc_kernel_variant(o.ldz, o.ldg);
    D.group_ok = (h->use_fused != 0 && ldsg > 0 && ldsg <= mpcx::lmpc_lds_limit() && ((cpv == 1 && !D.cost_direct) || (cpv == 2 && h->use_fused == 2))) ? 1 : 0;
    D.slo = U.up(o.slo, rc); D.shi = U.up(o.shi, rc);
}

// ---- heterogeneous batches: a bank of controllers solved together -------------------------------------------------------------
// In the reference every controller object owns its model (LMPC.hpp:751; ProblemBuilder.hpp:184-211 rebuilds the QP from it,
// :642-825).  A bank is K such objects -- same dimensions, same pattern of finite bounds, otherwise free: own A, B, C, weights,
// bounds, references, parameters -- condensed on the host cores in parallel and kept in one slab of HBM as K device structs; the
// kernels pick the struct of each instance (lmpc_model_of).  Per-model factors cannot be shared through L2: the assemble kernel
// reads its model's -Hinv and G Hinv once per instance, the solve the rows of Y in the working set -- this path is HBM-bound.
struct SlabUploader {
    static constexpr size_t kDevRegion = (size_t)1 << 44; // offsets from here on: the device-only region
    std::vector<char> host;                      // staging image of the uploaded region
    size_t dev_bytes = 0;                        // device-only region: arrays the condensing kernel fills (zeroed on the device, never staged)
    bool big_on_device = false;
    template <typename T>
    const T *up(const std::vector<T> &v, int &)
    {
        const size_t at = (host.size() + 15) / 16 * 16;
        host.resize(at + (v.size() ? v.size() : 1) * sizeof(T), 0);
        if (v.size()) std::memcpy(host.data() + at, v.data(), v.size() * sizeof(T));
        return reinterpret_cast<const T *>(at + 1);          // offset + 1 (so that offset 0 is not a null pointer); rebased below
    }
    const double *reserve_big(size_t n)
    {
        const size_t at = (dev_bytes + 15) / 16 * 16;
        dev_bytes = at + (n ? n : 1) * sizeof(double);
        return reinterpret_cast<const double *>(kDevRegion + at + 1);
    }
    template <typename T>
    const T *up_big(const std::vector<T> &v, int &rc)
    {
        if (!big_on_device) return up(v, rc);
        return reinterpret_cast<const T *>(reserve_big(v.size()));
    }
};

struct mpcx_lmpc_hetero {
    int device = 0, count = 0;
    mpcx_dims d{};
    mpcx::LmpcDev dev0{};                        // model 0 with device pointers (dimensions, LDS plan)
    mpcx::LmpcDev *models_d = nullptr;           // [count] device structs
    char *slab = nullptr, *slab_dev = nullptr;     // uploaded arrays / arrays the condensing kernel fills
    mpcx::LmpcScratch scratch{};                 // as mpcx_lmpc's, without the counters
    int active_words = 0, m_ref = 0;
    bool condensed_on_device = false;
    float setup_kernel_ms = 0, setup_total_ms = 0;   // the condensing kernel alone / the whole mpcx_lmpc_hetero_create
    double setup_flops = 0;                          // per controller (the host set-up's count)
    ~mpcx_lmpc_hetero()
    {
        if (models_d) (void)hipFree(models_d);
        if (slab) (void)hipFree(slab);
        if (slab_dev) (void)hipFree(slab_dev);
        mpcx::lmpc_scratch_release(scratch);
    }
};

static void rebase_dev(mpcx::LmpcDev &D, const char *base, const char *base_dev)
{
    // every pointer member was filled with (offset + 1) by SlabUploader: turn it into base + offset (of its region)
    auto fix = [&](auto &p) {
        using P = std::remove_reference_t<decltype(p)>;
        if (!p) return;
        const size_t off = reinterpret_cast<size_t>(p) - 1;
        p = off >= SlabUploader::kDevRegion ? reinterpret_cast<P>(base_dev + (off - SlabUploader::kDevRegion)) : reinterpret_cast<P>(base + off);
    };
    fix(D.A); fix(D.B); fix(D.C); fix(D.Bd); fix(D.Dd); fix(D.Wy); fix(D.Wu); fix(D.Wdu);
    fix(D.yref_s); fix(D.uref_s); fix(D.duref_s); fix(D.dmeas_s);
    fix(D.lo0x); fix(D.hi0x); fix(D.lo0u); fix(D.hi0u); fix(D.lo0y); fix(D.hi0y); fix(D.sX); fix(D.sU);
    fix(D.H); fix(D.Kinv); fix(D.Gr); fix(D.Gc); fix(D.Y); fix(D.lw); fix(D.uw); fix(D.rho_b); fix(D.lg0); fix(D.ug0); fix(D.rho_g);
    fix(D.g_kind); fix(D.g_step); fix(D.g_comp); fix(D.g_refrow);
    fix(D.f_kind); fix(D.f_step); fix(D.f_comp); fix(D.f_lo); fix(D.f_hi);
    fix(D.boxrow_ptr); fix(D.boxrow_ref); fix(D.boxrow_lo); fix(D.boxrow_hi); fix(D.blk);
    fix(D.MA0); fix(D.MA1); fix(D.Ym); fix(D.MA0p); fix(D.MA1p); fix(D.Ymp); fix(D.Hp); fix(D.slo); fix(D.shi); fix(D.MF0); fix(D.MF1);
}

extern "C" {

const char *mpcx_version(void) { return "mpcx 0.1.0 (gfx950)"; }
const char *mpcx_last_error(void) { return g_err.c_str(); }

void mpcx_lparams_default(mpcx_lparams *p)
{
    // mpc::LParameters defaults, reference include/mpc/Types.hpp:108-114,150-160
    p->maximum_iteration = 100; p->time_limit = 0; p->enable_warm_start = 0;
    p->alpha = 1.6; p->rho = 1e-6; p->eps_rel = 1e-4; p->eps_abs = 1e-4;
    p->eps_prim_inf = 1e-3; p->eps_dual_inf = 1e-3;
    p->verbose = 0; p->adaptive_rho = 1; p->polish = 1;
}

int mpcx_lmpc_create(const mpcx_dims *d, int device, mpcx_lmpc_t *out)
{
    if (!d || !out) return fail(MPCX_E_INVALID, "null argument");
    if (d->nx < 1 || d->nu < 1 || d->ny < 1 || d->ndu < 0 || d->ph < 1 || d->ch < 1 || d->ch > d->ph)
        return fail(MPCX_E_INVALID, "dimensions must satisfy nx,nu,ny,ph >= 1, 1 <= ch <= ph, ndu >= 0");
    if (d->nx > 64 || d->nu > 64 || d->ny > 64 || d->ndu > 64)
        return fail(MPCX_E_UNSUPPORTED, "nx, nu, ny, ndu must be <= 64 (one lane per component)");
    std::unique_ptr<mpcx_lmpc> h(new mpcx_lmpc(*d));
    h->device = device;
    h->host_only = device < 0;
    if (!h->host_only) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || device >= n)
            return fail(MPCX_E_DEVICE, "no such HIP device (the solve path has no CPU fallback)");
    }
    *out = h.release();
    return MPCX_OK;
}

int mpcx_lmpc_destroy(mpcx_lmpc_t h)
{
    if (!h) return MPCX_OK;
    if (!h->host_only) { (void)hipSetDevice(h->device); h->release(); h->release_staging(); }
    delete h;
    return MPCX_OK;
}

#define CHECK_H(h) do { if (!(h)) return fail(MPCX_E_INVALID, "null handle"); } while (0)

int mpcx_lmpc_set_state_space_model(mpcx_lmpc_t h, const double *A, const double *B, const double *C)
{
    CHECK_H(h);
    if (!A || !B || !C) return fail(MPCX_E_INVALID, "null matrix");
    auto &c = h->ctl;
    std::memcpy(c.A.a.data(), A, sizeof(double) * c.A.a.size());
    std::memcpy(c.B.a.data(), B, sizeof(double) * c.B.a.size());
    std::memcpy(c.C.a.data(), C, sizeof(double) * c.C.a.size());
    c.have_model = true;
    h->dirty = true;
    return MPCX_OK;
}

int mpcx_lmpc_set_disturbances(mpcx_lmpc_t h, const double *Bd, const double *Dd)
{
    CHECK_H(h);
    auto &c = h->ctl;
    if (c.d.ndu > 0) {
        if (!Bd || !Dd) return fail(MPCX_E_INVALID, "null matrix");
        std::memcpy(c.Bd.a.data(), Bd, sizeof(double) * c.Bd.a.size());
        std::memcpy(c.Dd.a.data(), Dd, sizeof(double) * c.Dd.a.size());
    }
    h->dirty = true;
    return MPCX_OK;
}

int mpcx_lmpc_set_objective_weights(mpcx_lmpc_t h, const double *OW, const double *UW, const double *DUW)
{
    CHECK_H(h);
    if (!OW || !UW || !DUW) return fail(MPCX_E_INVALID, "null matrix");
    h->ctl.set_objective(OW, UW, DUW);
    h->dirty = true;
    return MPCX_OK;
}

// Replicate-along-horizon helpers: {-1,-1} goes through the matrix setter, any other
// valid slice through the per-index setter, exactly as LMPC.hpp does (e.g. :436-481).
int mpcx_lmpc_set_objective_weights_slice(mpcx_lmpc_t h, const double *ow, const double *uw, const double *duw, int start, int end)
{
    CHECK_H(h);
    if (!ow || !uw || !duw) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    const int ph = c.d.ph;
    if (start == -1 && end == -1) {
        std::vector<double> O((size_t)c.d.ny * ph), U((size_t)c.d.nu * ph), D((size_t)c.d.nu * ph);
        for (int k = 0; k < ph; k++) {
            std::memcpy(&O[(size_t)k * c.d.ny], ow, sizeof(double) * c.d.ny);
            std::memcpy(&U[(size_t)k * c.d.nu], uw, sizeof(double) * c.d.nu);
            std::memcpy(&D[(size_t)k * c.d.nu], duw, sizeof(double) * c.d.nu);
        }
        c.set_objective(O.data(), U.data(), D.data());
    } else {
        if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
        for (int i = start; i < end; i++) c.set_objective_idx(i, ow, uw, duw);
    }
    h->dirty = true;
    return MPCX_OK;
}

int mpcx_lmpc_set_state_bounds(mpcx_lmpc_t h, const double *lo, const double *hi)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null matrix");
    h->ctl.set_state_bounds(lo, hi);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_state_bounds_slice(mpcx_lmpc_t h, const double *lo, const double *hi, int start, int end)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    if (start == -1 && end == -1) {
        std::vector<double> L((size_t)c.d.nx * c.d.ph), H((size_t)c.d.nx * c.d.ph);
        for (int k = 0; k < c.d.ph; k++) {
            std::memcpy(&L[(size_t)k * c.d.nx], lo, sizeof(double) * c.d.nx);
            std::memcpy(&H[(size_t)k * c.d.nx], hi, sizeof(double) * c.d.nx);
        }
        c.set_state_bounds(L.data(), H.data());
    } else {
        if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
        for (int i = start; i < end; i++) c.set_state_bounds_idx(i, lo, hi);
    }
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_input_bounds(mpcx_lmpc_t h, const double *lo, const double *hi)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null matrix");
    h->ctl.set_input_bounds(lo, hi);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_input_bounds_slice(mpcx_lmpc_t h, const double *lo, const double *hi, int start, int end)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    if (start == -1 && end == -1) {
        std::vector<double> L((size_t)c.d.nu * c.d.ch), H((size_t)c.d.nu * c.d.ch);
        for (int k = 0; k < c.d.ch; k++) {
            std::memcpy(&L[(size_t)k * c.d.nu], lo, sizeof(double) * c.d.nu);
            std::memcpy(&H[(size_t)k * c.d.nu], hi, sizeof(double) * c.d.nu);
        }
        c.set_input_bounds(L.data(), H.data());
    } else {
        if (!c.ctrl_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The control horizon slice is out of bounds");
        for (int i = start; i < end; i++) c.set_input_bounds_idx(i, lo, hi);
    }
    h->dirty = true;
    return MPCX_OK;
}
// Bounds on the input increments.  The reference's QP has these rows (ProblemBuilder.hpp:768-793) and no setter for them; columns past
// the control horizon are kept and not read (those moves stay pinned to zero).
static bool rate_column_ok(const double *lo, const double *hi, int nu, bool read)
{
    for (int j = 0; j < nu; j++) {
        if (std::isnan(lo[j]) || std::isnan(hi[j])) return false;
        if (read && lo[j] > hi[j]) return false;
    }
    return true;
}
int mpcx_lmpc_set_input_rate_bounds(mpcx_lmpc_t h, const double *lo, const double *hi)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null matrix");
    auto &c = h->ctl;
    for (int k = 0; k < c.d.ph; k++)
        if (!rate_column_ok(lo + (size_t)k * c.d.nu, hi + (size_t)k * c.d.nu, c.d.nu, k <= c.d.ch))
            return fail(MPCX_E_INVALID, "input rate bounds: NaN, or dumin > dumax within the control horizon");
    c.set_rate_bounds(lo, hi);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_input_rate_bounds_slice(mpcx_lmpc_t h, const double *lo, const double *hi, int start, int end)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    int s = start, e = end;
    if (start == -1 && end == -1) { s = 0; e = c.d.ph; }
    else if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
    if (!rate_column_ok(lo, hi, c.d.nu, s <= c.d.ch))
        return fail(MPCX_E_INVALID, "input rate bounds: NaN, or dumin > dumax within the control horizon");
    for (int i = s; i < e; i++) c.set_rate_bounds_idx(i, lo, hi);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_output_bounds(mpcx_lmpc_t h, const double *lo, const double *hi)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null matrix");
    h->ctl.set_output_bounds(lo, hi);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_output_bounds_slice(mpcx_lmpc_t h, const double *lo, const double *hi, int start, int end)
{
    CHECK_H(h);
    if (!lo || !hi) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    if (start == -1 && end == -1) {
        std::vector<double> L((size_t)c.d.ny * c.d.ph), H((size_t)c.d.ny * c.d.ph);
        for (int k = 0; k < c.d.ph; k++) {
            std::memcpy(&L[(size_t)k * c.d.ny], lo, sizeof(double) * c.d.ny);
            std::memcpy(&H[(size_t)k * c.d.ny], hi, sizeof(double) * c.d.ny);
        }
        c.set_output_bounds(L.data(), H.data());
    } else {
        if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
        for (int i = start; i < end; i++) c.set_output_bounds_idx(i, lo, hi);
    }
    h->dirty = true;
    return MPCX_OK;
}

// Soft constraints: a weight per state / output / scalar row, +inf = hard.  No counterpart in the reference's LMPC (its NLMPC has one slack for all
// rows, NLOptimizer.hpp:182-186).  A weight where no bound is finite is stored and has no effect.
static bool soft_weights_ok(const double *w, int n)
{
    for (int j = 0; w && j < n; j++)
        if (!(w[j] > 0.0)) return false;      // NaN, zero, negative
    return true;
}
int mpcx_lmpc_set_soft_constraint_weights_slice(mpcx_lmpc_t h, const double *xw, const double *yw, const double *sw, int start, int end)
{
    CHECK_H(h);
    auto &c = h->ctl;
    if (!soft_weights_ok(xw, c.d.nx) || !soft_weights_ok(yw, c.d.ny) || !soft_weights_ok(sw, 1))
        return fail(MPCX_E_INVALID, "soft constraint weights: NaN, zero or negative");
    if (start == -1 && end == -1) c.set_soft_weights(xw, yw, sw);
    else {
        if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
        for (int i = start; i < end; i++) c.set_soft_weights_idx(i, xw, yw, sw);
    }
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_soft_constraint_weights(mpcx_lmpc_t h, const double *xw, const double *yw, const double *sw)
{
    return mpcx_lmpc_set_soft_constraint_weights_slice(h, xw, yw, sw, -1, -1);
}

// Terminal cost 0.5 (x_ph - x_T)' P (x_ph - x_T) (include/mpcx.h).  No counterpart in the reference's LMPC
int mpcx_lmpc_set_terminal_cost(mpcx_lmpc_t h, const double *P, const double *xT, const double *Tx)
{
    CHECK_H(h);
    const std::string msg = h->ctl.set_terminal_cost(P, xT, Tx);
    if (!msg.empty()) return fail(MPCX_E_INVALID, msg);
    h->dirty = true;
    return MPCX_OK;
}

int mpcx_lmpc_set_scalar_constraint_slice(mpcx_lmpc_t h, double smin, double smax, const double *X, const double *U, int start, int end)
{
    CHECK_H(h);
    if (!X || !U) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    if (start == -1 && end == -1) {
        std::vector<double> L(c.d.ph, smin), H(c.d.ph, smax);
        c.set_scalar_vec(L.data(), H.data(), X, U);
    } else {
        if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
        for (int i = start; i < end; i++) c.set_scalar_idx(i, smin, smax, X, U);
    }
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_scalar_constraint_index(mpcx_lmpc_t h, int index, double smin, double smax, const double *X, const double *U)
{
    CHECK_H(h);
    if (!X || !U) return fail(MPCX_E_INVALID, "null vector");
    if (index < 0 || index >= h->ctl.d.ph) return fail(MPCX_E_INVALID, "Horizon index out of bounds");
    h->ctl.set_scalar_idx(index, smin, smax, X, U);
    h->dirty = true;
    return MPCX_OK;
}

// Linear rows lo <= Fx x_i + Fu v_i <= hi (include/mpcx.h).  No counterpart in the reference's LMPC
int mpcx_lmpc_set_linear_constraints(mpcx_lmpc_t h, int nc, const double *Fx, const double *Fu, const double *lo, const double *hi)
{
    CHECK_H(h);
    const std::string msg = h->ctl.set_linear(nc, Fx, Fu, lo, hi);
    if (!msg.empty()) return fail(MPCX_E_INVALID, msg);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_linear_constraints_slice(mpcx_lmpc_t h, int nc, const double *Fx, const double *Fu, const double *lo, const double *hi, int start, int end)
{
    CHECK_H(h);
    auto &c = h->ctl;
    int s = start, e = end;
    if (start == -1 && end == -1) { s = 0; e = c.d.ph; }
    else if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
    const std::string msg = c.set_linear_slice(nc, Fx, Fu, lo, hi, s, e);
    if (!msg.empty()) return fail(MPCX_E_INVALID, msg);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_linear_constraint_weights_slice(mpcx_lmpc_t h, const double *w, int start, int end)
{
    CHECK_H(h);
    auto &c = h->ctl;
    if (!(start == -1 && end == -1) && !c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
    const std::string msg = c.set_linear_weights(w, start, end);
    if (!msg.empty()) return fail(MPCX_E_INVALID, msg);
    h->dirty = true;
    return MPCX_OK;
}
int mpcx_lmpc_set_linear_constraint_weights(mpcx_lmpc_t h, const double *w)
{
    return mpcx_lmpc_set_linear_constraint_weights_slice(h, w, -1, -1);
}

int mpcx_lmpc_set_references(mpcx_lmpc_t h, const double *yref, const double *uref, const double *duref)
{
    CHECK_H(h);
    if (!yref || !uref || !duref) return fail(MPCX_E_INVALID, "null matrix");
    auto &c = h->ctl;
    std::memcpy(c.yRef.a.data(), yref, sizeof(double) * c.yRef.a.size());
    std::memcpy(c.uRef.a.data(), uref, sizeof(double) * c.uRef.a.size());
    std::memcpy(c.duRef.a.data(), duref, sizeof(double) * c.duRef.a.size());
    h->refs_dirty = true;        // the time-invariant terms stay (the reference's setReferences does not rebuild them either)
    return MPCX_OK;
}
int mpcx_lmpc_set_references_slice(mpcx_lmpc_t h, const double *yref, const double *uref, const double *duref, int start, int end)
{
    CHECK_H(h);
    if (!yref || !uref || !duref) return fail(MPCX_E_INVALID, "null vector");
    auto &c = h->ctl;
    int s = start, e = end;
    if (start == -1 && end == -1) { s = 0; e = c.d.ph; }
    else if (!c.pred_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The prediction horizon slice is out of bounds");
    for (int i = s; i < e; i++) {
        std::memcpy(c.yRef.col(i), yref, sizeof(double) * c.d.ny);
        std::memcpy(c.uRef.col(i), uref, sizeof(double) * c.d.nu);
        std::memcpy(c.duRef.col(i), duref, sizeof(double) * c.d.nu);
    }
    h->refs_dirty = true;        // the time-invariant terms stay (the reference's setReferences does not rebuild them either)
    return MPCX_OK;
}
int mpcx_lmpc_set_exogenous_inputs(mpcx_lmpc_t h, const double *dmeas)
{
    CHECK_H(h);
    auto &c = h->ctl;
    if (c.d.ndu > 0) {
        if (!dmeas) return fail(MPCX_E_INVALID, "null matrix");
        std::memcpy(c.dMeas.a.data(), dmeas, sizeof(double) * c.dMeas.a.size());
    }
    h->refs_dirty = true;        // the time-invariant terms stay (the reference's setReferences does not rebuild them either)
    return MPCX_OK;
}
int mpcx_lmpc_set_exogenous_inputs_slice(mpcx_lmpc_t h, const double *dmeas, int start, int end)
{
    CHECK_H(h);
    auto &c = h->ctl;
    int s = start, e = end;
    if (start == -1 && end == -1) { s = 0; e = c.d.ph; }
    // the reference validates this slice against the CONTROL horizon (LMPC.hpp:571, isControlHorizonSliceValid)
    else if (!c.ctrl_slice_valid(start, end)) return fail(MPCX_E_INVALID, "The control horizon slice is out of bounds");
    if (c.d.ndu > 0) {
        if (!dmeas) return fail(MPCX_E_INVALID, "null vector");
        for (int i = s; i < e; i++) std::memcpy(c.dMeas.col(i), dmeas, sizeof(double) * c.d.ndu);
    }
    h->refs_dirty = true;        // the time-invariant terms stay (the reference's setReferences does not rebuild them either)
    return MPCX_OK;
}

int mpcx_lmpc_set_optimizer_parameters(mpcx_lmpc_t h, const mpcx_lparams *p)
{
    CHECK_H(h);
    if (!p) return fail(MPCX_E_INVALID, "null parameters");
    if (p->maximum_iteration < 0 || !(p->alpha > 0 && p->alpha < 2) || !(p->rho > 0))
        return fail(MPCX_E_INVALID, "parameters out of range");
    h->ctl.prm = *p;
    h->dirty = true;
    return MPCX_OK;
}

int mpcx_lmpc_set_strict_infeasibility(mpcx_lmpc_t h, int on)
{
    CHECK_H(h);
    h->strict_infeasible = on != 0;
    h->dirty = true;
    return MPCX_OK;
}

// References / exogenous inputs changed and nothing else: the condensed matrices, their factors, the workspace and the
// queues stay where they are; what depends on the references -- the shared reference arrays and the constant column of the
// stacked maps of the MFMA assemble kernel -- is recomputed on the host (one roll-out per input component) and copied over
// the device arrays in place.
static int refresh_references(mpcx_lmpc_t h)
{
    const auto &c = h->ctl;
    h->ctl.refresh_fast_maps(h->cond);
    h->refs_dirty = false;
    ++h->n_ref_refreshes;
    if (h->host_only) return MPCX_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    // the arrays are overwritten in place: launches of this handle still in flight on a non-blocking stream (they read them) are not
    // ordered against a copy on the null stream -- wait for the device first (a reference change is a host-side event, not the hot path)
    if (hipDeviceSynchronize() != hipSuccess) return fail(MPCX_E_DEVICE, "hipDeviceSynchronize failed");
    const mpcx::LmpcDev &D = h->dev;
    const bool ok = h->reup(D.yref_s, c.yRef.a) && h->reup(D.uref_s, c.uRef.a) && h->reup(D.duref_s, c.duRef.a) &&
                    h->reup(D.dmeas_s, c.dMeas.a) && h->reup(D.MA0, h->cond.MA[0]) && h->reup(D.MA1, h->cond.MA[1]) &&
                    h->reup(D.MF0, h->cond.MF[0]) && h->reup(D.MF1, h->cond.MF[1]);
    if (ok && !h->cond.MA[0].empty()) {          // ... and their packed copies (lmpc_solve_group's)
        std::vector<double> pk(mpcx::lmpc_packed_len(h->cond.rowsA, h->cond.kin));
        for (int v = 0; v < 2; ++v) {
            mpcx::lmpc_pack_mfma_tiles(h->cond.MA[v].data(), h->cond.rowsA, h->cond.kin, pk.data());
            if (!h->reup(v ? D.MA1p : D.MA0p, pk)) return fail(MPCX_E_DEVICE, "device upload failed");
        }
    }
    return ok ? MPCX_OK : fail(MPCX_E_DEVICE, "device upload failed");
}

static int param_operand(mpcx_lmpc_t h, bool device);

int mpcx_lmpc_setup(mpcx_lmpc_t h)
{
    CHECK_H(h);
    if (!h->dirty) return h->refs_dirty ? refresh_references(h) : MPCX_OK;
    h->refs_dirty = false;
    ++h->n_full_setups;
    std::string msg = h->ctl.condense(h->cond);
    if (!msg.empty()) return fail(msg == "state-space model not set" ? MPCX_E_STATE : MPCX_E_NUMERIC, msg);
    const auto &c = h->ctl;
    const auto &o = h->cond;
    if (mpcx::lmpc_kernel_variant(o.ldz, o.ldg) < 0)
        return fail(MPCX_E_UNSUPPORTED, "condensed problem larger than 512 variables / rows");
    mpcx::LmpcDev &D = h->dev;
    fill_dev_scalars(h, c, o, D);
    h->param_cq.clear();
    h->model_xq.clear();                 // (built again when somebody asks: model_operand)
    if (h->host_only) { h->dirty = false; return MPCX_OK; }

    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    h->release();
    int rc = MPCX_OK;
    fill_dev_arrays(h, c, o, D, *h, rc);
    if (rc != MPCX_OK) return fail(rc, "device upload failed");
    {
        // (the linear part of MF1 does not depend on references or exogenous inputs: a reference refresh leaves this operand as it is)
        std::vector<double> t0p(mpcx::lmpc_sens_operand(o.nz, o.kin, o.rowsF, nullptr, nullptr));
        mpcx::lmpc_sens_operand(o.nz, o.kin, o.rowsF, o.MF[1].data(), t0p.data());
        h->sens_t0p = h->up(t0p, rc);
        if (rc != MPCX_OK) return fail(rc, "device upload failed");
    }
    // the parameter-sensitivity kernel's operand beside it (Cq depends on the model and the blocking alone): its launch allocates and copies nothing
    if (param_operand(h, true) != MPCX_OK) return MPCX_E_DEVICE;
    {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(mpcx::LmpcDev)) != hipSuccess) return fail(MPCX_E_DEVICE, "hipMalloc failed");
        h->allocs.push_back(p);
        if (hipMemcpy(p, &D, sizeof(mpcx::LmpcDev), hipMemcpyHostToDevice) != hipSuccess) return fail(MPCX_E_DEVICE, "hipMemcpy failed");
        h->dev_d = static_cast<mpcx::LmpcDev *>(p);
    }
    h->dirty = false;
    return MPCX_OK;
}

// The caller's batch as the kernels take it.  shared[4]: where a reference in MPCX_REF_SHARED mode is read from (yref, uref, duref, dmeas) -- the
// controller's own device arrays; null in a bank, where each controller reads its own through the model struct.
static int make_batch(const mpcx_dims &d, const mpcx_lmpc_batch *b, const double *const shared[4], mpcx::LmpcBatchDev &B)
{
    B = mpcx::LmpcBatchDev{};
    B.batch = b->batch; B.x0 = b->x0; B.u0 = b->u0;
    auto refsel = [&](const double *p, int mode, const double *sh, int n, const double *&op, long &bs, long &ks) -> bool {
        if (mode == MPCX_REF_SHARED) { op = sh; bs = 0; ks = n; return true; }
        if (!p) return false;
        if (mode == MPCX_REF_PER_INSTANCE) { op = p; bs = n; ks = 0; return true; }
        if (mode == MPCX_REF_PER_STEP) { op = p; bs = (long)d.ph * n; ks = n; return true; }
        return false;
    };
    if (!refsel(b->yref, b->yref_mode, shared[0], d.ny, B.yref, B.yref_bs, B.yref_ks) ||
        !refsel(b->uref, b->uref_mode, shared[1], d.nu, B.uref, B.uref_bs, B.uref_ks) ||
        !refsel(b->duref, b->duref_mode, shared[2], d.nu, B.duref, B.duref_bs, B.duref_ks) ||
        !refsel(b->dmeas, b->dmeas_mode, shared[3], d.ndu, B.dmeas, B.dmeas_bs, B.dmeas_ks))
        return fail(MPCX_E_INVALID, "reference array missing for a non-shared mode, or unknown mode");
    B.cmd = b->cmd; B.cost = b->cost; B.status = b->status; B.solver_status = b->solver_status;
    B.is_feasible = b->is_feasible; B.iterations = b->iterations;
    B.active_lower = b->active_lower; B.active_upper = b->active_upper;
    B.seq_state = b->seq_state; B.seq_output = b->seq_output; B.seq_input = b->seq_input;
    B.polish_rounds = b->polish_rounds; B.active_count = b->active_count;
    B.warm_lower = b->warm_active_lower; B.warm_upper = b->warm_active_upper; B.warm_shift = b->warm_shift;
    if ((B.warm_lower == nullptr) != (B.warm_upper == nullptr)) return fail(MPCX_E_INVALID, "warm_active_lower and warm_active_upper go together");
    return MPCX_OK;
}

// ... of a single controller: its argument checks, its own shared references, its cycle buffer
static int make_handle_batch(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, mpcx::LmpcBatchDev &B)
{
    if (b->batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (b->batch > 0 && (!b->x0 || !b->u0 || !b->cmd)) return fail(MPCX_E_INVALID, "x0, u0 and cmd are required");
    const auto &D = h->dev;
    const double *const shared[4] = {D.yref_s, D.uref_s, D.duref_s, D.dmeas_s};
    const int rc = make_batch(h->ctl.d, b, shared, B);
    B.dbg_cycles = h->dbg_cycles;
    return rc;
}

// Which kernels a call of this handle takes.  The MFMA assemble kernel serves shared or per-instance-constant output references with everything
// else shared, any other layout goes through the generic roll-out kernel; the one-kernel forms assemble the same way, so they need the same layouts.
// Automatic mode (use_fused < 0) takes the group form up to group_max instances -- of the whole batch where this handle solves a shard of one.
static mpcx::LmpcPlan lmpc_plan(const mpcx_lmpc *h, const mpcx_lmpc_batch *b)
{
    using mpcx::LmpcAssemble; using mpcx::LmpcForm;
    mpcx::LmpcPlan p{LmpcAssemble::Generic, LmpcForm::TwoKernels, 0};
    if (b->uref_mode != MPCX_REF_SHARED || b->duref_mode != MPCX_REF_SHARED || b->dmeas_mode != MPCX_REF_SHARED || h->force_generic) return p;
    if (b->yref_mode == MPCX_REF_SHARED) p.assemble = LmpcAssemble::MfmaSharedYref;
    else if (b->yref_mode == MPCX_REF_PER_INSTANCE) p.assemble = LmpcAssemble::MfmaInstanceYref;
    else return p;
    const int per_instance = p.assemble == LmpcAssemble::MfmaInstanceYref ? 1 : 0;
    const int whole = b->batch > h->total_batch ? b->batch : h->total_batch;
    if (h->dev.group_ok && (h->use_fused == 2 || (h->use_fused < 0 && whole <= h->group_max))) { p.form = LmpcForm::Group; p.fused = 3 + per_instance; }
    else if (h->dev.fused_ok && !h->dbg_cycles && h->use_fused == 1) { p.form = LmpcForm::FusedMatvec; p.fused = 1 + per_instance; }
    return p;
}
// the bank: roll-out assemble, lean solve, ADMM fallback
static constexpr mpcx::LmpcPlan kHeteroPlan{mpcx::LmpcAssemble::Generic, mpcx::LmpcForm::TwoKernels, 0};

// a launch that failed: a step that broke off may have filed failures nobody served
static int launch_failed(int lr, const mpcx::LmpcScratch &sc, void *stream)
{
    (void)mpcx::lmpc_fallback_reset(sc.fq, stream);
    if (lr == -2) return fail(MPCX_E_UNSUPPORTED, "problem dimensions exceed the kernel's LDS budget");
    return fail(MPCX_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
}

int mpcx_lmpc_solve_batch(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream)
{
    CHECK_H(h);
    if (!b) return fail(MPCX_E_INVALID, "null batch");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the solve path needs a HIP device, there is no CPU fallback");
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (b->batch == 0) return MPCX_OK;      // an empty batch is a no-op, whatever its pointers
    mpcx::LmpcBatchDev B;
    rc = make_handle_batch(h, b, B);
    if (rc != MPCX_OK) return rc;
    if (mpcx::lmpc_scratch_reserve(h->scratch, h->dev, b->batch, true, stream) != 0) return fail(MPCX_E_DEVICE, "workspace allocation failed");
    const int lr = mpcx::lmpc_launch(h->dev, h->dev_d, B, h->scratch, stream, 7, lmpc_plan(h, b));
    if (lr == 0) { h->solved_full = h->n_full_setups; h->solved_refs = h->n_ref_refreshes; }
    else h->solved_full = h->solved_refs = -1;
    return lr == 0 ? MPCX_OK : launch_failed(lr, h->scratch, stream);
}

int mpcx_lmpc_sens_size(void) { return (int)sizeof(mpcx_lmpc_sens); }

int mpcx_lmpc_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_sens *s, void *stream)
{
    CHECK_H(h);
    if (!s) return fail(MPCX_E_INVALID, "null sensitivity descriptor");
    if (s->mode != MPCX_SENS_JACOBIAN && s->mode != MPCX_SENS_VJP) return fail(MPCX_E_INVALID, "unknown sensitivity mode");
    if (s->batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (s->batch > 0 && (!s->active_lower || !s->active_upper)) return fail(MPCX_E_INVALID, "active_lower and active_upper are required");
    if (s->batch > 0 && s->mode == MPCX_SENS_VJP && !s->seed_cmd && !s->seed_input) return fail(MPCX_E_INVALID, "a vector-Jacobian product needs seed_cmd or seed_input");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the sensitivity kernel needs a HIP device, there is no CPU fallback");
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (s->batch == 0) return MPCX_OK;
    mpcx::LmpcSensArgs a{};
    a.batch = s->batch; a.jacobian = s->mode == MPCX_SENS_JACOBIAN;
    a.active_lower = s->active_lower; a.active_upper = s->active_upper; a.status = s->status;
    a.seed_cmd = a.jacobian ? nullptr : s->seed_cmd; a.seed_input = a.jacobian ? nullptr : s->seed_input;
    a.d_x0 = s->d_x0; a.d_u0 = s->d_u0; a.d_yref = s->d_yref; a.flags = s->flags;
    const int lr = mpcx::lmpc_sens_launch(h->dev, h->dev_d, h->sens_t0p, a, stream);
    if (lr == -2) return fail(MPCX_E_UNSUPPORTED, "problem dimensions exceed the sensitivity kernel's LDS budget");
    return lr == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
}

// Cq of the current set-up on the host (a host-only handle: at first use) and, with a device, packed in HBM (by the set-up)
static int param_operand(mpcx_lmpc_t h, bool device)
{
    const auto &c = h->ctl;
    const auto &o = h->cond;
    if (h->param_cq.empty()) {
        h->param_cq.resize(mpcx::lmpc_param_sens_cq(c.d.nx, c.d.nu, c.d.ny, c.d.ph, o.nz, nullptr, nullptr, nullptr, nullptr, nullptr));
        mpcx::lmpc_param_sens_cq(c.d.nx, c.d.nu, c.d.ny, c.d.ph, o.nz, c.A.a.data(), c.B.a.data(), c.C.a.data(), o.blk.data(), h->param_cq.data());
    }
    if (device && !h->param_cqp) {
        const int rows16 = (c.d.ny * c.d.ph + 15) / 16 * 16;
        std::vector<double> pk(mpcx::lmpc_packed_len(rows16, o.nz));
        mpcx::lmpc_pack_mfma_tiles(h->param_cq.data(), rows16, o.nz, pk.data());
        int rc = MPCX_OK;
        h->param_cqp = h->up(pk, rc);
        if (rc != MPCX_OK) { h->param_cqp = nullptr; return fail(rc, "device upload failed"); }
    }
    return MPCX_OK;
}

int mpcx_lmpc_param_sens_size(void) { return (int)sizeof(mpcx_lmpc_param_sens); }

int mpcx_lmpc_param_sens_reserve(mpcx_lmpc_t h, int batch)
{
    CHECK_H(h);
    if (batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the parameter-sensitivity kernel needs a HIP device, there is no CPU fallback");
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    const size_t need = mpcx::lmpc_param_sens_partials(h->dev, batch);
    if (need > h->param_part_cap) {
        if (h->param_part) (void)hipFree(h->param_part);
        h->param_part = nullptr; h->param_part_cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&h->param_part), need * sizeof(double)) != hipSuccess) return fail(MPCX_E_DEVICE, "allocation of the partial sums failed");
        h->param_part_cap = need;
    }
    return MPCX_OK;
}

int mpcx_lmpc_param_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_param_sens *s, void *stream)
{
    CHECK_H(h);
    if (!s) return fail(MPCX_E_INVALID, "null parameter-sensitivity descriptor");
    const mpcx_lmpc_batch *b = s->solved;
    if (!b) return fail(MPCX_E_INVALID, "the solved batch is required");
    if (b->batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (s->reduce != 0 && s->reduce != 1) return fail(MPCX_E_INVALID, "reduce must be 0 or 1");
    if (b->batch > 0 && (!b->active_lower || !b->active_upper)) return fail(MPCX_E_INVALID, "active_lower and active_upper of the solved batch are required");
    if (b->batch > 0 && (!b->seq_output || !b->seq_input)) return fail(MPCX_E_INVALID, "seq_output and seq_input of the solved batch are required");
    if (b->batch > 0 && (!b->x0 || !b->u0)) return fail(MPCX_E_INVALID, "x0 and u0 of the solved batch are required");
    if (b->batch > 0 && !s->seed_cmd && !s->seed_input) return fail(MPCX_E_INVALID, "a parameter sensitivity needs seed_cmd or seed_input");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the parameter-sensitivity kernel needs a HIP device, there is no CPU fallback");
    // (a set-up that ran since the handle's last solve -- any call sets a changed controller up -- has replaced what that solve's active sets refer to)
    if (h->dirty || h->refs_dirty || !h->dev_d || h->solved_full != h->n_full_setups || h->solved_refs != h->n_ref_refreshes)
        return fail(MPCX_E_STATE, "the controller changed since the set-up that solved this batch (or nothing was solved): solve again first");
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (b->batch == 0) return MPCX_OK;
    mpcx::LmpcBatchDev B;
    {
        // (cmd is not read here; the solve's own check of it does not apply)
        const auto &D = h->dev;
        const double *const shared[4] = {D.yref_s, D.uref_s, D.duref_s, D.dmeas_s};
        const int rc = make_batch(h->ctl.d, b, shared, B);
        if (rc != MPCX_OK) return rc;
    }
    if (s->reduce && mpcx::lmpc_param_sens_partials(h->dev, b->batch) > h->param_part_cap)
        return fail(MPCX_E_STATE, "reduce = 1 needs mpcx_lmpc_param_sens_reserve for this batch size first: the launch allocates nothing");
    if (!h->param_cqp) return fail(MPCX_E_STATE, "the controller was never set up on the device");
    mpcx::LmpcParamSensArgs a{};
    a.batch = b->batch; a.reduce = s->reduce != 0;
    a.active_lower = b->active_lower; a.active_upper = b->active_upper; a.status = b->status;
    a.seed_cmd = s->seed_cmd; a.seed_input = s->seed_input;
    a.u0 = b->u0; a.seq_output = b->seq_output; a.seq_input = b->seq_input;
    a.yref = B.yref; a.yref_bs = B.yref_bs; a.yref_ks = B.yref_ks;
    a.uref = B.uref; a.uref_bs = B.uref_bs; a.uref_ks = B.uref_ks;
    a.duref = B.duref; a.duref_bs = B.duref_bs; a.duref_ks = B.duref_ks;
    a.d_oweight = s->d_oweight; a.d_uweight = s->d_uweight; a.d_duweight = s->d_duweight; a.d_lower = s->d_lower; a.d_upper = s->d_upper;
    a.flags = s->flags; a.n_used = s->n_used; a.partials = s->reduce ? h->param_part : nullptr;
    const int lr = mpcx::lmpc_param_sens_launch(h->dev, h->dev_d, h->param_cqp, a, stream);
    if (lr == -2) return fail(MPCX_E_UNSUPPORTED, "problem dimensions exceed the parameter-sensitivity kernel's LDS budget");
    return lr == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
}

// Xq of the current set-up on the host (at first use) and, with a device, packed in HBM
static int model_operand(mpcx_lmpc_t h, bool device)
{
    const auto &c = h->ctl;
    const auto &o = h->cond;
    if (h->model_xq.empty()) {
        h->model_xq.resize(mpcx::lmpc_model_sens_xq(c.d.nx, c.d.nu, c.d.ph, o.nz, nullptr, nullptr, nullptr, nullptr));
        mpcx::lmpc_model_sens_xq(c.d.nx, c.d.nu, c.d.ph, o.nz, c.A.a.data(), c.B.a.data(), o.blk.data(), h->model_xq.data());
    }
    if (device && !h->model_xqp) {
        const int rows16 = (c.d.nx * c.d.ph + 15) / 16 * 16;
        std::vector<double> pk(mpcx::lmpc_packed_len(rows16, o.nz));
        mpcx::lmpc_pack_mfma_tiles(h->model_xq.data(), rows16, o.nz, pk.data());
        int rc = MPCX_OK;
        h->model_xqp = h->up(pk, rc);
        if (rc != MPCX_OK) { h->model_xqp = nullptr; return fail(rc, "device upload failed"); }
    }
    return MPCX_OK;
}

int mpcx_lmpc_model_sens_size(void) { return (int)sizeof(mpcx_lmpc_model_sens); }

int mpcx_lmpc_model_sens_reserve(mpcx_lmpc_t h, int batch)
{
    CHECK_H(h);
    if (batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the model-sensitivity kernel needs a HIP device, there is no CPU fallback");
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    rc = model_operand(h, true);
    if (rc != MPCX_OK) return rc;
    const size_t need = mpcx::lmpc_model_sens_partials(h->dev, batch);
    if (need > h->model_part_cap) {
        if (h->model_part) (void)hipFree(h->model_part);
        h->model_part = nullptr; h->model_part_cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&h->model_part), need * sizeof(double)) != hipSuccess) return fail(MPCX_E_DEVICE, "allocation of the partial sums failed");
        h->model_part_cap = need;
    }
    return MPCX_OK;
}

int mpcx_lmpc_model_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_model_sens *s, void *stream)
{
    CHECK_H(h);
    if (!s) return fail(MPCX_E_INVALID, "null model-sensitivity descriptor");
    const mpcx_lmpc_batch *b = s->solved;
    if (!b) return fail(MPCX_E_INVALID, "the solved batch is required");
    if (b->batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (s->reduce != 0 && s->reduce != 1) return fail(MPCX_E_INVALID, "reduce must be 0 or 1");
    if (b->batch > 0 && (!b->active_lower || !b->active_upper)) return fail(MPCX_E_INVALID, "active_lower and active_upper of the solved batch are required");
    if (b->batch > 0 && (!b->x0 || !b->u0)) return fail(MPCX_E_INVALID, "x0 and u0 of the solved batch are required");
    if (b->batch > 0 && !s->seed_cmd && !s->seed_input) return fail(MPCX_E_INVALID, "a model sensitivity needs seed_cmd or seed_input");
    if (b->batch > 0 && (!b->seq_state || !b->seq_output || !b->seq_input)) return fail(MPCX_E_STATE, "the solved batch carries no sequences: seq_state, seq_output and seq_input are required");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the model-sensitivity kernel needs a HIP device, there is no CPU fallback");
    if (h->dirty || h->refs_dirty || !h->dev_d || h->solved_full != h->n_full_setups || h->solved_refs != h->n_ref_refreshes)
        return fail(MPCX_E_STATE, "the controller changed since the set-up that solved this batch (or nothing was solved): solve again first");
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (b->batch == 0) return MPCX_OK;
    mpcx::LmpcBatchDev B;
    {
        const auto &D = h->dev;
        const double *const shared[4] = {D.yref_s, D.uref_s, D.duref_s, D.dmeas_s};
        const int rc = make_batch(h->ctl.d, b, shared, B);
        if (rc != MPCX_OK) return rc;
    }
    if (s->reduce && mpcx::lmpc_model_sens_partials(h->dev, b->batch) > h->model_part_cap)
        return fail(MPCX_E_STATE, "reduce = 1 needs mpcx_lmpc_model_sens_reserve for this batch size first: the launch allocates nothing");
    if (!h->model_xqp) {
        // the first launch after a set-up builds and uploads Xq, unless a capture is under way: then mpcx_lmpc_model_sens_reserve comes first
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (stream && hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(MPCX_E_STATE, "a captured launch needs mpcx_lmpc_model_sens_reserve after the set-up first: the launch allocates nothing");
        const int rc = model_operand(h, true);
        if (rc != MPCX_OK) return rc;
    }
    mpcx::LmpcModelSensArgs a{};
    a.batch = b->batch; a.reduce = s->reduce != 0;
    a.active_lower = b->active_lower; a.active_upper = b->active_upper; a.status = b->status;
    a.seed_cmd = s->seed_cmd; a.seed_input = s->seed_input;
    a.u0 = b->u0; a.seq_state = b->seq_state; a.seq_output = b->seq_output; a.seq_input = b->seq_input;
    a.yref = B.yref; a.yref_bs = B.yref_bs; a.yref_ks = B.yref_ks;
    a.uref = B.uref; a.uref_bs = B.uref_bs; a.uref_ks = B.uref_ks;
    a.duref = B.duref; a.duref_bs = B.duref_bs; a.duref_ks = B.duref_ks;
    a.dmeas = B.dmeas; a.dmeas_bs = B.dmeas_bs; a.dmeas_ks = B.dmeas_ks;
    a.d_A = s->d_A; a.d_B = s->d_B; a.d_C = s->d_C; a.d_Bd = s->d_Bd; a.d_Dd = s->d_Dd;
    a.flags = s->flags; a.n_used = s->n_used; a.partials = s->reduce ? h->model_part : nullptr;
    const int lr = mpcx::lmpc_model_sens_launch(h->dev, h->dev_d, h->model_xqp, a, stream);
    if (lr == -2) return fail(MPCX_E_UNSUPPORTED, "problem dimensions exceed the model-sensitivity kernel's LDS budget");
    return lr == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
}

struct mpcx_lmpc_graph {
    hipGraphExec_t exec = nullptr;
    int device = 0;
    mpcx_lmpc_t owner = nullptr;        // the controller whose step was captured
};

int mpcx_lmpc_graph_create(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream, mpcx_lmpc_graph_t *out)
{
    CHECK_H(h);
    if (!b || !out) return fail(MPCX_E_INVALID, "null argument");
    if (!stream) return fail(MPCX_E_INVALID, "a graph is captured on a non-default stream");
    if (b->batch <= 0) return fail(MPCX_E_INVALID, "empty batch");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // one plain solve first: it runs whatever set-up is pending, sizes the workspace and configures the kernels -- none of
    // which can be part of a capture
    int rc = mpcx_lmpc_solve_batch(h, b, stream);
    if (rc != MPCX_OK) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(MPCX_E_DEVICE, "the warm-up solve failed");
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return fail(MPCX_E_DEVICE, "hipStreamBeginCapture failed");
    rc = mpcx_lmpc_solve_batch(h, b, stream);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc != MPCX_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ec != hipSuccess || !graph) return fail(MPCX_E_DEVICE, "hipStreamEndCapture failed");
    auto *g = new mpcx_lmpc_graph;
    g->device = h->device;
    g->owner = h;
    const hipError_t ei = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { delete g; return fail(MPCX_E_DEVICE, "hipGraphInstantiate failed"); }
    *out = g;
    return MPCX_OK;
}

int mpcx_lmpc_graph_launch(mpcx_lmpc_graph_t g, void *stream)
{
    if (!g || !g->exec) return fail(MPCX_E_INVALID, "null graph");
    // a setter since the capture needs a set-up pass the captured launches do not contain (mpcx_lmpc_solve_batch runs it; a
    // reference-only change is picked up by one plain solve, anything else needs a new graph)
    if (g->owner && (g->owner->dirty || g->owner->refs_dirty))
        return fail(MPCX_E_STATE, "the controller changed since the graph was captured: call mpcx_lmpc_solve_batch once (references) or capture again");
    if (hipSetDevice(g->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (hipGraphLaunch(g->exec, reinterpret_cast<hipStream_t>(stream)) != hipSuccess) return fail(MPCX_E_DEVICE, "hipGraphLaunch failed");
    return MPCX_OK;
}

int mpcx_lmpc_graph_destroy(mpcx_lmpc_graph_t g)
{
    if (!g) return MPCX_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    delete g;
    return MPCX_OK;
}

// ---- the closed loop on the device ------------------------------------------------------------------------------------------------
// A tick is the owner's ordinary step (mpcx_lmpc_solve_batch, or mpcx_lmpc_hetero_solve_batch for a bank, on the loop's own x / u buffers) followed
// by lmpc_loop_advance; both are captured once, as a linear chain on one stream, and a run is "begin and pack kernels, then the tick graph `ticks`
// times".  Tick 0 solves cold and the later ticks with the carried working sets: the two differ in the descriptor's warm pointers, which a captured
// launch cannot change, so they are two graphs.
struct mpcx_lmpc_loop {
    mpcx_lmpc_t owner = nullptr;                 // a controller's loop ...
    mpcx_lmpc_hetero_t bank = nullptr;           // ... or a bank's, with the caller's instance -> controller map (device array or null)
    const int32_t *model_index = nullptr;
    int device = 0, ticks = 0;
    int setups = 0;                              // the owner's count of full set-ups when the loop was made: a later one freed what the graphs point to
    mpcx::LmpcLoopDev L{};
    hipGraphExec_t first = nullptr, next = nullptr;   // tick 0; every later tick (null: the same graph serves all)
    char *slab = nullptr;                        // every private buffer of the loop, one allocation
    mpcx_lmpc_batch step{};                      // the cold step's descriptor and the loop's kind: what a backward pass (mpcx_lmpc_loop_grad_*) starts from
    bool plain = true;
    ~mpcx_lmpc_loop()
    {
        if (first) (void)hipGraphExecDestroy(first);
        if (next) (void)hipGraphExecDestroy(next);
        if (slab) (void)hipFree(slab);
    }
    int solve(const mpcx_lmpc_batch *b, void *s) const { return owner ? mpcx_lmpc_solve_batch(owner, b, s) : mpcx_lmpc_hetero_solve_batch(bank, b, model_index, s); }
};

int mpcx_lmpc_loop_desc_size(void) { return (int)sizeof(mpcx_lmpc_loop_desc); }
int mpcx_lmpc_observer_desc_size(void) { return (int)sizeof(mpcx_lmpc_observer_desc); }
int mpcx_lmpc_disturbance_observer_desc_size(void) { return (int)sizeof(mpcx_lmpc_disturbance_observer_desc); }
int mpcx_lmpc_target_desc_size(void) { return (int)sizeof(mpcx_lmpc_target_desc); }

// one tick -- the step of descriptor `b`, then the advance kernel -- captured on `s`
static int capture_tick(const mpcx_lmpc_loop &l, const mpcx_lmpc_batch *b, hipStream_t s, hipGraphExec_t *exec)
{
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return fail(MPCX_E_DEVICE, "hipStreamBeginCapture failed");
    int rc = l.solve(b, s);
    const int la = rc == MPCX_OK ? mpcx::lmpc_loop_advance(l.L, s) : 0;
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc == MPCX_OK && la != 0) rc = fail(MPCX_E_DEVICE, "launch of the advance kernel failed");
    if (rc == MPCX_OK && (ec != hipSuccess || !graph)) rc = fail(MPCX_E_DEVICE, "hipStreamEndCapture failed");
    if (rc == MPCX_OK && hipGraphInstantiate(exec, graph, nullptr, nullptr, 0) != hipSuccess) rc = fail(MPCX_E_DEVICE, "hipGraphInstantiate failed");
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
}

// what a descriptor must satisfy whatever it is given to: the checks that need no look at a controller's or a bank's state
static int check_loop_desc(const mpcx_lmpc_loop_desc *d)
{
    if (d->batch <= 0) return fail(MPCX_E_INVALID, "a loop needs batch >= 1");
    if (d->ticks <= 0) return fail(MPCX_E_INVALID, "a loop needs ticks >= 1");
    if (!d->x0 || !d->u0) return fail(MPCX_E_INVALID, "x0 and u0 are required");
    if (!d->traj_x || !d->traj_u) return fail(MPCX_E_INVALID, "traj_x and traj_u are required");
    const double *const ref_p[4] = {d->yref, d->uref, d->duref, d->dmeas};
    const int ref_m[4] = {d->yref_mode, d->uref_mode, d->duref_mode, d->dmeas_mode};
    static const char *const ref_name[4] = {"yref", "uref", "duref", "dmeas"};
    for (int a = 0; a < 4; ++a) {
        if (ref_m[a] < MPCX_REF_SHARED || ref_m[a] > MPCX_REF_PREVIEW) return fail(MPCX_E_INVALID, std::string(ref_name[a]) + ": unknown reference mode");
        if (ref_m[a] != MPCX_REF_SHARED && !ref_p[a]) return fail(MPCX_E_INVALID, std::string(ref_name[a]) + ": array missing for a non-shared mode");
    }
    if (d->plant_batch && (d->plant_A || d->plant_B || d->plant_Bd))
        return fail(MPCX_E_INVALID, "plant_batch (a plant per instance) and plant_A / plant_B / plant_Bd (one plant for the batch) exclude each other");
    return MPCX_OK;
}

// "one for the batch (a host array) or one per instance (a device array)": what every observer and target descriptor must satisfy, likewise
// without a look at the owner's state.  bank: its controllers differ, one for the batch cannot serve them all
struct PerInstanceNouns {
    const char *what, *loop, *type;              // "null <what>: <loop> needs an <type>"
    const char *one;                             // the field with one for the batch; <one>_batch has one per instance
    const char *its_loop, *needs;                // "... <its_loop> takes <one>_batch, not <one>", "<needs> <one> or <one>_batch"
};
static const PerInstanceNouns kObserverNouns = {"observer", "an observed loop", "mpcx_lmpc_observer_desc", "gain", "its observed loop", "an observer needs"};
static const PerInstanceNouns kDisturbanceObserverNouns = {"observer", "an offset-free loop", "mpcx_lmpc_disturbance_observer_desc", "gain", "its offset-free loop",
                                                           "a disturbance observer needs"};
static const PerInstanceNouns kTargetNouns = {"target", "a loop with steady-state targets", "mpcx_lmpc_target_desc", "map", "its loop", "steady-state targets need"};

static int check_one_or_per_instance(const void *desc, const void *one, const void *per_instance, bool bank, const PerInstanceNouns &n)
{
    const std::string o = n.one, ob = o + "_batch";
    if (!desc) return fail(MPCX_E_INVALID, std::string("null ") + n.what + ": " + n.loop + " needs an " + n.type);
    if (one && per_instance) return fail(MPCX_E_INVALID, o + " (one " + o + " for the batch) and " + ob + " (a " + o + " per instance) exclude each other");
    if (bank && one) return fail(MPCX_E_INVALID, std::string("a bank's controllers differ: ") + n.its_loop + " takes " + ob + ", not " + o);
    if (!one && !per_instance) return fail(MPCX_E_INVALID, std::string(n.needs) + " " + o + " or " + ob);
    return MPCX_OK;
}

// what kind of loop an entry makes
enum class LoopKind { Plain, Observed, OffsetFree, OffsetFreeTarget };

// the six fields the two observer descriptors share
struct ObserverView {
    const double *gain, *gain_batch, *xhat0, *meas_noise;
    double *traj_xhat, *traj_y;
};
extern "C++" template <typename Desc> static ObserverView observer_view(const Desc *o) { return {o->gain, o->gain_batch, o->xhat0, o->meas_noise, o->traj_xhat, o->traj_y}; }

// What an entry was given.  o: the observer of an observed loop; od: the disturbance observer of an offset-free loop; td: its targets; each null
// where the kind has none.
struct LoopRequest {
    LoopKind kind;
    const mpcx_lmpc_loop_desc *d;
    const mpcx_lmpc_observer_desc *o;
    const mpcx_lmpc_disturbance_observer_desc *od;
    const mpcx_lmpc_target_desc *td;
    void *stream;
    mpcx_lmpc_loop_t *out;
    bool offset_free() const { return kind == LoopKind::OffsetFree || kind == LoopKind::OffsetFreeTarget; }
    bool targets() const { return kind == LoopKind::OffsetFreeTarget; }
};

// What all eight entries refuse before they look at the owner's state, in this order: the loop descriptor, the observer and target descriptors, the
// owner's dimensions (dm; without exogenous inputs there is no disturbance model).  The owner itself is the caller's to check, ahead of this.
static int check_loop_request(const LoopRequest &r, bool bank, const mpcx_dims &dm)
{
    if (!r.d || !r.out) return fail(MPCX_E_INVALID, "null argument");
    int rc = check_loop_desc(r.d);
    if (rc == MPCX_OK && r.kind == LoopKind::Observed) rc = check_one_or_per_instance(r.o, r.o ? r.o->gain : nullptr, r.o ? r.o->gain_batch : nullptr, bank, kObserverNouns);
    if (rc == MPCX_OK && r.offset_free())
        rc = check_one_or_per_instance(r.od, r.od ? r.od->gain : nullptr, r.od ? r.od->gain_batch : nullptr, bank, kDisturbanceObserverNouns);
    if (rc == MPCX_OK && r.targets()) rc = check_one_or_per_instance(r.td, r.td ? r.td->map : nullptr, r.td ? r.td->map_batch : nullptr, bank, kTargetNouns);
    if (rc == MPCX_OK && r.offset_free() && dm.ndu == 0)
        rc = fail(MPCX_E_INVALID, "ndu = 0: the controller has no disturbance model (Bd, Dd) to estimate a disturbance with");
    return rc;
}

// Where step 0 of tick k's reference lies in an array of the given mode, n values a step: value(b, k, a) = src[b * bs + k * tick + a]
struct RefLayout { long bs, tick; };
static RefLayout ref_layout(int mode, long n, int ph, int ticks)
{
    switch (mode) {
    case MPCX_REF_SHARED: return {0, 0};
    case MPCX_REF_PER_INSTANCE: return {n, 0};
    case MPCX_REF_PER_STEP: return {ph * n, 0};
    default: return {(ticks + ph) * n, n};       // MPCX_REF_PREVIEW
    }
}

// The loop's private buffers, one allocation.  loop_slab runs twice over the same statements -- once without a base to size the slab, once with it to
// hand out the pointers -- so a buffer is named in one place.
extern "C++" struct LoopSlab {
    char *base = nullptr;
    size_t total = 0;
    template <typename T> T *take(size_t count)
    {
        const size_t at = total;
        total = (total + count * sizeof(T) + 255) / 256 * 256;
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
};

// What loop_build decides before it allocates anything
struct LoopPlan {
    mpcx_lmpc_t h;                               // the controller of a controller's loop; null: a bank's
    mpcx_dims dm;
    const mpcx_lmpc_loop_desc *d;
    bool observed, offset_free, targets;
    ObserverView o;                              // (observed)
    const mpcx_lmpc_disturbance_observer_desc *od;
    const mpcx_lmpc_target_desc *td;
    const double *ref_p[4]; int ref_m[4], ref_n[4];   // yref, uref, duref, dmeas: array, mode, values a step
    bool packed;                                 // a plant per instance: the caller's array; in a bank also the default, each instance's own controller
    bool own_d;                                  // a bank's "shared" exogenous input: each controller's own
    bool preview(int a) const                    // a preview array the solve sees through a staging window (dhat and us replace two of them)
    {
        return ref_m[a] == MPCX_REF_PREVIEW && ref_n[a] > 0 && !(offset_free && a == 3) && !(targets && a == 1);
    }
};

// the solve's buffers, which the loop reads (LmpcLoopDev has them const) and the step descriptor writes
struct LoopResults { double *cmd, *cost; int32_t *ints; uint32_t *sets; double *plant, *gain, *map; };

static void loop_slab(const LoopPlan &p, LoopSlab &s, mpcx::LmpcLoopDev &L, LoopResults &r)
{
    const mpcx_dims &dm = p.dm;
    const size_t B = (size_t)L.batch, aw = (size_t)L.aw;
    auto block = [&](mpcx::LoopBlock b) { return s.take<double>(mpcx::lmpc_loop_block_len(L, b)); };
    r.plant = s.take<double>((size_t)dm.nx * (dm.nx + dm.nu + dm.ndu));
    L.x = s.take<double>(B * dm.nx);
    L.u = s.take<double>(B * dm.nu);
    r.cmd = s.take<double>(B * dm.nu);
    r.cost = s.take<double>(B);
    r.ints = s.take<int32_t>(6 * B);             // status, solver status, feasibility, iterations, polish rounds, active count
    r.sets = s.take<uint32_t>(4 * B * aw);       // active lower and upper, warm lower and upper
    L.state = s.take<int>(2);
    for (int a = 0; a < 4; ++a)
        if (p.preview(a)) L.pv_dst[a] = s.take<double>(B * dm.ph * p.ref_n[a]);
    if (p.packed) L.pk = L.ok = block(mpcx::kPlantBlock);
    if (p.own_d) L.d_own = s.take<double>(B * dm.ndu);
    if (p.observed) {
        L.xt = s.take<double>(B * dm.nx);
        if (!p.packed) L.ok = block(mpcx::kPlantBlock);      // (one plant for the batch: one tile)
        L.ek = block(mpcx::kEstimatorBlock);
        L.mk = block(mpcx::kMeasurementBlock);
        if (p.o.gain) r.gain = s.take<double>((size_t)(dm.nx + (p.offset_free ? dm.ndu : 0)) * dm.ny);
    }
    if (p.offset_free) {                         // the estimate the solve reads, and Ld
        L.dhat = s.take<double>(B * dm.ndu);
        L.dk = block(mpcx::kDisturbanceGainBlock);
    }
    if (p.targets) {                             // the input reference the solve reads, and T
        L.us = s.take<double>(B * dm.nu);
        L.tk = block(mpcx::kTargetMapBlock);
        if (p.td->map) r.map = s.take<double>((size_t)dm.nu * (dm.ny + dm.ndu + dm.nu));
    }
}

// the one plant for the batch, row-major per matrix (the setters' and the descriptor's matrices are column-major), to the device
static int upload_plant(const LoopPlan &p, double *plant_d)
{
    const mpcx_dims &dm = p.dm;
    const double *Ah = p.d->plant_A, *Bh = p.d->plant_B, *Dh = p.d->plant_Bd;
    if (p.h) {                                   // what the descriptor leaves out is the controller's own
        const auto &c = p.h->ctl;
        if (!Ah) Ah = c.A.a.data();
        if (!Bh) Bh = c.B.a.data();
        if (!Dh) Dh = c.Bd.a.data();
    }
    const size_t plant_len = (size_t)dm.nx * (dm.nx + dm.nu + dm.ndu);
    std::vector<double> P(plant_len ? plant_len : 1);
    double *pa = P.data(), *pb = pa + (size_t)dm.nx * dm.nx, *pd = pb + (size_t)dm.nx * dm.nu;
    for (int i = 0; i < dm.nx; ++i) {
        for (int j = 0; j < dm.nx; ++j) pa[(size_t)i * dm.nx + j] = Ah[(size_t)j * dm.nx + i];
        for (int j = 0; j < dm.nu; ++j) pb[(size_t)i * dm.nu + j] = Bh[(size_t)j * dm.nx + i];
        for (int j = 0; j < dm.ndu; ++j) pd[(size_t)i * dm.ndu + j] = Dh[(size_t)j * dm.nx + i];
    }
    if (hipMemcpy(plant_d, P.data(), plant_len * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(MPCX_E_DEVICE, "upload of the plant failed");
    return MPCX_OK;
}

// an observed loop's model, gain and logs; an offset-free loop's on top
static int wire_observer(const LoopPlan &p, mpcx::LmpcLoopDev &L, const LoopResults &r)
{
    const mpcx_dims &dm = p.dm;
    if (p.h) { L.mA = p.h->dev.A; L.mB = p.h->dev.B; L.mBd = p.h->dev.Bd; L.mC = p.h->dev.C; L.mDd = p.h->dev.Dd; }
    if (p.o.gain) {
        const size_t gain_len = (size_t)(dm.nx + (p.offset_free ? dm.ndu : 0)) * dm.ny;
        if (hipMemcpy(r.gain, p.o.gain, gain_len * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(MPCX_E_DEVICE, "upload of the observer gain failed");
        L.gain = r.gain;
    }
    L.gain_batch = p.o.gain_batch; L.xhat0 = p.o.xhat0; L.meas_noise = p.o.meas_noise; L.traj_xhat = p.o.traj_xhat; L.traj_y = p.o.traj_y;
    if (p.offset_free) { L.dhat0 = p.od->dhat0; L.traj_dhat = p.od->traj_dhat; }
    return MPCX_OK;
}

// the map, and r_k and ubar_k: step 0 of the tick's yref and uref in whichever layout they have; "shared" is the controller's own (a bank: a null
// source, each instance's controller)
static int wire_targets(const LoopPlan &p, mpcx::LmpcLoopDev &L, const LoopResults &r)
{
    const mpcx_dims &dm = p.dm;
    if (p.td->map) {
        const size_t map_len = (size_t)dm.nu * (dm.ny + dm.ndu + dm.nu);
        if (hipMemcpy(r.map, p.td->map, map_len * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(MPCX_E_DEVICE, "upload of the target map failed");
        L.tmap = r.map;
    }
    L.tmap_batch = p.td->map_batch; L.traj_us = p.td->traj_us;
    const RefLayout yl = ref_layout(p.ref_m[0], dm.ny, dm.ph, L.ticks), ul = ref_layout(p.ref_m[1], dm.nu, dm.ph, L.ticks);
    L.r_src = p.ref_m[0] == MPCX_REF_SHARED ? (p.h ? p.h->dev.yref_s : nullptr) : p.ref_p[0]; L.r_bs = yl.bs; L.r_tick = yl.tick;
    L.ub_src = p.ref_m[1] == MPCX_REF_SHARED ? (p.h ? p.h->dev.uref_s : nullptr) : p.ref_p[1]; L.ub_bs = ul.bs; L.ub_tick = ul.tick;
    return MPCX_OK;
}

// The step's descriptor: the loop's own state, input and result buffers; a preview array is seen through its staging window, per step; an
// offset-free loop's exogenous input is the loop's own estimate and a loop with targets' input reference its own us (the descriptor's dmeas drives the
// plant alone and its uref is ubar, read by the loop's kernels: no windows)
static mpcx_lmpc_batch step_descriptor(const LoopPlan &p, mpcx::LmpcLoopDev &L, const LoopResults &r)
{
    const size_t B = (size_t)L.batch, aw = (size_t)L.aw;
    mpcx_lmpc_batch cold{};
    cold.batch = L.batch; cold.x0 = L.x; cold.u0 = L.u;
    const double *sp[4]; int sm[4];
    for (int a = 0; a < 4; ++a) {
        sp[a] = p.ref_p[a]; sm[a] = p.ref_m[a];
        if (p.offset_free && a == 3) { sp[a] = L.dhat; sm[a] = MPCX_REF_PER_INSTANCE; continue; }
        if (p.targets && a == 1) { sp[a] = L.us; sm[a] = MPCX_REF_PER_INSTANCE; continue; }
        if (p.ref_m[a] != MPCX_REF_PREVIEW) continue;
        if (p.ref_n[a] == 0) { sp[a] = nullptr; sm[a] = MPCX_REF_SHARED; continue; }      // (no exogenous inputs: nothing to preview)
        L.pv_src[a] = p.ref_p[a]; L.pv_n[a] = p.ref_n[a];
        sp[a] = L.pv_dst[a]; sm[a] = MPCX_REF_PER_STEP;
    }
    cold.yref = sp[0]; cold.yref_mode = sm[0]; cold.uref = sp[1]; cold.uref_mode = sm[1];
    cold.duref = sp[2]; cold.duref_mode = sm[2]; cold.dmeas = sp[3]; cold.dmeas_mode = sm[3];
    cold.cmd = r.cmd; cold.cost = r.cost;
    cold.status = r.ints; cold.solver_status = r.ints + B; cold.is_feasible = r.ints + 2 * B; cold.iterations = r.ints + 3 * B;
    cold.polish_rounds = r.ints + 4 * B; cold.active_count = r.ints + 5 * B;
    if (p.d->carry_working_set) { cold.active_lower = r.sets; cold.active_upper = r.sets + B * aw; }
    return cold;
}

// The loop of a controller (h) or of a bank (f, model_index), once the request and the owner's state have been checked and the owner is set up on
// the current device.  dm, active_words: the owner's.
static int loop_build(mpcx_lmpc_t h, mpcx_lmpc_hetero_t f, const int32_t *model_index, const mpcx_dims &dm, int active_words, const LoopRequest &rq)
{
    const mpcx_lmpc_loop_desc *d = rq.d;
    hipStream_t s = reinterpret_cast<hipStream_t>(rq.stream);
    std::unique_ptr<mpcx_lmpc_loop> l(new mpcx_lmpc_loop);
    l->owner = h; l->bank = f; l->model_index = model_index; l->ticks = d->ticks;
    if (h) { l->device = h->device; l->setups = h->n_full_setups; } else l->device = f->device;
    mpcx::LmpcLoopDev &L = l->L;

    // the plan: what kind of loop, which plant, which blocks differ from instance to instance
    LoopPlan p{};
    p.h = h; p.dm = dm; p.d = d;
    p.observed = rq.kind != LoopKind::Plain; p.offset_free = rq.offset_free(); p.targets = rq.targets();
    if (p.observed) p.o = p.offset_free ? observer_view(rq.od) : observer_view(rq.o);
    p.od = rq.od; p.td = rq.td;
    const double *const ref_p[4] = {d->yref, d->uref, d->duref, d->dmeas};
    const int ref_m[4] = {d->yref_mode, d->uref_mode, d->duref_mode, d->dmeas_mode}, ref_n[4] = {dm.ny, dm.nu, dm.nu, dm.ndu};
    for (int a = 0; a < 4; ++a) { p.ref_p[a] = ref_p[a]; p.ref_m[a] = ref_m[a]; p.ref_n[a] = ref_n[a]; }
    const bool uniform = d->plant_A || d->plant_B || d->plant_Bd;
    p.packed = d->plant_batch || (f && !uniform);
    p.own_d = f && dm.ndu > 0 && d->dmeas_mode == MPCX_REF_SHARED;
    L.batch = d->batch; L.ticks = d->ticks; L.nx = dm.nx; L.nu = dm.nu; L.ndu = dm.ndu; L.ph = dm.ph; L.aw = active_words; L.ny = dm.ny;
    L.dobs = p.offset_free ? 1 : 0; L.tgt = p.targets ? 1 : 0;
    mpcx::lmpc_loop_plan_lds(L);
    // a block is one tile (stride 0) where it is the same for every instance: one plant for the batch; a controller's own model with one gain (the
    // estimator and Ld); a controller's own outputs (the measurement); one map for the batch (T).  Else a tile per ipw instances
    auto stride = [&](mpcx::LoopBlock b, bool one_tile) { return one_tile ? 0L : (long)mpcx::lmpc_loop_tile_len(L, b); };
    const bool one_gain = h && p.observed && p.o.gain;
    L.ok_ts = stride(mpcx::kPlantBlock, !p.packed);
    L.ek_ts = stride(mpcx::kEstimatorBlock, one_gain);
    L.mk_ts = stride(mpcx::kMeasurementBlock, h != nullptr);
    L.dk_ts = stride(mpcx::kDisturbanceGainBlock, one_gain);
    L.tk_ts = stride(mpcx::kTargetMapBlock, p.targets && rq.td->map);

    // the slab: sized, allocated, handed out
    LoopSlab slab;
    LoopResults r{};
    loop_slab(p, slab, L, r);
    if (hipMalloc(reinterpret_cast<void **>(&l->slab), slab.total) != hipSuccess) { l->slab = nullptr; return fail(MPCX_E_DEVICE, "allocation of the loop's buffers failed"); }
    if (hipMemset(l->slab, 0, slab.total) != hipSuccess) return fail(MPCX_E_DEVICE, "hipMemset failed");
    slab.base = l->slab; slab.total = 0;
    loop_slab(p, slab, L, r);

    // the plant, the owner's models, the caller's arrays and logs
    const size_t B = (size_t)d->batch, aw = (size_t)active_words;
    int rc = MPCX_OK;
    if (p.packed) L.pk_src = d->plant_batch;
    else rc = upload_plant(p, r.plant);
    if (rc != MPCX_OK) return rc;
    if (f) { L.models = f->models_d; L.model_index = model_index; }
    L.plant = r.plant; L.x0 = d->x0; L.u0 = d->u0; L.noise = d->noise;
    L.cmd = r.cmd; L.cost = r.cost;
    L.status = r.ints; L.solver_status = r.ints + B; L.iterations = r.ints + 3 * B; L.polish_rounds = r.ints + 4 * B; L.active_count = r.ints + 5 * B;
    L.active_lower = r.sets; L.active_upper = r.sets + B * aw;
    if (d->carry_working_set) { L.warm_lower = r.sets + 2 * B * aw; L.warm_upper = r.sets + 3 * B * aw; }
    L.traj_x = d->traj_x; L.traj_u = d->traj_u; L.traj_cost = d->traj_cost;
    L.traj_status = d->traj_status; L.traj_solver_status = d->traj_solver_status; L.traj_iterations = d->traj_iterations;
    L.traj_polish_rounds = d->traj_polish_rounds; L.traj_active_count = d->traj_active_count;
    if (p.observed) rc = wire_observer(p, L, r);
    if (rc == MPCX_OK && p.targets) rc = wire_targets(p, L, r);
    if (rc != MPCX_OK) return rc;

    // the step's descriptors: tick 0 solves cold, the later ticks with the carried working sets
    const mpcx_lmpc_batch cold = step_descriptor(p, L, r);
    l->step = cold; l->plain = !p.observed;
    mpcx_lmpc_batch warm = cold;
    warm.warm_active_lower = L.warm_lower; warm.warm_active_upper = L.warm_upper; warm.warm_shift = 1;
    const bool two = d->carry_working_set && d->ticks > 1;

    // d_k, the sample that drives the plant: step 0 of the tick's exogenous input in whichever layout it has; a bank's "shared" is the per-instance
    // array the pack kernel fills
    if (dm.ndu > 0) {
        const RefLayout dl = ref_layout(p.own_d ? MPCX_REF_PER_INSTANCE : d->dmeas_mode, dm.ndu, dm.ph, d->ticks);
        L.dmeas = p.own_d ? L.d_own : d->dmeas_mode == MPCX_REF_SHARED ? h->dev.dmeas_s : d->dmeas;
        L.d_bs = dl.bs; L.d_tick = dl.tick;
    }

    // one plain pass first, as mpcx_lmpc_graph_create does: it sizes the workspace and configures the kernels, none of which can be captured; then
    // the capture
    const int pr = mpcx::lmpc_loop_prepare(L);
    if (pr != 0) return pr == -2 ? fail(MPCX_E_UNSUPPORTED, "the advance kernel's tiles exceed a compute unit's LDS") : fail(MPCX_E_DEVICE, "hipFuncSetAttribute failed");
    if (mpcx::lmpc_loop_begin(L, s) != 0) return fail(MPCX_E_DEVICE, "launch of the begin kernel failed");
    if (mpcx::lmpc_loop_pack_plants(L, s) != 0 || mpcx::lmpc_loop_pack_observer(L, s) != 0) return fail(MPCX_E_DEVICE, "launch of the pack kernel failed");
    rc = l->solve(&cold, s);
    if (rc == MPCX_OK && mpcx::lmpc_loop_advance(L, s) != 0) rc = fail(MPCX_E_DEVICE, "launch of the advance kernel failed");
    if (rc == MPCX_OK && two) rc = l->solve(&warm, s);
    if (rc != MPCX_OK) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(MPCX_E_DEVICE, "the warm-up ticks failed");
    rc = capture_tick(*l, &cold, s, &l->first);
    if (rc == MPCX_OK && two) rc = capture_tick(*l, &warm, s, &l->next);
    if (rc != MPCX_OK) return rc;
    *rq.out = l.release();
    return MPCX_OK;
}

// a controller's loop: its model must be set, it must live on a device, and it is set up before the loop is built
static int lmpc_loop_create(mpcx_lmpc_t h, const LoopRequest &r)
{
    CHECK_H(h);
    int rc = check_loop_request(r, false, h->ctl.d);
    if (rc != MPCX_OK) return rc;
    if (!h->ctl.have_model) return fail(MPCX_E_STATE, "state-space model not set");
    if (h->host_only) return fail(MPCX_E_STATE, "host-only handle: a loop runs on a HIP device");
    if (!r.stream) return fail(MPCX_E_INVALID, "a loop is captured on a non-default stream");
    rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    return loop_build(h, nullptr, nullptr, h->ctl.d, h->dev.active_words, r);
}

// a bank's loop (the bank is followed only behind a good descriptor)
static int hetero_loop_create(mpcx_lmpc_hetero_t f, const int32_t *model_index, const LoopRequest &r)
{
    if (!f) return fail(MPCX_E_INVALID, "null argument");
    const int rc = check_loop_request(r, true, f->d);
    if (rc != MPCX_OK) return rc;
    const mpcx_lmpc_loop_desc *d = r.d;
    if (!model_index && d->batch != f->count) return fail(MPCX_E_INVALID, "without a model index the batch must be the bank: instance b uses controller b");
    // a bank keeps no host copy of its controllers' models: there is no "the controller's own" to complete a one-for-all plant with
    if ((d->plant_A || d->plant_B || d->plant_Bd) && (!d->plant_A || !d->plant_B || (f->d.ndu > 0 && !d->plant_Bd)))
        return fail(MPCX_E_INVALID, "a bank's loop takes plant_A, plant_B and plant_Bd together (or plant_batch, or none: each instance's own controller)");
    if (!r.stream) return fail(MPCX_E_INVALID, "a loop is captured on a non-default stream");
    if (hipSetDevice(f->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    return loop_build(nullptr, f, model_index, f->d, f->active_words, r);
}

int mpcx_lmpc_loop_create(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, void *stream, mpcx_lmpc_loop_t *out)
{
    return lmpc_loop_create(h, {LoopKind::Plain, d, nullptr, nullptr, nullptr, stream, out});
}

int mpcx_lmpc_loop_create_observed(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_observer_desc *o, void *stream, mpcx_lmpc_loop_t *out)
{
    return lmpc_loop_create(h, {LoopKind::Observed, d, o, nullptr, nullptr, stream, out});
}

int mpcx_lmpc_loop_create_offset_free(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o, void *stream, mpcx_lmpc_loop_t *out)
{
    return lmpc_loop_create(h, {LoopKind::OffsetFree, d, nullptr, o, nullptr, stream, out});
}

int mpcx_lmpc_loop_create_offset_free_target(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o,
                                             const mpcx_lmpc_target_desc *t, void *stream, mpcx_lmpc_loop_t *out)
{
    return lmpc_loop_create(h, {LoopKind::OffsetFreeTarget, d, nullptr, o, t, stream, out});
}

int mpcx_lmpc_hetero_loop_create(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const int32_t *model_index, void *stream, mpcx_lmpc_loop_t *out)
{
    return hetero_loop_create(f, model_index, {LoopKind::Plain, d, nullptr, nullptr, nullptr, stream, out});
}

int mpcx_lmpc_hetero_loop_create_observed(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_observer_desc *o, const int32_t *model_index,
                                          void *stream, mpcx_lmpc_loop_t *out)
{
    return hetero_loop_create(f, model_index, {LoopKind::Observed, d, o, nullptr, nullptr, stream, out});
}

int mpcx_lmpc_hetero_loop_create_offset_free(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o,
                                             const int32_t *model_index, void *stream, mpcx_lmpc_loop_t *out)
{
    return hetero_loop_create(f, model_index, {LoopKind::OffsetFree, d, nullptr, o, nullptr, stream, out});
}

int mpcx_lmpc_hetero_loop_create_offset_free_target(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o,
                                                    const mpcx_lmpc_target_desc *t, const int32_t *model_index, void *stream, mpcx_lmpc_loop_t *out)
{
    return hetero_loop_create(f, model_index, {LoopKind::OffsetFreeTarget, d, nullptr, o, t, stream, out});
}

// Steady-state target maps and the product with them (include/mpcx.h; kernels in target_kernels.hip, declared in lmpc_device.hpp)
int mpcx_target_map_batch(int device, int nx, int nu, int ndu, int ny, int batch, const double *A, const double *B, const double *Bd, const double *C,
                          const double *Dd, double *map_u, double *map_x, int32_t *flags, void *stream)
{
    if (nx < 1 || nu < 1 || ny < 1 || ndu < 0) return fail(MPCX_E_INVALID, "need nx, nu, ny >= 1 and ndu >= 0");
    if (batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (!A || !B || !C || !map_u || (ndu > 0 && (!Bd || !Dd))) return fail(MPCX_E_INVALID, "A, B, C and map_u (with ndu > 0 also Bd and Dd) are required");
    if ((size_t)nx + nu + ny + ndu > 4096 || mpcx::target_map_lds_bytes(nx, nu, ndu, ny) > mpcx::lmpc_lds_limit())
        return fail(MPCX_E_UNSUPPORTED, "the augmented KKT matrix exceeds the LDS a workgroup may request");
    if (batch == 0) return MPCX_OK;
    if (hipSetDevice(device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    const int rc = mpcx::target_map_launch(nx, nu, ndu, ny, batch, A, B, Bd, C, Dd, map_u, map_x, flags, mpcx::lmpc_lds_limit(), stream);
    if (rc == -2) return fail(MPCX_E_UNSUPPORTED, "the augmented KKT matrix exceeds the LDS a workgroup may request");
    if (rc != 0) return fail(MPCX_E_DEVICE, "target map kernel launch failed");
    return MPCX_OK;
}

int mpcx_target_apply_batch(int device, int nu, int ndu, int ny, int batch, const double *map_u, int map_per_instance, const double *r,
                            const double *dhat, const double *ubar, double *us, void *stream)
{
    if (nu < 1 || ny < 1 || ndu < 0) return fail(MPCX_E_INVALID, "need nu, ny >= 1 and ndu >= 0");
    if (batch < 0) return fail(MPCX_E_INVALID, "negative batch");
    if (!map_u || !r || !ubar || !us || (ndu > 0 && !dhat)) return fail(MPCX_E_INVALID, "map_u, r, ubar and us (with ndu > 0 also dhat) are required");
    if (batch == 0) return MPCX_OK;
    if (hipSetDevice(device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (mpcx::target_apply_launch(nu, ndu, ny, batch, map_u, map_per_instance ? 1 : 0, r, dhat, ubar, us, stream) != 0)
        return fail(MPCX_E_DEVICE, "target product kernel launch failed");
    return MPCX_OK;
}

// The steady-state Kalman predictor gain of the controller's own (A, C) by Riccati iteration (include/mpcx.h), host doubles throughout.
int mpcx_lmpc_kalman_gain(mpcx_lmpc_t h, const double *Qw, const double *Rv, double *gain_out, double *P_out, int *iterations)
{
    CHECK_H(h);
    if (!Qw || !Rv || !gain_out) return fail(MPCX_E_INVALID, "Qw, Rv and gain_out are required");
    if (!h->ctl.have_model) return fail(MPCX_E_STATE, "state-space model not set");
    using mpcx::Mat;
    const int nx = h->ctl.d.nx, ny = h->ctl.d.ny;
    const Mat &A = h->ctl.A, &Cm = h->ctl.C;
    Mat Q(nx, nx), R(ny, ny);
    std::memcpy(Q.a.data(), Qw, Q.a.size() * sizeof(double));
    std::memcpy(R.a.data(), Rv, R.a.size() * sizeof(double));
    auto symmetric = [](const Mat &M) {
        double big = 0.0, skew = 0.0;
        for (int j = 0; j < M.c; ++j)
            for (int i = 0; i < M.r; ++i) { big = std::max(big, std::fabs(M(i, j))); skew = std::max(skew, std::fabs(M(i, j) - M(j, i))); }
        return std::isfinite(big) && skew <= 1e-12 * big;
    };
    if (!symmetric(Q)) return fail(MPCX_E_INVALID, "Qw is not symmetric");
    if (!symmetric(R)) return fail(MPCX_E_INVALID, "Rv is not symmetric");
    { Mat Rc = R; if (!(mpcx::cholesky_lower(Rc) > 0.0)) return fail(MPCX_E_INVALID, "Rv is not positive definite"); }
    const Mat At = mpcx::transpose(A), Ct = mpcx::transpose(Cm);
    // K = A P C', S = C P C' + Rv, gain = K S^-1 (S symmetric positive definite: by its Cholesky factor, row by row of K)
    auto gain_of = [&](const Mat &P, Mat &K, Mat &G) {
        const Mat PCt = mpcx::matmul(P, Ct);
        K = mpcx::matmul(A, PCt);
        Mat S = mpcx::matmul(Cm, PCt);
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < ny; ++i) S(i, j) = 0.5 * (S(i, j) + S(j, i)) + R(i, j);
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < j; ++i) S(i, j) = S(j, i);
        if (!(mpcx::cholesky_lower(S) > 0.0)) return false;
        G = Mat(nx, ny);
        std::vector<double> z(ny);
        for (int r = 0; r < nx; ++r) {           // S g = k for row r of K: forward with the factor, back with its transpose
            for (int i = 0; i < ny; ++i) { double v = K(r, i); for (int j = 0; j < i; ++j) v -= S(i, j) * z[j]; z[i] = v / S(i, i); }
            for (int i = ny - 1; i >= 0; --i) { double v = z[i]; for (int j = i + 1; j < ny; ++j) v -= S(j, i) * z[j]; z[i] = v / S(i, i); }
            for (int i = 0; i < ny; ++i) G(r, i) = z[i];
        }
        return true;
    };
    constexpr int kMaxRiccati = 100000;
    Mat P = Q, K, G;
    int it = 0;
    bool converged = false;
    for (; it < kMaxRiccati && !converged; ++it) {
        if (!gain_of(P, K, G)) return fail(MPCX_E_NUMERIC, "C P C' + Rv does not factor");
        Mat Pn = mpcx::matmul(mpcx::matmul(A, P), At);
        const Mat GKt = mpcx::matmul(G, mpcx::transpose(K));
        for (size_t e = 0; e < Pn.a.size(); ++e) Pn.a[e] += Q.a[e] - GKt.a[e];
        double big = 0.0, change = 0.0;
        bool finite = true;
        for (int j = 0; j < nx; ++j)
            for (int i = 0; i <= j; ++i) {
                const double v = 0.5 * (Pn(i, j) + Pn(j, i));
                Pn(i, j) = v; Pn(j, i) = v;
                finite = finite && std::isfinite(v);
                big = std::max(big, std::fabs(v));
                change = std::max(change, std::fabs(v - P(i, j)));
            }
        if (!finite) return fail(MPCX_E_NUMERIC, "the Riccati iteration diverged: is (A, C) detectable?");
        converged = change <= 1e-14 * big;
        P = Pn;
    }
    if (iterations) *iterations = it;
    if (!converged) return fail(MPCX_E_NUMERIC, "the Riccati iteration has not converged after 100000 steps: is (A, C) detectable?");
    if (!gain_of(P, K, G)) return fail(MPCX_E_NUMERIC, "C P C' + Rv does not factor");
    std::memcpy(gain_out, G.a.data(), G.a.size() * sizeof(double));
    if (P_out) std::memcpy(P_out, P.a.data(), P.a.size() * sizeof(double));
    return MPCX_OK;
}

static int loop_usable(mpcx_lmpc_loop_t l)
{
    if (!l || !l->first) return fail(MPCX_E_INVALID, "null loop");
    const mpcx_lmpc_t h = l->owner;              // (a bank has no setters: nothing can have changed)
    if (h && (h->dirty || h->refs_dirty || h->n_full_setups != l->setups))
        return fail(MPCX_E_STATE, "the controller changed since the loop was created: create a new loop");
    if (hipSetDevice(l->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    return MPCX_OK;
}

int mpcx_lmpc_loop_run(mpcx_lmpc_loop_t l, void *stream)
{
    int rc = loop_usable(l);
    if (rc != MPCX_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mpcx::lmpc_loop_begin(l->L, stream) != 0) return fail(MPCX_E_DEVICE, "launch of the begin kernel failed");
    if (mpcx::lmpc_loop_pack_plants(l->L, stream) != 0 || mpcx::lmpc_loop_pack_observer(l->L, stream) != 0) return fail(MPCX_E_DEVICE, "launch of the pack kernel failed");
    for (int k = 0; k < l->ticks; ++k)
        if (hipGraphLaunch(k > 0 && l->next ? l->next : l->first, s) != hipSuccess) return fail(MPCX_E_DEVICE, "hipGraphLaunch failed");
    return MPCX_OK;
}

int mpcx_lmpc_loop_debug_replay(mpcx_lmpc_loop_t l, void *stream)
{
    int rc = loop_usable(l);
    if (rc != MPCX_OK) return rc;
    if (hipGraphLaunch(l->next ? l->next : l->first, reinterpret_cast<hipStream_t>(stream)) != hipSuccess) return fail(MPCX_E_DEVICE, "hipGraphLaunch failed");
    return MPCX_OK;
}

int mpcx_lmpc_loop_debug_tick(mpcx_lmpc_loop_t l, int *tick)
{
    if (!l || !tick) return fail(MPCX_E_INVALID, "null argument");
    if (hipSetDevice(l->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(tick, l->L.state, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MPCX_E_DEVICE, "reading the tick counter failed");
    return MPCX_OK;
}

int mpcx_lmpc_loop_destroy(mpcx_lmpc_loop_t l)
{
    if (!l) return MPCX_OK;
    (void)hipSetDevice(l->device);
    delete l;
    return MPCX_OK;
}

// ---- the backward pass of the plain closed loop ---------------------------------------------------------------------
// A backward tick is the owner's cold solve on the loop's own x / u buffers (staged from the trajectories by the begin and adjoint kernels), the VJP
// launch seeded with the handle's c buffer, where asked for the weight and model launches (reduce = 0, into per-tick buffers), and
// lmpc_loop_grad_adjoint; captured once as a linear chain on one stream.  A run is "begin kernel, the tick graph `ticks` times, finish kernel,
// and with reduce = 1 the ordered sums".
struct mpcx_lmpc_loop_grad {
    mpcx_lmpc_loop_t loop = nullptr;
    int device = 0;
    mpcx::LmpcLoopGradDev G{};
    mpcx::LmpcLoopGradSum sums[2] = {};          // reduce = 1: plant and weights; the model
    bool sum[2] = {false, false};
    hipGraphExec_t tick = nullptr;
    char *slab = nullptr;
    // what the tick's launches are given: the descriptors live as long as the handle (the weight and model descriptors point to `solve`)
    mpcx_lmpc_batch solve{};
    mpcx_lmpc_sens sens{};
    mpcx_lmpc_param_sens param{};
    mpcx_lmpc_model_sens model{};
    bool want_param = false, want_model = false;
    ~mpcx_lmpc_loop_grad()
    {
        if (tick) (void)hipGraphExecDestroy(tick);
        if (slab) (void)hipFree(slab);
    }
    // the launches of one backward tick on `s`
    int chain(void *s) const
    {
        int rc = mpcx_lmpc_solve_batch(loop->owner, &solve, s);
        if (rc == MPCX_OK) rc = mpcx_lmpc_sensitivity_batch(loop->owner, &sens, s);
        if (rc == MPCX_OK && want_param) rc = mpcx_lmpc_param_sensitivity_batch(loop->owner, &param, s);
        if (rc == MPCX_OK && want_model) rc = mpcx_lmpc_model_sensitivity_batch(loop->owner, &model, s);
        if (rc == MPCX_OK && mpcx::lmpc_loop_grad_adjoint(G, s) != 0) rc = fail(MPCX_E_DEVICE, "launch of the adjoint kernel failed");
        return rc;
    }
};

int mpcx_lmpc_loop_grad_desc_size(void) { return (int)sizeof(mpcx_lmpc_loop_grad_desc); }

int mpcx_lmpc_loop_grad_create(mpcx_lmpc_loop_t l, const mpcx_lmpc_loop_grad_desc *d, void *stream, mpcx_lmpc_loop_grad_t *out)
{
    if (!l || !out) return fail(MPCX_E_INVALID, "null argument");
    if (!d) return fail(MPCX_E_INVALID, "null gradient descriptor");
    if (!d->seed_x && !d->seed_u) return fail(MPCX_E_INVALID, "a loop gradient needs seed_x or seed_u");
    if (d->reduce != 0 && d->reduce != 1) return fail(MPCX_E_INVALID, "reduce must be 0 or 1");
    if (l->bank) return fail(MPCX_E_INVALID, "a bank's loop has no backward pass yet (a follow-up): create the gradient on a controller's plain loop");
    if (!l->plain) return fail(MPCX_E_INVALID, "an observed, offset-free or target loop has no backward pass yet (a follow-up): the estimator's adjoint is not built");
    if (!stream) return fail(MPCX_E_INVALID, "a loop gradient is captured on a non-default stream");
    int rc = loop_usable(l);
    if (rc != MPCX_OK) return rc;
    mpcx_lmpc_t h = l->owner;
    const mpcx::LmpcLoopDev &L = l->L;
    const mpcx_dims &dm = h->ctl.d;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::unique_ptr<mpcx_lmpc_loop_grad> g(new mpcx_lmpc_loop_grad);
    g->loop = l; g->device = l->device;
    mpcx::LmpcLoopGradDev &G = g->G;
    G.batch = L.batch; G.ticks = L.ticks; G.nx = L.nx; G.nu = L.nu; G.ndu = L.ndu; G.ny = L.ny; G.ph = L.ph; G.ipw = L.ipw;
    mpcx::lmpc_loop_grad_plan_lds(G);
    G.plant = L.plant; G.pk = L.pk; G.traj_x = L.traj_x; G.traj_u = L.traj_u; G.u0 = L.u0;
    G.dmeas = L.dmeas; G.d_bs = L.d_bs; G.d_tick = L.d_tick; G.x = L.x; G.u = L.u;
    for (int a = 0; a < 4; ++a) { G.pv_src[a] = L.pv_src[a]; G.pv_dst[a] = L.pv_dst[a]; G.pv_n[a] = L.pv_n[a]; }
    G.seed_x = d->seed_x; G.seed_u = d->seed_u;
    G.d_noise = d->d_noise; G.d_x0 = d->d_x0; G.d_u0 = d->d_u0; G.a_yref = d->d_yref;

    // the slots: the three weights, the five matrices (Bd and Dd only with exogenous inputs)
    const size_t B = (size_t)L.batch;
    const int nx = dm.nx, nu = dm.nu, ndu = dm.ndu, ny = dm.ny, ph = dm.ph;
    double *const user[mpcx::kLoopGradSlots] = {d->d_oweight, d->d_uweight, d->d_duweight, d->d_A, d->d_B, d->d_C, ndu > 0 ? d->d_Bd : nullptr, ndu > 0 ? d->d_Dd : nullptr};
    const int len[mpcx::kLoopGradSlots] = {ny * ph, nu * ph, nu * ph, nx * nx, nx * nu, ny * nx, nx * ndu, ny * ndu};
    const int plen = nx * (nx + nu + ndu);
    g->want_param = user[0] || user[1] || user[2];
    g->want_model = user[3] || user[4] || user[5] || user[6] || user[7];
    const bool seq = g->want_param || g->want_model;
    const bool reduce = d->reduce == 1;

    // the handle's buffers, one allocation (LoopSlab: sized in a first pass, handed out in a second)
    double *tick_out[mpcx::kLoopGradSlots] = {}, *acc[mpcx::kLoopGradSlots] = {}, *a_plant = nullptr, *gx = nullptr, *gu = nullptr, *gy = nullptr;
    double *seq_state = nullptr, *seq_output = nullptr, *seq_input = nullptr, *part[2] = {nullptr, nullptr};
    int32_t *tflags = nullptr, *flags = nullptr;
    auto carve = [&](LoopSlab &sl) {
        G.lam = sl.take<double>(B * nx); G.mu = sl.take<double>(B * nu); G.c = sl.take<double>(B * nu);
        gx = sl.take<double>(B * nx); gu = sl.take<double>(B * nu); gy = sl.take<double>(B * ny);
        tflags = sl.take<int32_t>(3 * B);
        flags = d->flags ? d->flags : sl.take<int32_t>(B);
        G.state = sl.take<int>(2);
        for (int k = 0; k < mpcx::kLoopGradSlots; ++k) {
            if (!user[k]) continue;
            tick_out[k] = sl.take<double>(B * len[k]);
            acc[k] = reduce ? sl.take<double>(B * len[k]) : user[k];
        }
        if (d->d_plant) a_plant = reduce ? sl.take<double>(B * plen) : d->d_plant;
        if (seq) {
            seq_state = sl.take<double>(B * (ph + 1) * nx); seq_output = sl.take<double>(B * (ph + 1) * ny); seq_input = sl.take<double>(B * (ph + 1) * nu);
        }
        if (reduce) {
            const size_t groups = mpcx::lmpc_loop_grad_groups(L.batch);
            part[0] = sl.take<double>(groups * (size_t)(1 + plen + len[0] + len[1] + len[2]));
            part[1] = sl.take<double>(groups * (size_t)(1 + len[3] + len[4] + len[5] + len[6] + len[7]));
        }
    };
    LoopSlab slab;
    carve(slab);
    if (hipSetDevice(g->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (hipMalloc(reinterpret_cast<void **>(&g->slab), slab.total) != hipSuccess) { g->slab = nullptr; return fail(MPCX_E_DEVICE, "allocation of the gradient's buffers failed"); }
    if (hipMemset(g->slab, 0, slab.total) != hipSuccess) return fail(MPCX_E_DEVICE, "hipMemset failed");
    slab.base = g->slab; slab.total = 0;
    carve(slab);
    G.gx = gx; G.gu = gu; G.gy = gy; G.tflags = tflags; G.flags = flags; G.a_plant = a_plant;
    G.ntf = 1 + (g->want_param ? 1 : 0) + (g->want_model ? 1 : 0);
    for (int k = 0; k < mpcx::kLoopGradSlots; ++k) { G.tick_out[k] = tick_out[k]; G.acc[k] = acc[k]; G.len[k] = len[k]; }

    // the tick's descriptors: the loop's cold step with its active sets (the loop's own buffers, carried or not) and, for weights and model, sequences
    g->solve = l->step;
    g->solve.active_lower = const_cast<uint32_t *>(L.active_lower); g->solve.active_upper = const_cast<uint32_t *>(L.active_upper);
    g->solve.warm_active_lower = g->solve.warm_active_upper = nullptr; g->solve.warm_shift = 0;
    g->solve.seq_state = seq_state; g->solve.seq_output = seq_output; g->solve.seq_input = seq_input;
    g->sens.batch = L.batch; g->sens.active_lower = L.active_lower; g->sens.active_upper = L.active_upper; g->sens.status = g->solve.status;
    g->sens.mode = MPCX_SENS_VJP; g->sens.seed_cmd = G.c;
    g->sens.d_x0 = gx; g->sens.d_u0 = gu; g->sens.d_yref = gy; g->sens.flags = tflags;
    int row = 1;
    if (g->want_param) {
        g->param.solved = &g->solve; g->param.seed_cmd = G.c; g->param.reduce = 0;
        g->param.d_oweight = tick_out[0]; g->param.d_uweight = tick_out[1]; g->param.d_duweight = tick_out[2];
        g->param.flags = tflags + B * row++;
    }
    if (g->want_model) {
        g->model.solved = &g->solve; g->model.seed_cmd = G.c; g->model.reduce = 0;
        g->model.d_A = tick_out[3]; g->model.d_B = tick_out[4]; g->model.d_C = tick_out[5]; g->model.d_Bd = tick_out[6]; g->model.d_Dd = tick_out[7];
        g->model.flags = tflags + B * row++;
        rc = mpcx_lmpc_model_sens_reserve(h, 0);     // the model launch's operand, outside the capture
        if (rc != MPCX_OK) return rc;
    }
    if (reduce) {
        mpcx::LmpcLoopGradSum &s0 = g->sums[0], &s1 = g->sums[1];
        s0.src[0] = a_plant; s0.dst[0] = d->d_plant; s0.len[0] = a_plant ? plen : 0;
        for (int k = 0; k < 3; ++k) { s0.src[1 + k] = acc[k]; s0.dst[1 + k] = user[k]; s0.len[1 + k] = acc[k] ? len[k] : 0; }
        for (int k = 0; k < 5; ++k) { s1.src[k] = acc[3 + k]; s1.dst[k] = user[3 + k]; s1.len[k] = acc[3 + k] ? len[3 + k] : 0; }
        s0.flags = s1.flags = flags; s0.batch = s1.batch = L.batch;
        s0.part = part[0]; s1.part = part[1];
        s0.n_used = d->n_used; s1.n_used = nullptr;
        g->sum[0] = a_plant || g->want_param || d->n_used; g->sum[1] = g->want_model;
    }

    // one plain backward tick first (it configures the kernels, which cannot be captured), then the capture
    const int pr = mpcx::lmpc_loop_grad_prepare(G);
    if (pr != 0) return pr == -2 ? fail(MPCX_E_UNSUPPORTED, "the adjoint kernel's tiles exceed a compute unit's LDS") : fail(MPCX_E_DEVICE, "hipFuncSetAttribute failed");
    if (mpcx::lmpc_loop_grad_begin(G, s) != 0) return fail(MPCX_E_DEVICE, "launch of the begin kernel failed");
    rc = g->chain(s);
    if (rc != MPCX_OK) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(MPCX_E_DEVICE, "the warm-up backward tick failed");
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return fail(MPCX_E_DEVICE, "hipStreamBeginCapture failed");
    rc = g->chain(s);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc == MPCX_OK && (ec != hipSuccess || !graph)) rc = fail(MPCX_E_DEVICE, "hipStreamEndCapture failed");
    if (rc == MPCX_OK && hipGraphInstantiate(&g->tick, graph, nullptr, nullptr, 0) != hipSuccess) rc = fail(MPCX_E_DEVICE, "hipGraphInstantiate failed");
    if (graph) (void)hipGraphDestroy(graph);
    if (rc != MPCX_OK) return rc;
    *out = g.release();
    return MPCX_OK;
}

int mpcx_lmpc_loop_grad_run(mpcx_lmpc_loop_grad_t g, void *stream)
{
    if (!g || !g->tick) return fail(MPCX_E_INVALID, "null loop gradient");
    int rc = loop_usable(g->loop);
    if (rc != MPCX_OK) return rc;
    // (the weight and model launches differentiate "the batch this handle solved last": every tick's re-solve is that batch when they run)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mpcx::lmpc_loop_grad_begin(g->G, stream) != 0) return fail(MPCX_E_DEVICE, "launch of the begin kernel failed");
    for (int k = 0; k < g->G.ticks; ++k)
        if (hipGraphLaunch(g->tick, s) != hipSuccess) return fail(MPCX_E_DEVICE, "hipGraphLaunch failed");
    if (mpcx::lmpc_loop_grad_finish(g->G, stream) != 0) return fail(MPCX_E_DEVICE, "launch of the finish kernel failed");
    for (int k = 0; k < 2; ++k)
        if (g->sum[k] && mpcx::lmpc_loop_grad_sum(g->sums[k], stream) != 0) return fail(MPCX_E_DEVICE, "launch of the ordered sums failed");
    return MPCX_OK;
}

int mpcx_lmpc_loop_grad_destroy(mpcx_lmpc_loop_grad_t g)
{
    if (!g) return MPCX_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return MPCX_OK;
}

int mpcx_lmpc_solve_host(mpcx_lmpc_t h, int batch, const double *x0, const double *u0,
                         double *cmd, double *cost, int32_t *status, int32_t *solver_status, int32_t *is_feasible,
                         double *seq_state, double *seq_output, double *seq_input)
{
    CHECK_H(h);
    if (batch < 0 || (batch > 0 && (!x0 || !u0 || !cmd))) return fail(MPCX_E_INVALID, "x0, u0 and cmd are required");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the solve path needs a HIP device, there is no CPU fallback");
    if (batch == 0) return MPCX_OK;
    int rc = mpcx_lmpc_setup(h);                 // active_words below comes from the condensed model
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    const auto &d = h->ctl.d;
    const size_t B = (size_t)batch, n1 = (size_t)d.ph + 1, aw = (size_t)h->dev.active_words;
    const size_t per = d.nx + d.nu + d.nu + 1 + n1 * (d.nx + d.ny + d.nu);
    if (B > h->stage_cap) {                       // staging buffers live in the handle: no allocation in the steady state
        h->release_staging();
        if (hipMalloc(reinterpret_cast<void **>(&h->stage_d), B * per * sizeof(double)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&h->stage_i), B * 4 * sizeof(int32_t)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&h->stage_act), B * 4 * aw * sizeof(uint32_t)) != hipSuccess) {
            h->release_staging();
            return fail(MPCX_E_DEVICE, "staging allocation failed");
        }
        h->stage_cap = B;
    }
    double *dx0 = h->stage_d, *du0 = dx0 + B * d.nx, *dcmd = du0 + B * d.nu, *dcost = dcmd + B * d.nu;
    double *dss = dcost + B, *dso = dss + B * n1 * d.nx, *dsi = dso + B * n1 * d.ny;
    int32_t *ibuf = h->stage_i;
    if (hipMemcpy(dx0, x0, B * d.nx * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(du0, u0, B * d.nu * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MPCX_E_DEVICE, "copy of x0 / u0 to the device failed");
    mpcx_lmpc_batch b{};
    b.batch = batch; b.x0 = dx0; b.u0 = du0;
    b.cmd = dcmd; b.cost = dcost;
    b.status = ibuf; b.solver_status = ibuf + B; b.is_feasible = ibuf + 2 * B; b.iterations = ibuf + 3 * B;
    const bool want_seq = seq_state || seq_output || seq_input;
    if (want_seq) { b.seq_state = dss; b.seq_output = dso; b.seq_input = dsi; }
    // LParameters::enable_warm_start (LOptimizer.hpp:268-281, LMPC.hpp:677-722): the reference re-uses the previous call's
    // primal / dual pair; what carries over here is the previous call's active set, shifted one step (receding horizon).
    // Two pairs of bitmaps alternate between "previous" and "current".
    if (h->ctl.prm.enable_warm_start) {
        uint32_t *cur = h->stage_act, *prev = h->stage_act + 2 * B * aw;
        if (h->warm_batch == batch) {
            if (hipMemcpy(prev, cur, 2 * B * aw * sizeof(uint32_t), hipMemcpyDeviceToDevice) != hipSuccess)
                return fail(MPCX_E_DEVICE, "device copy failed");
            b.warm_active_lower = prev; b.warm_active_upper = prev + B * aw; b.warm_shift = 1;
        }
    }
    // the active sets of this call stay on the device: the next call's warm start reads them, and so does mpcx_lmpc_sensitivity_host
    b.active_lower = h->stage_act; b.active_upper = h->stage_act + B * aw;
    h->sens_batch = 0;
    rc = mpcx_lmpc_solve_batch(h, &b, nullptr);
    if (rc == MPCX_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(MPCX_E_DEVICE, "kernel execution failed");
    h->warm_batch = (rc == MPCX_OK && h->ctl.prm.enable_warm_start) ? batch : 0;
    h->sens_batch = rc == MPCX_OK ? batch : 0;
    h->sens_has_seq = want_seq;
    if (rc == MPCX_OK) {
        bool ok = true;
        auto back = [&](void *dst, const void *src, size_t bytes) { if (dst) ok = ok && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
        back(cmd, dcmd, B * d.nu * sizeof(double)); back(cost, dcost, B * sizeof(double));
        back(status, ibuf, B * sizeof(int32_t)); back(solver_status, ibuf + B, B * sizeof(int32_t)); back(is_feasible, ibuf + 2 * B, B * sizeof(int32_t));
        back(seq_state, dss, B * n1 * d.nx * sizeof(double)); back(seq_output, dso, B * n1 * d.ny * sizeof(double));
        back(seq_input, dsi, B * n1 * d.nu * sizeof(double));
        if (!ok) rc = fail(MPCX_E_DEVICE, "copy of the results to the host failed");
    }
    return rc;
}

int mpcx_lmpc_sensitivity_host(mpcx_lmpc_t h, double *d_x0, double *d_u0, double *d_yref, int32_t *flags)
{
    CHECK_H(h);
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the sensitivity kernel needs a HIP device, there is no CPU fallback");
    if (h->sens_batch <= 0 || h->dirty) return fail(MPCX_E_STATE, "no solve to differentiate: call mpcx_lmpc_solve_host first (and after any change of the controller)");
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    const auto &d = h->ctl.d;
    const size_t B = (size_t)h->sens_batch, aw = (size_t)h->dev.active_words, nin = (size_t)d.nx + d.nu + d.ny;
    const size_t per = (size_t)d.nu * nin + 1;           // the three Jacobians, and room for the flag
    if (B > h->sens_stage_cap) {
        if (h->sens_stage) (void)hipFree(h->sens_stage);
        h->sens_stage = nullptr; h->sens_stage_cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&h->sens_stage), B * per * sizeof(double)) != hipSuccess) return fail(MPCX_E_DEVICE, "staging allocation failed");
        h->sens_stage_cap = B;
    }
    double *kx = h->sens_stage, *ku = kx + B * d.nu * d.nx, *ky = ku + B * d.nu * d.nu;
    int32_t *fl = reinterpret_cast<int32_t *>(ky + B * d.nu * d.ny);
    mpcx_lmpc_sens s{};
    s.batch = h->sens_batch; s.active_lower = h->stage_act; s.active_upper = h->stage_act + B * aw; s.status = h->stage_i;
    s.mode = MPCX_SENS_JACOBIAN; s.d_x0 = kx; s.d_u0 = ku; s.d_yref = ky; s.flags = fl;
    int rc = mpcx_lmpc_sensitivity_batch(h, &s, nullptr);
    if (rc == MPCX_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(MPCX_E_DEVICE, "kernel execution failed");
    if (rc != MPCX_OK) return rc;
    bool ok = true;
    auto back = [&](void *dst, const void *src, size_t bytes) { if (dst) ok = ok && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    back(d_x0, kx, B * d.nu * d.nx * sizeof(double)); back(d_u0, ku, B * d.nu * d.nu * sizeof(double)); back(d_yref, ky, B * d.nu * d.ny * sizeof(double));
    back(flags, fl, B * sizeof(int32_t));
    return ok ? MPCX_OK : fail(MPCX_E_DEVICE, "copy of the results to the host failed");
}

int mpcx_lmpc_param_sensitivity_host(mpcx_lmpc_t h, const double *seed_cmd, const double *seed_input, int reduce,
                                     double *d_oweight, double *d_uweight, double *d_duweight, double *d_lower, double *d_upper, int32_t *flags, int32_t *n_used)
{
    CHECK_H(h);
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the parameter-sensitivity kernel needs a HIP device, there is no CPU fallback");
    if (h->sens_batch <= 0 || h->dirty || h->refs_dirty || !h->sens_has_seq || h->solved_full != h->n_full_setups || h->solved_refs != h->n_ref_refreshes)
        return fail(MPCX_E_STATE, "no solve to differentiate: call mpcx_lmpc_solve_host with its sequences first (and after any change of the controller)");
    if (!seed_cmd && !seed_input) return fail(MPCX_E_INVALID, "a parameter sensitivity needs seed_cmd or seed_input");
    if (reduce != 0 && reduce != 1) return fail(MPCX_E_INVALID, "reduce must be 0 or 1");
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    const auto &d = h->ctl.d;
    const size_t B = (size_t)h->sens_batch, aw = (size_t)h->dev.active_words, n1 = (size_t)d.ph + 1, mr = (size_t)h->dev.m_ref;
    const size_t nw = (size_t)(d.ny + 2 * d.nu) * d.ph, nseed = (size_t)d.nu + n1 * d.nu;
    const size_t per = nseed + nw + 2 * mr + 2;           // seeds, the five outputs, and room for flag and count
    if (B * per > h->param_stage_cap) {
        if (h->param_stage) (void)hipFree(h->param_stage);
        h->param_stage = nullptr; h->param_stage_cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&h->param_stage), B * per * sizeof(double)) != hipSuccess) return fail(MPCX_E_DEVICE, "staging allocation failed");
        h->param_stage_cap = B * per;
    }
    int rc = reduce ? mpcx_lmpc_param_sens_reserve(h, h->sens_batch) : MPCX_OK;
    if (rc != MPCX_OK) return rc;
    double *sc = h->param_stage, *si = sc + B * d.nu, *gow = si + B * n1 * d.nu, *guw = gow + B * d.ny * d.ph, *gdw = guw + B * d.nu * d.ph;
    double *glo = gdw + B * d.nu * d.ph, *gup = glo + B * mr;
    int32_t *fl = reinterpret_cast<int32_t *>(gup + B * mr), *nu_ = fl + B;
    if ((seed_cmd && hipMemcpy(sc, seed_cmd, B * d.nu * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) ||
        (seed_input && hipMemcpy(si, seed_input, B * n1 * d.nu * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
        return fail(MPCX_E_DEVICE, "copy of the seeds to the device failed");
    // the batch mpcx_lmpc_solve_host solved, where it left it: the staging buffers' layout of that function
    double *dx0 = h->stage_d, *du0 = dx0 + B * d.nx, *dcmd = du0 + B * d.nu, *dcost = dcmd + B * d.nu;
    double *dss = dcost + B, *dso = dss + B * n1 * d.nx, *dsi = dso + B * n1 * d.ny;
    mpcx_lmpc_batch b{};
    b.batch = h->sens_batch; b.x0 = dx0; b.u0 = du0; b.cmd = dcmd; b.status = h->stage_i;
    b.active_lower = h->stage_act; b.active_upper = h->stage_act + B * aw; b.seq_output = dso; b.seq_input = dsi;
    mpcx_lmpc_param_sens s{};
    s.solved = &b; s.seed_cmd = seed_cmd ? sc : nullptr; s.seed_input = seed_input ? si : nullptr; s.reduce = reduce;
    s.d_oweight = gow; s.d_uweight = guw; s.d_duweight = gdw; s.d_lower = glo; s.d_upper = gup; s.flags = fl; s.n_used = nu_;
    rc = mpcx_lmpc_param_sensitivity_batch(h, &s, nullptr);
    if (rc == MPCX_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(MPCX_E_DEVICE, "kernel execution failed");
    if (rc != MPCX_OK) return rc;
    const size_t lead = reduce ? 1 : B;
    bool ok = true;
    auto back = [&](void *dst, const void *src, size_t bytes) { if (dst) ok = ok && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    back(d_oweight, gow, lead * d.ny * d.ph * sizeof(double)); back(d_uweight, guw, lead * d.nu * d.ph * sizeof(double));
    back(d_duweight, gdw, lead * d.nu * d.ph * sizeof(double)); back(d_lower, glo, lead * mr * sizeof(double)); back(d_upper, gup, lead * mr * sizeof(double));
    back(flags, fl, B * sizeof(int32_t));
    if (reduce) back(n_used, nu_, sizeof(int32_t));
    return ok ? MPCX_OK : fail(MPCX_E_DEVICE, "copy of the results to the host failed");
}

int mpcx_lmpc_model_sensitivity_host(mpcx_lmpc_t h, const double *seed_cmd, const double *seed_input, int reduce,
                                     double *d_A, double *d_B, double *d_C, double *d_Bd, double *d_Dd, int32_t *flags, int32_t *n_used)
{
    CHECK_H(h);
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle: the model-sensitivity kernel needs a HIP device, there is no CPU fallback");
    if (h->sens_batch <= 0 || h->dirty || h->refs_dirty || !h->sens_has_seq || h->solved_full != h->n_full_setups || h->solved_refs != h->n_ref_refreshes)
        return fail(MPCX_E_STATE, "no solve to differentiate: call mpcx_lmpc_solve_host with its sequences first (and after any change of the controller)");
    if (!seed_cmd && !seed_input) return fail(MPCX_E_INVALID, "a model sensitivity needs seed_cmd or seed_input");
    if (reduce != 0 && reduce != 1) return fail(MPCX_E_INVALID, "reduce must be 0 or 1");
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    const auto &d = h->ctl.d;
    const size_t B = (size_t)h->sens_batch, aw = (size_t)h->dev.active_words, n1 = (size_t)d.ph + 1;
    const size_t nA = (size_t)d.nx * d.nx, nB = (size_t)d.nx * d.nu, nC = (size_t)d.ny * d.nx, nBd = (size_t)d.nx * d.ndu, nDd = (size_t)d.ny * d.ndu;
    const size_t nseed = (size_t)d.nu + n1 * d.nu;
    const size_t per = nseed + nA + nB + nC + nBd + nDd + 2;           // seeds, the five outputs, and room for flag and count
    if (B * per > h->model_stage_cap) {
        if (h->model_stage) (void)hipFree(h->model_stage);
        h->model_stage = nullptr; h->model_stage_cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&h->model_stage), B * per * sizeof(double)) != hipSuccess) return fail(MPCX_E_DEVICE, "staging allocation failed");
        h->model_stage_cap = B * per;
    }
    int rc = mpcx_lmpc_model_sens_reserve(h, reduce ? h->sens_batch : 0);
    if (rc != MPCX_OK) return rc;
    double *sc = h->model_stage, *si = sc + B * d.nu, *gA = si + B * n1 * d.nu, *gB = gA + B * nA, *gC = gB + B * nB, *gBd = gC + B * nC, *gDd = gBd + B * nBd;
    int32_t *fl = reinterpret_cast<int32_t *>(gDd + B * nDd), *nu_ = fl + B;
    if ((seed_cmd && hipMemcpy(sc, seed_cmd, B * d.nu * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) ||
        (seed_input && hipMemcpy(si, seed_input, B * n1 * d.nu * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
        return fail(MPCX_E_DEVICE, "copy of the seeds to the device failed");
    // the batch mpcx_lmpc_solve_host solved, where it left it: the staging buffers' layout of that function
    double *dx0 = h->stage_d, *du0 = dx0 + B * d.nx, *dcmd = du0 + B * d.nu, *dcost = dcmd + B * d.nu;
    double *dss = dcost + B, *dso = dss + B * n1 * d.nx, *dsi = dso + B * n1 * d.ny;
    mpcx_lmpc_batch b{};
    b.batch = h->sens_batch; b.x0 = dx0; b.u0 = du0; b.cmd = dcmd; b.status = h->stage_i;
    b.active_lower = h->stage_act; b.active_upper = h->stage_act + B * aw; b.seq_state = dss; b.seq_output = dso; b.seq_input = dsi;
    mpcx_lmpc_model_sens s{};
    s.solved = &b; s.seed_cmd = seed_cmd ? sc : nullptr; s.seed_input = seed_input ? si : nullptr; s.reduce = reduce;
    s.d_A = gA; s.d_B = gB; s.d_C = gC; s.d_Bd = gBd; s.d_Dd = gDd; s.flags = fl; s.n_used = nu_;
    rc = mpcx_lmpc_model_sensitivity_batch(h, &s, nullptr);
    if (rc == MPCX_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(MPCX_E_DEVICE, "kernel execution failed");
    if (rc != MPCX_OK) return rc;
    const size_t lead = reduce ? 1 : B;
    bool ok = true;
    auto back = [&](void *dst, const void *src, size_t bytes) { if (dst && bytes) ok = ok && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    back(d_A, gA, lead * nA * sizeof(double)); back(d_B, gB, lead * nB * sizeof(double)); back(d_C, gC, lead * nC * sizeof(double));
    back(d_Bd, gBd, lead * nBd * sizeof(double)); back(d_Dd, gDd, lead * nDd * sizeof(double));
    back(flags, fl, B * sizeof(int32_t));
    if (reduce) back(n_used, nu_, sizeof(int32_t));
    return ok ? MPCX_OK : fail(MPCX_E_DEVICE, "copy of the results to the host failed");
}

int mpcx_lmpc_time_solve_batch(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream, int repeats, float *ms_mean)
{
    CHECK_H(h);
    if (!b || !ms_mean || repeats < 1) return fail(MPCX_E_INVALID, "bad argument");
    if (h->host_only) return fail(MPCX_E_DEVICE, "host-only handle");
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    if (hipSetDevice(h->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(MPCX_E_DEVICE, "hipEventCreate failed");
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < repeats; i++) {
        rc = mpcx_lmpc_solve_batch(h, b, stream);
        if (rc != MPCX_OK) break;
    }
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_mean = ms / (float)repeats;
    return rc;
}

int mpcx_lmpc_get_info(mpcx_lmpc_t h, mpcx_lmpc_info *info)
{
    CHECK_H(h);
    if (!info) return fail(MPCX_E_INVALID, "null info");
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    const auto &o = h->cond;
    const auto &d = h->ctl.d;
    info->n_ref = o.n_ref; info->m_ref = o.m_ref; info->neq_ref = o.neq_ref;
    info->nz = o.nz; info->mg = o.mg; info->active_words = o.active_words;
    info->kernel_variant = mpcx::lmpc_kernel_variant(o.ldz, o.ldg);
    info->flops_setup = o.flops_setup;
    const double nz = o.nz, mg = o.mg;
    info->flops_per_admm_iter = 2 * nz * nz + 4 * mg * nz + 12 * nz + 10 * mg;
    info->flops_fixed_per_solve = 2.0 * d.ph * d.nx * d.nx + 2.0 * (d.ph + 1) * d.ny * d.nx +
                                  2.0 * d.ph * (d.nx * d.nx + d.ny * d.nx + d.nx * d.nu) +
                                  2.0 * nz * (nz + mg) + 2.0 * nz * nz;
    info->bytes_per_solve = 8.0 * (d.nx + d.nu) + 8.0 * d.nu + 8.0 + 16.0;
    return MPCX_OK;
}

/* ---- heterogeneous batches -------------------------------------------------------------------------------------------------- */
int mpcx_lmpc_hetero_create(const mpcx_lmpc_t *controllers, int count, int device, mpcx_lmpc_hetero_t *out)
{
    return mpcx_lmpc_hetero_create_ex(controllers, count, device, 0, out);
}

int mpcx_lmpc_hetero_create_ex(const mpcx_lmpc_t *controllers, int count, int device, int condense_on_host, mpcx_lmpc_hetero_t *out)
{
    if (!controllers || !out || count < 1) return fail(MPCX_E_INVALID, "need at least one controller");
    const auto t_begin = std::chrono::steady_clock::now();
    for (int k = 0; k < count; ++k) if (!controllers[k]) return fail(MPCX_E_INVALID, "null controller in the bank");
    int ndev = 0;
    if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev)
        return fail(MPCX_E_DEVICE, "no such HIP device (the solve path has no CPU fallback)");
    // Controller 0 is condensed in full on the host: it fixes the structure (dimensions, constraint rows) and says whether the
    // dimensions fit the device kernel.  The others: in full too (condense_on_host, or dimensions beyond the kernel's LDS plan), or
    // their structure and O(n) arrays only -- the O(n^3) arrays of all K are then computed by lmpc_condense_models.
    std::vector<mpcx::Condensed> cond((size_t)count);
    std::vector<std::string> errs((size_t)count);
    errs[0] = controllers[0]->ctl.condense(cond[0]);
    if (!errs[0].empty()) return fail(MPCX_E_NUMERIC, "controller 0: " + errs[0]);
    bool on_device = !condense_on_host;
    {
        mpcx::LmpcDev probe{};
        probe.nz = cond[0].nz; probe.mg = cond[0].mg; probe.nx = controllers[0]->ctl.d.nx; probe.ny = controllers[0]->ctl.d.ny;
        if (mpcx::lmpc_condense_lds(probe, nullptr, nullptr) > mpcx::lmpc_lds_limit() - 64) on_device = false;
    }
    const mpcx::Condensed *like = on_device ? &cond[0] : nullptr;
    {
        unsigned nt = std::thread::hardware_concurrency();
        if (nt < 1) nt = 1;
        if (nt > 32) nt = 32;
        if ((int)nt > count) nt = (unsigned)count;
        std::atomic<int> next{0};
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; ++t)
            pool.emplace_back([&]() {
                for (int k = next.fetch_add(1) + 1; k < count; k = next.fetch_add(1) + 1) errs[(size_t)k] = controllers[k]->ctl.condense(cond[(size_t)k], like);
            });
        for (auto &th : pool) th.join();
    }
    for (int k = 0; k < count; ++k)
        if (!errs[(size_t)k].empty()) return fail(MPCX_E_NUMERIC, "controller " + std::to_string(k) + ": " + errs[(size_t)k]);
    // one structure for all: dimensions, constraint rows (which bounds are finite), move blocking
    const auto &c0 = controllers[0]->ctl;
    const auto &o0 = cond[0];
    if (mpcx::lmpc_kernel_variant(o0.ldz, o0.ldg) < 0) return fail(MPCX_E_UNSUPPORTED, "condensed problem larger than 512 variables / rows");
    for (int k = 1; k < count; ++k) {
        const auto &ck = controllers[k]->ctl;
        const auto &ok = cond[(size_t)k];
        const bool same = ck.d.nx == c0.d.nx && ck.d.nu == c0.d.nu && ck.d.ny == c0.d.ny && ck.d.ndu == c0.d.ndu && ck.d.ph == c0.d.ph && ck.d.ch == c0.d.ch &&
                          ok.nz == o0.nz && ok.mg == o0.mg && ok.g_refrow == o0.g_refrow && ok.boxrow_ptr == o0.boxrow_ptr && ok.boxrow_ref == o0.boxrow_ref &&
                          ok.fixed_rows.size() == o0.fixed_rows.size() && ok.blk == o0.blk;
        if (!same) return fail(MPCX_E_INVALID, "controller " + std::to_string(k) + " differs from controller 0 in dimensions or in which bounds are finite");
        // ... and one pattern of soft rows; the weights may differ
        for (size_t r = 0; r < o0.g_soft.size(); ++r)
            if ((ok.g_soft[r] > 0.0) != (o0.g_soft[r] > 0.0))
                return fail(MPCX_E_INVALID, "controller " + std::to_string(k) + " differs from controller 0 in which constraint rows are soft");
        // ... and a terminal cost in every controller or in none (the wavefronts' LDS plan is controller 0's); P, xT and Tx may differ
        if (ck.have_terminal != c0.have_terminal)
            return fail(MPCX_E_INVALID, "controller " + std::to_string(k) + " differs from controller 0 in whether it has a terminal cost");
        // ... and as many linear rows (the LDS plan again, and the row numbering); Fx, Fu and the bounds may differ
        if (ck.linear_rows_live() != c0.linear_rows_live())
            return fail(MPCX_E_INVALID, "controller " + std::to_string(k) + " differs from controller 0 in the number of its linear rows");
    }
    std::unique_ptr<mpcx_lmpc_hetero> f(new mpcx_lmpc_hetero);
    f->device = device; f->count = count; f->d = c0.d; f->active_words = o0.active_words; f->m_ref = o0.m_ref;
    if (hipSetDevice(device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    SlabUploader U;
    U.big_on_device = on_device;
    std::vector<mpcx::LmpcDev> devs((size_t)count);
    int rc = MPCX_OK;
    for (int k = 0; k < count; ++k) {
        auto &o = cond[(size_t)k];
        // the stacked maps of the MFMA assemble kernel serve sixteen instances of ONE model: not used here, not uploaded
        o.MA[0].clear(); o.MA[1].clear(); o.MF[0].clear(); o.MF[1].clear(); o.Ym.clear();
        fill_dev_scalars(controllers[k], controllers[k]->ctl, o, devs[(size_t)k]);
        fill_dev_arrays(controllers[k], controllers[k]->ctl, o, devs[(size_t)k], U, rc);
        devs[(size_t)k].fused_ok = 0; devs[(size_t)k].group_ok = 0;
    }
    if (hipMalloc(reinterpret_cast<void **>(&f->slab), U.host.size()) != hipSuccess ||
        hipMemcpy(f->slab, U.host.data(), U.host.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MPCX_E_DEVICE, "could not upload the bank (" + std::to_string(U.host.size() >> 20) + " MiB)");
    if (U.dev_bytes) {
        if (hipMalloc(reinterpret_cast<void **>(&f->slab_dev), U.dev_bytes) != hipSuccess || hipMemset(f->slab_dev, 0, U.dev_bytes) != hipSuccess)
            return fail(MPCX_E_DEVICE, "could not allocate the bank's factors (" + std::to_string(U.dev_bytes >> 20) + " MiB)");
    }
    for (auto &D : devs) rebase_dev(D, f->slab, f->slab_dev);
    if (hipMalloc(reinterpret_cast<void **>(&f->models_d), sizeof(mpcx::LmpcDev) * (size_t)count) != hipSuccess ||
        hipMemcpy(f->models_d, devs.data(), sizeof(mpcx::LmpcDev) * (size_t)count, hipMemcpyHostToDevice) != hipSuccess)
        return fail(MPCX_E_DEVICE, "could not upload the bank's model table");
    f->dev0 = devs[0];
    f->setup_flops = cond[0].flops_setup;
    if (on_device) {
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, nullptr);
        const int lr = mpcx::lmpc_condense_launch(f->models_d, f->dev0, count, nullptr);
        (void)hipEventRecord(e1, nullptr);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&f->setup_kernel_ms, e0, e1);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (lr != 0) return fail(MPCX_E_DEVICE, "the device condensing kernel could not be launched (" + std::to_string(lr) + ")");
        const hipError_t es = hipDeviceSynchronize();
        if (es != hipSuccess) return fail(MPCX_E_DEVICE, std::string("the device condensing kernel failed: ") + hipGetErrorString(es));
        // what LmpcController::condense reports on the host (MPCX_E_NUMERIC for a Hessian / ADMM matrix that does not factor), and what the
        // host path reports as "differs from controller 0" (a constraint row that vanishes in one controller but not in the first)
        if (hipMemcpy(devs.data(), f->models_d, sizeof(mpcx::LmpcDev) * (size_t)count, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(MPCX_E_DEVICE, "could not read the bank's model table back");
        for (int k = 0; k < count; ++k) {
            const int cs = devs[(size_t)k].cond_status;
            if (cs & 1) return fail(MPCX_E_NUMERIC, "controller " + std::to_string(k) + ": condensed Hessian is not positive semidefinite");
            if (cs & 2) return fail(MPCX_E_NUMERIC, "controller " + std::to_string(k) + ": ADMM matrix is not positive definite");
            if (cs & 4) return fail(MPCX_E_INVALID, "controller " + std::to_string(k) + " differs from controller 0: one of its constraint rows does not depend on the inputs");
        }
    }
    f->condensed_on_device = on_device;
    f->setup_total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    *out = f.release();
    return MPCX_OK;
}

int mpcx_lmpc_hetero_destroy(mpcx_lmpc_hetero_t f)
{
    if (!f) return MPCX_OK;
    (void)hipSetDevice(f->device);
    delete f;
    return MPCX_OK;
}

/* testing aid: one O(n^3) array ("H", "Kinv", "Gr", "Gc", "Y", "rho_b", "rho_g") of model k copied to the host; returns its length */
// testing aid: {instances the fallback kernel served in the last step that had any since the previous read, entries the failure queue holds, wavefronts of the fallback
// kernel's grid at a full batch}; waits for the device
static bool fallback_state(const mpcx::LmpcScratch &sc, double *out3)
{
    int *const fq = sc.fq;
    int served = 0;
    // (the idle fallback launch writes nothing, not even a zero here: the read clears the figure, so that it speaks of the steps since the last read)
    if (fq && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&served, fq + mpcx::kFqServed, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemset(fq + mpcx::kFqServed, 0, sizeof(int)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) return false;
    const int w = mpcx::lmpc_fallback_waves();
    out3[0] = served; out3[1] = (double)sc.cap; out3[2] = fq ? (sc.pslots < w ? sc.pslots : w) : w;
    return true;
}

int mpcx_lmpc_hetero_debug_get(mpcx_lmpc_hetero_t f, int k, const char *name, double *out, int cap)
{
    if (!f || k < 0 || k >= f->count || !name) return fail(MPCX_E_INVALID, "bad argument");
    if (hipSetDevice(f->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (std::string(name) == "fallback") {
        if (out && cap >= 3 && !fallback_state(f->scratch, out)) return fail(MPCX_E_DEVICE, "hipMemcpy failed");
        return 3;
    }
    mpcx::LmpcDev D;
    if (hipMemcpy(&D, f->models_d + k, sizeof(D), hipMemcpyDeviceToHost) != hipSuccess) return fail(MPCX_E_DEVICE, "hipMemcpy failed");
    const std::string n(name);
    const double *src = nullptr; size_t len = 0;
    if (n == "H") { src = D.H; len = (size_t)D.ldz * D.ldz; } else if (n == "Kinv") { src = D.Kinv; len = (size_t)D.ldz * D.ldz; }
    else if (n == "Gr") { src = D.Gr; len = (size_t)D.ldg * D.ldz; } else if (n == "Gc") { src = D.Gc; len = (size_t)D.ldz * D.ldg; }
    else if (n == "Y") { src = D.Y; len = (size_t)D.ldy * D.ldy; } else if (n == "rho_b") { src = D.rho_b; len = (size_t)D.ldz; }
    else if (n == "rho_g") { src = D.rho_g; len = (size_t)D.ldg; } else if (n == "g_soft") { src = MPCX_G_SOFT(D); len = (size_t)D.ldg; }
    else if (n == "flags") {       // cost_direct, condensed on the device, condensing kernel ms, whole create ms, set-up flops per controller
        if (out && cap >= 5) { out[0] = D.cost_direct; out[1] = f->condensed_on_device ? 1.0 : 0.0; out[2] = f->setup_kernel_ms; out[3] = f->setup_total_ms; out[4] = f->setup_flops; }
        return 5;
    }
    else return fail(MPCX_E_INVALID, "unknown array name");
    if (!out) return (int)len;
    if ((size_t)cap < len) return fail(MPCX_E_INVALID, "buffer too small");
    if (hipMemcpy(out, src, len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(MPCX_E_DEVICE, "hipMemcpy failed");
    return (int)len;
}

int mpcx_lmpc_hetero_get_info(mpcx_lmpc_hetero_t f, int *count, int *active_words, int *m_ref, double *bytes_per_model)
{
    if (!f) return fail(MPCX_E_INVALID, "null bank");
    if (count) *count = f->count;
    if (active_words) *active_words = f->active_words;
    if (m_ref) *m_ref = f->m_ref;
    if (bytes_per_model) {
        const auto &D = f->dev0;
        // what a solve reads of its own model: -Hinv and G Hinv once (assemble), the model and weight arrays, the bounds
        *bytes_per_model = 8.0 * ((double)D.nz * D.ldy + (double)D.nx * D.nx + (double)D.nx * D.nu + (double)D.ny * D.nx +
                                  (double)(D.ph + 1) * (D.ny + D.nu) + (double)D.ph * D.nu + 2.0 * D.ldz + 2.0 * D.ldg);
    }
    return MPCX_OK;
}

int mpcx_lmpc_hetero_solve_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_batch *b, const int32_t *model_index, void *stream)
{
    if (!f || !b) return fail(MPCX_E_INVALID, "null argument");
    if (hipSetDevice(f->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    if (b->batch == 0) return MPCX_OK;
    if (b->batch < 0 || !b->x0 || !b->u0 || !b->cmd) return fail(MPCX_E_INVALID, "x0, u0 and cmd are required");
    if (!model_index && b->batch != f->count) return fail(MPCX_E_INVALID, "without a model index the batch must be the bank: instance b uses controller b");
    // references: per instance or per step from the caller; "shared" = each controller's own (its setReferences), read through the model
    const double *const own[4] = {nullptr, nullptr, nullptr, nullptr};
    mpcx::LmpcBatchDev B;
    const int rc = make_batch(f->d, b, own, B);
    if (rc != MPCX_OK) return rc;
    B.n_models = f->count; B.model_index = model_index;
    if (mpcx::lmpc_scratch_reserve(f->scratch, f->dev0, b->batch, false, stream) != 0) return fail(MPCX_E_DEVICE, "workspace allocation failed");
    const int lr = mpcx::lmpc_launch(f->dev0, f->models_d, B, f->scratch, stream, 7, kHeteroPlan);
    return lr == 0 ? MPCX_OK : launch_failed(lr, f->scratch, stream);
}

int mpcx_lmpc_hetero_sensitivity_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_sens *s, const int32_t *model_index, void *stream)
{
    if (!f) return fail(MPCX_E_INVALID, "null bank");
    if (!s) return fail(MPCX_E_INVALID, "null sensitivity descriptor");
    if (s->mode != MPCX_SENS_JACOBIAN && s->mode != MPCX_SENS_VJP) return fail(MPCX_E_INVALID, "unknown sensitivity mode");
    if (s->batch < 1) return fail(MPCX_E_INVALID, "batch below 1");
    if (!s->active_lower || !s->active_upper) return fail(MPCX_E_INVALID, "active_lower and active_upper are required");
    if (s->mode == MPCX_SENS_VJP && !s->seed_cmd && !s->seed_input) return fail(MPCX_E_INVALID, "a vector-Jacobian product needs seed_cmd or seed_input");
    if (!model_index && s->batch != f->count) return fail(MPCX_E_INVALID, "without a model index the batch must be the bank: instance b uses controller b");
    if (hipSetDevice(f->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    mpcx::LmpcBankSensArgs a{};
    a.s.batch = s->batch; a.s.jacobian = s->mode == MPCX_SENS_JACOBIAN;
    a.s.active_lower = s->active_lower; a.s.active_upper = s->active_upper; a.s.status = s->status;
    a.s.seed_cmd = a.s.jacobian ? nullptr : s->seed_cmd; a.s.seed_input = a.s.jacobian ? nullptr : s->seed_input;
    a.s.d_x0 = s->d_x0; a.s.d_u0 = s->d_u0; a.s.d_yref = s->d_yref; a.s.flags = s->flags;
    a.models = f->models_d; a.model_index = model_index; a.n_models = f->count;
    const int lr = mpcx::lmpc_bank_sens_launch(f->dev0, a, stream);
    if (lr == -2) return fail(MPCX_E_UNSUPPORTED, "problem dimensions exceed the bank sensitivity kernel's LDS budget");
    return lr == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
}

int mpcx_lmpc_bank_grad_size(void) { return (int)sizeof(mpcx_lmpc_bank_grad); }

int mpcx_lmpc_hetero_gradient_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_bank_grad *g, const int32_t *model_index, void *stream)
{
    if (!f) return fail(MPCX_E_INVALID, "null bank");
    if (!g) return fail(MPCX_E_INVALID, "null gradient descriptor");
    const mpcx_lmpc_batch *b = g->solved;
    if (!b) return fail(MPCX_E_INVALID, "the solved batch is required");
    if (b->batch < 1) return fail(MPCX_E_INVALID, "batch below 1");
    if (!g->seed_cmd && !g->seed_input) return fail(MPCX_E_INVALID, "a gradient needs seed_cmd or seed_input");
    if (!b->active_lower || !b->active_upper) return fail(MPCX_E_INVALID, "active_lower and active_upper of the solved batch are required");
    if (!b->x0 || !b->u0) return fail(MPCX_E_INVALID, "x0 and u0 of the solved batch are required");
    if (!b->seq_output || !b->seq_input) return fail(MPCX_E_INVALID, "the solved batch carries no sequences: seq_output and seq_input are required");
    const bool with_model = f->d.ndu > 0 ? (g->d_A || g->d_B || g->d_C || g->d_Bd || g->d_Dd) : (g->d_A || g->d_B || g->d_C);
    if (with_model && !b->seq_state) return fail(MPCX_E_INVALID, "a model output needs seq_state of the solved batch");
    if (!model_index && b->batch != f->count) return fail(MPCX_E_INVALID, "without a model index the batch must be the bank: instance b uses controller b");
    const double *const dv[10] = {g->d_oweight, g->d_uweight, g->d_duweight, g->d_lower, g->d_upper, g->d_A, g->d_B, g->d_C, g->d_Bd, g->d_Dd};
    const double *const cv[10] = {g->c_oweight, g->c_uweight, g->c_duweight, g->c_lower, g->c_upper, g->c_A, g->c_B, g->c_C, g->c_Bd, g->c_Dd};
    bool sums = g->n_used != nullptr, any_d = false;
    for (int k = 0; k < 10; ++k) {
        if (cv[k] && !dv[k]) return fail(MPCX_E_INVALID, "a per-controller sum needs the per-instance output it adds up");
        sums = sums || cv[k]; any_d = any_d || dv[k];
    }
    if (sums && (!g->group_order || !g->group_offsets)) return fail(MPCX_E_INVALID, "per-controller sums need group_order and group_offsets");
    if (g->n_used && !g->flags && !any_d) return fail(MPCX_E_INVALID, "n_used needs flags or a per-instance output");
    if (hipSetDevice(f->device) != hipSuccess) return fail(MPCX_E_DEVICE, "hipSetDevice failed");
    // references: per instance or per step from the caller; "shared" = each controller's own, read through the model
    const double *const own[4] = {nullptr, nullptr, nullptr, nullptr};
    mpcx::LmpcBatchDev B;
    const int rc = make_batch(f->d, b, own, B);
    if (rc != MPCX_OK) return rc;
    mpcx::LmpcBankGradArgs a{};
    a.batch = b->batch;
    a.active_lower = b->active_lower; a.active_upper = b->active_upper; a.status = b->status;
    a.seed_cmd = g->seed_cmd; a.seed_input = g->seed_input;
    a.u0 = b->u0; a.seq_state = b->seq_state; a.seq_output = b->seq_output; a.seq_input = b->seq_input;
    a.yref = B.yref; a.yref_bs = B.yref_bs; a.yref_ks = B.yref_ks;
    a.uref = B.uref; a.uref_bs = B.uref_bs; a.uref_ks = B.uref_ks;
    a.duref = B.duref; a.duref_bs = B.duref_bs; a.duref_ks = B.duref_ks;
    a.dmeas = B.dmeas; a.dmeas_bs = B.dmeas_bs; a.dmeas_ks = B.dmeas_ks;
    a.d_oweight = g->d_oweight; a.d_uweight = g->d_uweight; a.d_duweight = g->d_duweight; a.d_lower = g->d_lower; a.d_upper = g->d_upper;
    a.d_A = g->d_A; a.d_B = g->d_B; a.d_C = g->d_C; a.d_Bd = g->d_Bd; a.d_Dd = g->d_Dd;
    a.flags = g->flags;
    a.models = f->models_d; a.model_index = model_index; a.n_models = f->count;
    a.group_order = g->group_order; a.group_offsets = g->group_offsets;
    a.c_oweight = g->c_oweight; a.c_uweight = g->c_uweight; a.c_duweight = g->c_duweight; a.c_lower = g->c_lower; a.c_upper = g->c_upper;
    a.c_A = g->c_A; a.c_B = g->c_B; a.c_C = g->c_C; a.c_Bd = g->c_Bd; a.c_Dd = g->c_Dd;
    a.n_used = g->n_used;
    const int lr = mpcx::lmpc_bank_grad_launch(f->dev0, a, stream);
    if (lr == -2) return fail(MPCX_E_UNSUPPORTED, "problem dimensions exceed the bank gradient kernel's LDS budget");
    return lr == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
}

int mpcx_lmpc_hetero_time_solve_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_batch *b, const int32_t *model_index, void *stream, int repeats, float *ms_mean)
{
    if (!f || !b || !ms_mean || repeats < 1) return fail(MPCX_E_INVALID, "bad argument");
    int rc = mpcx_lmpc_hetero_solve_batch(f, b, model_index, stream);
    if (rc != MPCX_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(MPCX_E_DEVICE, "hipEventCreate failed");
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < repeats && rc == MPCX_OK; i++) rc = mpcx_lmpc_hetero_solve_batch(f, b, model_index, stream);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_mean = ms / (float)repeats;
    return rc;
}

/* profiling aid: mean time (ms) of the assemble and of the solve kernel, each timed alone with
 * HIP events on `stream` (the solve kernel re-reads the workspace the assemble kernel left). */
int mpcx_lmpc_debug_time_kernels(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream, int repeats, float *ms2)
{
    CHECK_H(h);
    if (!b || !ms2 || repeats < 1 || h->host_only) return fail(MPCX_E_INVALID, "bad argument");
    int rc = mpcx_lmpc_solve_batch(h, b, stream);      // sizes the workspace, fills it
    if (rc != MPCX_OK) return rc;
    mpcx::LmpcBatchDev B;
    rc = make_handle_batch(h, b, B);
    if (rc != MPCX_OK) return rc;
    const mpcx::LmpcPlan plan = lmpc_plan(h, b);
    auto launch = [&](int which) { return mpcx::lmpc_launch(h->dev, h->dev_d, B, h->scratch, stream, which, plan); };
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int which = 1; which <= 4; which *= 2) {
        float ms = 0;
        if (which == 2 && h->dev.cost_direct) {
            // with pending costs the solve leaves w in t0's place: every timed launch needs a freshly assembled workspace
            for (int i = 0; i < repeats; i++) {
                launch(1);
                (void)hipEventRecord(e0, s);
                launch(2);
                (void)hipEventRecord(e1, s);
                (void)hipEventSynchronize(e1);
                float one = 0;
                (void)hipEventElapsedTime(&one, e0, e1);
                ms += one;
            }
        } else {
            (void)hipEventRecord(e0, s);
            for (int i = 0; i < repeats; i++) launch(which);
            (void)hipEventRecord(e1, s);
            (void)hipEventSynchronize(e1);
            (void)hipEventElapsedTime(&ms, e0, e1);
        }
        // the solve kernels ran without the fallback behind them: what they filed in the failure queue is dropped (outside the timed window), so that
        // slot 2 times the idle fallback launch and the next step starts from an empty queue
        if (which == 2) (void)mpcx::lmpc_fallback_reset(h->scratch.fq, stream);
        ms2[which == 1 ? 0 : (which == 2 ? 1 : 2)] = ms / (float)repeats;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return MPCX_OK;
}

/* testing aid: how many full set-ups (condensing + device rebuild) and how many reference-only refreshes have run */
int mpcx_lmpc_debug_setup_counts(mpcx_lmpc_t h, int *full, int *refs)
{
    CHECK_H(h);
    if (full) *full = h->n_full_setups;
    if (refs) *refs = h->n_ref_refreshes;
    return MPCX_OK;
}

/* experiment / testing knob: 1 = wherever the dimensions allow, compute each instance's record inside the solve kernel instead of
 * handing it over through the HBM workspace; 0 = never; -1 = automatic (the default: from 16384 instances on) */
int mpcx_lmpc_debug_use_fused(mpcx_lmpc_t h, int on)
{
    CHECK_H(h);
    h->use_fused = on < 0 ? -1 : (on > 2 ? 2 : on);      // 2: lmpc_solve_group (assemble + solve in one workgroup of sixteen wavefronts)
    h->dirty = true;
    return MPCX_OK;
}

/* Sharding: this handle is given contiguous shards of a batch of `total` instances (one rank of N).  The kernel form is chosen for the
 * whole batch's size, so that a shard's results are, bit for bit, the rows of the unsharded solve also where the two sizes lie on either
 * side of the threshold between the in-workgroup form and the two-kernel form (0: every call is a whole batch, the default). */
int mpcx_lmpc_set_total_batch(mpcx_lmpc_t h, int total)
{
    CHECK_H(h);
    if (total < 0) return fail(MPCX_E_INVALID, "negative batch");
    h->total_batch = total;
    return MPCX_OK;
}

/* testing aid: 1 = always use the generic (roll-out) assemble kernel */
int mpcx_lmpc_debug_force_generic(mpcx_lmpc_t h, int on)
{
    CHECK_H(h);
    h->force_generic = on != 0;
    return MPCX_OK;
}

/* experiment knob: rounds the polish-only kernel may spend before handing an instance to the ADMM kernel, and the number of
 * ADMM iterations between two polish attempts there */
int mpcx_lmpc_debug_set_rounds(mpcx_lmpc_t h, int rounds0, int check_every)
{
    CHECK_H(h);
    h->dbg_rounds0 = rounds0; h->dbg_check_every = check_every;
    h->dirty = true;
    return MPCX_OK;
}

/* profiling aid: device buffer [B x 8] of int64 receiving per-phase cycle stamps */
int mpcx_lmpc_debug_set_cycle_buffer(mpcx_lmpc_t h, void *dev_ptr)
{
    CHECK_H(h);
    h->dbg_cycles = static_cast<long long *>(dev_ptr);
    return MPCX_OK;
}

/* testing aid: the wave-wide sums of the lean LMPC kernels on nvec vectors of 64 doubles, every lane of the old and of the new form
 * (include/mpcx.h) */
int mpcx_lmpc_debug_wave_reduce(const double *in, double *out, int nvec, void *stream)
{
    if (!in || !out || nvec < 0) return fail(MPCX_E_INVALID, "mpcx_lmpc_debug_wave_reduce: null buffer or negative count");
    return mpcx::lmpc_debug_wave_reduce(in, out, nvec, stream) == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, "mpcx_lmpc_debug_wave_reduce: launch failed");
}
int mpcx_lmpc_debug_ws_solve(const double *Y, int n, int ldy, int nz, const int *wsidx, const double *wsb, const int *na, const double *t0, double *out,
                             int count, void *stream)
{
    if (!Y || !wsidx || !wsb || !na || !t0 || !out || count < 0) return fail(MPCX_E_INVALID, "mpcx_lmpc_debug_ws_solve: null buffer or negative count");
    const int rc = mpcx::lmpc_debug_ws_solve(Y, n, ldy, nz, wsidx, wsb, na, t0, out, count, stream);
    if (rc == -2) return fail(MPCX_E_INVALID, "mpcx_lmpc_debug_ws_solve: nz and n - nz must be even and in 2 .. 128, ldy even and >= n");
    return rc == 0 ? MPCX_OK : fail(MPCX_E_DEVICE, "mpcx_lmpc_debug_ws_solve: launch failed");
}

/* ---- testing aid (not part of the reference-facing surface): copy a condensed array to
 * the host so that CPU-only tests can check the set-up without a GPU. ------------------ */
int mpcx_lmpc_debug_get(mpcx_lmpc_t h, const char *name, double *out, int cap)
{
    CHECK_H(h);
    int rc = mpcx_lmpc_setup(h);
    if (rc != MPCX_OK) return rc;
    const auto &o = h->cond;
    const std::vector<double> *v = nullptr;
    std::vector<double> tmp;
    std::string n(name ? name : "");
    if (n == "H") v = &o.H; else if (n == "Kinv") v = &o.Kinv; else if (n == "Gr") v = &o.Gr;
    else if (n == "Gc") v = &o.Gc; else if (n == "Y") v = &o.Y; else if (n == "lw") v = &o.lw;
    else if (n == "uw") v = &o.uw; else if (n == "rho_b") v = &o.rho_b; else if (n == "lg0") v = &o.lg0;
    else if (n == "ug0") v = &o.ug0; else if (n == "rho_g") v = &o.rho_g; else if (n == "g_soft") v = &o.g_soft;
    else if (n == "dims") {
        tmp = {(double)o.nz, (double)o.mg, (double)o.ldz, (double)o.ldg, (double)o.ldy, (double)o.nf,
               (double)o.n_ref, (double)o.m_ref, (double)o.neq_ref, (double)o.fixed_rows.size(),
               (double)h->dev.lds_per_wave, (double)(o.h_regularised ? 1 : 0)};
        v = &tmp;
    } else if (n == "MA0") v = &o.MA[0]; else if (n == "MA1") v = &o.MA[1]; else if (n == "Ym") v = &o.Ym;
    else if (n == "MA0p" || n == "MA1p" || n == "Ymp") {      // the packed copies lmpc_solve_group / lmpc_assemble_mfma read (computed here as at upload)
        const std::vector<double> &src = n == "Ymp" ? o.Ym : o.MA[n == "MA1p" ? 1 : 0];
        const int rows = n == "Ymp" ? o.ldy16 : o.rowsA, K = n == "Ymp" ? o.nz16 : o.kin;
        if (!src.empty()) { tmp.resize(mpcx::lmpc_packed_len(rows, K)); mpcx::lmpc_pack_mfma_tiles(src.data(), rows, K, tmp.data()); }
        v = &tmp;
    } else if (n == "flags") {           // which forms of the solve this controller can take: cost from its definition (lmpc_cost_mfma follows lmpc_solve), one-workgroup form, fused mat-vec form
        tmp = {(double)h->dev.cost_direct, (double)h->dev.group_ok, (double)h->dev.fused_ok};
        v = &tmp;
    } else if (n == "dims_maps") {
        tmp = {(double)o.kin, (double)o.nxp, (double)o.nup, (double)o.nyp, (double)o.ione, (double)o.nz16, (double)o.mg16,
               (double)o.ns, (double)o.ns16, (double)o.kq16, (double)o.rowsA, (double)o.ldy16};
        v = &tmp;
    } else if (n == "g_refrow") { tmp.assign(o.g_refrow.begin(), o.g_refrow.end()); v = &tmp; }
    else if (n == "MF1") v = &o.MF[1];
    else if (n == "dims_fused") { tmp = {(double)o.rowsF, (double)o.nsp, (double)o.kin, (double)o.nxp, (double)o.nup, (double)o.nyp, (double)o.ione}; v = &tmp; }
    else if (n == "boxrow_ptr") { tmp.assign(o.boxrow_ptr.begin(), o.boxrow_ptr.end()); v = &tmp; }
    else if (n == "boxrow_ref") { tmp.assign(o.boxrow_ref.begin(), o.boxrow_ref.end()); v = &tmp; }
    else if (n == "blk") { tmp.assign(o.blk.begin(), o.blk.end()); v = &tmp; }
    else if (n == "Cq") { if (param_operand(h, false) != MPCX_OK) return MPCX_E_DEVICE; v = &h->param_cq; }
    else if (n == "Xq") { if (model_operand(h, false) != MPCX_OK) return MPCX_E_DEVICE; v = &h->model_xq; }
    else if (n == "model") {              // A | B | C | Bd | Dd as stored, column-major
        for (const mpcx::Mat *m : {&h->ctl.A, &h->ctl.B, &h->ctl.C, &h->ctl.Bd, &h->ctl.Dd}) tmp.insert(tmp.end(), m->a.begin(), m->a.end());
        v = &tmp;
    }
    else if (n == "wDeltaU") v = &h->ctl.wDeltaU.a;
    else if (n == "scalar") { tmp = h->ctl.scalar_linear_block(); v = &tmp; }      // sX | row c: Fx(c, :), Fu(c, :) of the live linear rows
    else if (n == "sU") v = &h->ctl.sU;
    else if (n == "g_step") { tmp.assign(o.g_step.begin(), o.g_step.end()); v = &tmp; }
    else if (n == "g_kind") { tmp.assign(o.g_kind.begin(), o.g_kind.end()); v = &tmp; }
    else if (n == "g_comp") { tmp.assign(o.g_comp.begin(), o.g_comp.end()); v = &tmp; }
    else if (n == "slo") v = &o.slo; else if (n == "shi") v = &o.shi;
    else if (n == "wOutput") v = &h->ctl.wOutput.a; else if (n == "wU") v = &h->ctl.wU.a;      // the weights as stored, [ny | nu x (ph + 1)] internal columns
    else if (n == "linear") {             // the linear rows as stored: [nc | Fx | Fu | lo | hi | weights], the matrices column-major; [0] without any
        const auto &c = h->ctl;
        tmp = {(double)c.nlin};
        for (const mpcx::Mat *m : {&c.linFx, &c.linFu, &c.linLo, &c.linHi, &c.linSoft}) tmp.insert(tmp.end(), m->a.begin(), m->a.end());
        v = &tmp;
    }
    else if (n == "fixed_rows") {         // [kind, step, comp, refrow, lo, hi] of every row that sees no decision variable
        for (const auto &r : o.fixed_rows) tmp.insert(tmp.end(), {(double)r.kind, (double)r.step, (double)r.comp, (double)r.refrow, r.lo, r.hi});
        v = &tmp;
    }
    else if (n == "terminal") { tmp = h->ctl.terminal_block(); v = &tmp; }      // [P | xT | Tx] as stored (P symmetrised); empty without the term
    else if (n == "ws_limit") {           // most rows a working set may hold, the lists' capacity, doubles of a wavefront's large-working-set slot
        tmp = {(double)mpcx::ws_limit(o.nz, o.mg, o.n_soft), (double)mpcx::ws_capacity(mpcx::ws_limit(o.nz, o.mg, o.n_soft)), (double)mpcx::lmpc_slot_len(h->dev)};
        v = &tmp;
    }
    else if (n == "fallback") {           // the failure queue: served in the last step that had failures, capacity, fallback wavefronts
        tmp.assign(3, 0.0);
        if (out && !h->host_only) {
            if (hipSetDevice(h->device) != hipSuccess || !fallback_state(h->scratch, tmp.data())) return fail(MPCX_E_DEVICE, "hipMemcpy failed");
        }
        v = &tmp;
    }
    else return fail(MPCX_E_INVALID, "unknown array name");
    if (!out) return (int)v->size();
    if (cap < (int)v->size()) return fail(MPCX_E_INVALID, "buffer too small");
    std::memcpy(out, v->data(), sizeof(double) * v->size());
    return (int)v->size();
}

}  // extern "C"
