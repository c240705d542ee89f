// TEST INFRASTRUCTURE -- runs the bank's gradient kernels (libmpc_amd/csrc/lmpc_bank_grad.hip, compiled unchanged: lmpc_bank_grad_launch,
// lmpc_bank_gradient, lmpc_bank_grad_reduce) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of
// libmpcx.so.  Compiled with clang++ (the kernel's helpers name the components of an ext_vector_type).
//
//   run_bank_grad <lds_limit bytes> < numbers
//   stdin, whitespace separated: nx nu ndu ny ph nz mg ldz ldg ldy active_words n_soft m_ref flag_word (LmpcDev::adaptive_rho) K batch, then 22
//   switches: want d_oweight d_uweight d_duweight d_lower d_upper d_A d_B d_C d_Bd d_Dd, flags, the ten c_* in that order, n_used; then arrays,
//   each as its length followed by its values.  The structure the controllers share: g_kind, g_step, g_comp, g_refrow [ldg], boxrow_ptr [nz + 1],
//   boxrow_ref, blk [ph + 1]; for each of the K controllers Y [ldy ldy], model (A | B | C | Bd | Dd), Wy (the terminal block behind it), Wu, Wdu,
//   sX (the linear rows behind it), sU, rho_g [2 ldg] (the soft rows' 1 / weight in its second half), lg0, ug0 [ldg], and its own references
//   yref [ph ny], uref, duref [ph nu], dmeas [ph ndu] (column-major, as mpcx_lmpc_debug_get returns them); then model_index [batch], active_lower,
//   active_upper [batch active_words], status [batch], seed_cmd [batch nu], seed_input [batch (ph + 1) nu], u0 [batch nu], seq_state
//   [batch (ph + 1) nx], seq_output, seq_input, yref [batch ny] (per instance), group_order [batch], group_offsets [K + 1] -- model_index,
//   status, the seeds, seq_state, yref and the group arrays may have length 0: a null pointer (yref: each controller's own)
//   stdout: one JSON object: rc (what lmpc_bank_grad_launch returned), the ten d_*, flags, the ten c_*, n_used
// Every output array is followed by a guard of kPad elements that must come back untouched (the test checks them), an output that was not asked for
// is passed as a null pointer.  The kernel's LDS is one array of the size of the limit and a guard behind it that must come back untouched (exit 4).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#undef __shared__
#define __shared__ thread_local

constexpr int kPad = 64, kLdsDoubles = 160 * 1024 / 8;
constexpr double kGuard = -7.25e300;
constexpr int kGuardI = -77;
static size_t g_limit = (size_t)kLdsDoubles * 8;

inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }

// the kernel's `extern __shared__ double smem[]`: a block-scope declaration, so a member of the namespace around the kernel
namespace mpcx { namespace { alignas(64) thread_local double smem[kLdsDoubles + kPad]; } }

#include "../../libmpc_amd/csrc/lmpc_bank_grad.hip"

size_t mpcx::lmpc_lds_limit() { return g_limit; }
int mpcx::lmpc_raise_dynamic_lds(LmpcLdsCache &, std::initializer_list<const void *>, size_t bytes) { return bytes <= g_limit ? 0 : -3; }

static double next_d()
{
    double v;
    if (scanf("%lf", &v) != 1) { fprintf(stderr, "input ended early\n"); exit(3); }
    return v;
}
static int next_i() { return (int)next_d(); }
// an array: its length, then its values; `want` < 0: any length
static std::vector<double> read_d(long want)
{
    const long n = (long)next_d();
    if (n < 0 || (want >= 0 && n != want)) { fprintf(stderr, "an array of %ld values where %ld were expected\n", n, want); exit(2); }
    std::vector<double> v((size_t)n);
    for (double &x : v) x = next_d();
    return v;
}
static std::vector<int> read_i(long want) { const std::vector<double> d = read_d(want); return std::vector<int>(d.begin(), d.end()); }
static std::vector<double> read_opt(long want)
{
    const long n = (long)next_d();
    if (n != 0 && n != want) { fprintf(stderr, "an optional array of %ld values where %ld were expected\n", n, want); exit(2); }
    std::vector<double> v((size_t)n);
    for (double &x : v) x = next_d();
    return v;
}
static void put(const char *name, const std::vector<double> &v)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) {
        if (std::isnan(v[i])) printf("%sNaN", i ? ", " : "");
        else if (std::isinf(v[i])) printf("%s%sInfinity", i ? ", " : "", v[i] < 0 ? "-" : "");
        else printf("%s%.17g", i ? ", " : "", v[i]);
    }
    printf("], ");
}
static void put_i(const char *name, const std::vector<int32_t> &v, const char *end)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", (int)v[i]);
    printf("]%s", end);
}

struct Controller { std::vector<double> Y, model, wy, wu, wdu, sx, su, rho_g, lg0, ug0, yref, uref, duref, dmeas; };

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: run_bank_grad lds_limit < numbers\n"); return 2; }
    g_limit = (size_t)atoll(argv[1]);
    if (g_limit > (size_t)kLdsDoubles * 8) { fprintf(stderr, "bad limit\n"); return 2; }
    mpcx::LmpcDev M;
    memset(&M, 0, sizeof(M));
    M.nx = next_i(); M.nu = next_i(); M.ndu = next_i(); M.ny = next_i(); M.ph = next_i(); M.nz = next_i(); M.mg = next_i(); M.ldz = next_i(); M.ldg = next_i();
    M.ldy = next_i(); M.active_words = next_i(); M.n_soft = next_i(); M.m_ref = next_i(); M.adaptive_rho = next_i();
    const int K = next_i(), batch = next_i();
    int want[22];
    for (int &w : want) w = next_i();
    if (M.nx < 1 || M.nu < 1 || M.ndu < 0 || M.ny < 1 || M.ph < 1 || M.nz < 1 || M.mg < 0 || M.ldz < M.nz || M.ldg < M.mg || M.ldy != M.ldz + M.ldg || (M.ldy & 1) ||
        batch < 1 || K < 1 || M.m_ref < 1 || M.m_ref > 32 * M.active_words) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const int nx = M.nx, nu = M.nu, ndu = M.ndu, ny = M.ny, ph = M.ph, nc = MPCX_LINEAR_NC(M);
    const std::vector<int> gkind = read_i(M.ldg), gstep = read_i(M.ldg), gcomp = read_i(M.ldg), refrow = read_i(M.ldg), bptr = read_i(M.nz + 1), bref = read_i(-1), blk = read_i(ph + 1);
    M.g_kind = gkind.data(); M.g_step = gstep.data(); M.g_comp = gcomp.data(); M.g_refrow = refrow.data();
    M.boxrow_ptr = bptr.data(); M.boxrow_ref = bref.data(); M.blk = blk.data();
    std::vector<Controller> ctl((size_t)K);
    std::vector<mpcx::LmpcDev> models((size_t)K, M);
    for (int k = 0; k < K; ++k) {
        Controller &c = ctl[(size_t)k];
        c.Y = read_d((long)M.ldy * M.ldy);
        c.model = read_d(nx * nx + nx * nu + ny * nx + nx * ndu + ny * ndu);
        c.wy = read_d((ph + 1) * ny + (MPCX_HAS_TERMINAL(M) ? mpcx::lmpc_terminal_len(nx, ny, ndu) : 0)); c.wu = read_d((ph + 1) * nu); c.wdu = read_d(ph * nu);
        c.sx = read_d(nx + nc * (nx + nu)); c.su = read_d(nu); c.rho_g = read_d(2 * M.ldg); c.lg0 = read_d(M.ldg); c.ug0 = read_d(M.ldg);
        c.yref = read_d(ph * ny); c.uref = read_d(ph * nu); c.duref = read_d(ph * nu); c.dmeas = read_d(ph * ndu);
        mpcx::LmpcDev &D = models[(size_t)k];
        D.Y = c.Y.data(); D.A = c.model.data(); D.B = D.A + nx * nx; D.C = D.B + nx * nu; D.Bd = D.C + ny * nx; D.Dd = D.Bd + nx * ndu;
        D.Wy = c.wy.data(); D.Wu = c.wu.data(); D.Wdu = c.wdu.data(); D.sX = c.sx.data(); D.sU = c.su.data();
        D.rho_g = c.rho_g.data(); D.lg0 = c.lg0.data(); D.ug0 = c.ug0.data();
        D.yref_s = c.yref.data(); D.uref_s = c.uref.data(); D.duref_s = c.duref.data(); D.dmeas_s = c.dmeas.data();
    }
    const size_t nb = (size_t)batch, aw = (size_t)M.active_words, n1 = (size_t)ph + 1;
    const std::vector<double> indexd = read_opt((long)nb);
    const std::vector<int32_t> index(indexd.begin(), indexd.end());
    if (index.empty() && batch != K) { fprintf(stderr, "no model index: the batch must be the bank\n"); return 2; }
    const std::vector<double> ald = read_d((long)(nb * aw)), aud = read_d((long)(nb * aw));
    std::vector<uint32_t> al(nb * aw), au(nb * aw);                  // (words up to 2^32 - 1: through a wider integer)
    for (size_t i = 0; i < al.size(); ++i) { al[i] = (uint32_t)(long long)ald[i]; au[i] = (uint32_t)(long long)aud[i]; }
    const std::vector<double> statd = read_opt((long)nb);
    const std::vector<int32_t> status(statd.begin(), statd.end());
    const std::vector<double> sc = read_opt((long)(nb * nu)), si = read_opt((long)(nb * n1 * nu));
    const std::vector<double> u0 = read_d((long)(nb * nu)), sx = read_opt((long)(nb * n1 * nx)), so = read_d((long)(nb * n1 * ny)), sq = read_d((long)(nb * n1 * nu));
    const std::vector<double> yr = read_opt((long)(nb * ny));
    const std::vector<double> ordd = read_opt((long)nb), offd = read_opt((long)K + 1);
    const std::vector<int32_t> order(ordd.begin(), ordd.end()), offsets(offd.begin(), offd.end());

    const size_t len[10] = {(size_t)ny * ph, (size_t)nu * ph, (size_t)nu * ph, (size_t)M.m_ref, (size_t)M.m_ref,
                            (size_t)nx * nx, (size_t)nx * nu, (size_t)ny * nx, (size_t)nx * ndu, (size_t)ny * ndu};
    std::vector<double> dv[10], cv[10];
    for (int k = 0; k < 10; ++k) { dv[k].assign(nb * len[k] + kPad, kGuard); cv[k].assign((size_t)K * len[k] + kPad, kGuard); }
    std::vector<int32_t> flags(nb + kPad, kGuardI), n_used((size_t)K + kPad, kGuardI);
    for (double &v : mpcx::smem) v = kGuard;
    mpcx::LmpcBankGradArgs a{};
    a.batch = batch; a.active_lower = al.data(); a.active_upper = au.data();
    a.status = status.empty() ? nullptr : status.data();
    a.seed_cmd = sc.empty() ? nullptr : sc.data(); a.seed_input = si.empty() ? nullptr : si.data();
    a.u0 = u0.data(); a.seq_state = sx.empty() ? nullptr : sx.data(); a.seq_output = so.data(); a.seq_input = sq.data();
    a.yref = yr.empty() ? nullptr : yr.data(); a.yref_bs = yr.empty() ? 0 : ny; a.yref_ks = yr.empty() ? ny : 0;
    a.uref = nullptr; a.uref_bs = 0; a.uref_ks = nu;              // each controller's own
    a.duref = nullptr; a.duref_bs = 0; a.duref_ks = nu;
    a.dmeas = nullptr; a.dmeas_bs = 0; a.dmeas_ks = ndu;
    double **dp[10] = {&a.d_oweight, &a.d_uweight, &a.d_duweight, &a.d_lower, &a.d_upper, &a.d_A, &a.d_B, &a.d_C, &a.d_Bd, &a.d_Dd};
    double **cp[10] = {&a.c_oweight, &a.c_uweight, &a.c_duweight, &a.c_lower, &a.c_upper, &a.c_A, &a.c_B, &a.c_C, &a.c_Bd, &a.c_Dd};
    for (int k = 0; k < 10; ++k) { *dp[k] = want[k] ? dv[k].data() : nullptr; *cp[k] = want[11 + k] ? cv[k].data() : nullptr; }
    a.flags = want[10] ? flags.data() : nullptr; a.n_used = want[21] ? n_used.data() : nullptr;
    a.models = models.data(); a.model_index = index.empty() ? nullptr : index.data(); a.n_models = K;
    a.group_order = order.empty() ? nullptr : order.data(); a.group_offsets = offsets.empty() ? nullptr : offsets.data();
    const int rc = mpcx::lmpc_bank_grad_launch(models[0], a, nullptr);
    for (size_t i = g_limit / 8; i < sizeof(mpcx::smem) / sizeof(double); ++i)
        if (mpcx::smem[i] != kGuard) { fprintf(stderr, "LDS behind the limit was written (double %zu)\n", i); return 4; }
    static const char *const dn[10] = {"d_oweight", "d_uweight", "d_duweight", "d_lower", "d_upper", "d_A", "d_B", "d_C", "d_Bd", "d_Dd"};
    static const char *const cn[10] = {"c_oweight", "c_uweight", "c_duweight", "c_lower", "c_upper", "c_A", "c_B", "c_C", "c_Bd", "c_Dd"};
    printf("{\"rc\": %d, ", rc);
    for (int k = 0; k < 10; ++k) put(dn[k], dv[k]);
    put_i("flags", flags, ", ");
    for (int k = 0; k < 10; ++k) put(cn[k], cv[k]);
    put_i("n_used", n_used, "}\n");
    return 0;
}
