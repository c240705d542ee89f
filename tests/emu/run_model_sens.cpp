// TEST INFRASTRUCTURE -- runs the model-sensitivity kernels (libmpc_amd/csrc/lmpc_model_sens.hip, compiled unchanged: lmpc_model_sens_launch,
// lmpc_model_sensitivity, lmpc_sens_reduce) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of
// libmpcx.so.  Compiled with clang++ (the kernel's helpers name the components of an ext_vector_type).
//
//   run_model_sens <lds_limit bytes> < numbers
//   stdin, whitespace separated: nx nu ndu ny ph nz mg ldz ldg ldy nz16 active_words n_soft m_ref flag_word (LmpcDev::adaptive_rho) batch reduce
//   want_A want_B want_C want_Bd want_Dd want_flags want_n_used, then arrays, each as its length followed by its values: Y [ldy ldy], Xq [rows16 nz]
//   (both column-major, as mpcx_lmpc_debug_get returns them), A, B, C, Wy (the terminal block behind it), Wu, Wdu, sX (the linear rows behind it), sU,
//   rho_g [2 ldg] (the soft rows' 1 / weight in its second half), lg0, ug0, g_kind, g_step, g_comp, g_refrow, boxrow_ptr, boxrow_ref, blk,
//   active_lower, active_upper [batch active_words], status [batch], seed_cmd [batch nu], seed_input [batch (ph + 1) nu] (length 0: a null pointer),
//   u0 [batch nu], seq_state [batch (ph + 1) nx], seq_output, seq_input, yref [batch ph ny], uref, duref [batch ph nu], dmeas [batch ph ndu]
//   stdout: one JSON object: rc (what lmpc_model_sens_launch returned), d_A, d_B, d_C, d_Bd, d_Dd, flags, n_used
// Every output array is followed by a guard of kPad elements that must come back untouched (the test checks them), an output that was not asked for
// is passed as a null pointer.  The kernel's LDS is one array of the size of the limit and a guard behind it that must come back untouched (exit 4);
// so is the partials buffer (exit 5).
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

#include "../../libmpc_amd/csrc/lmpc_model_sens.hip"

size_t mpcx::lmpc_lds_limit() { return g_limit; }
int mpcx::lmpc_raise_dynamic_lds(LmpcLdsCache &, std::initializer_list<const void *>, size_t bytes) { return bytes <= g_limit ? 0 : -3; }
void mpcx::lmpc_pack_mfma_tiles(const double *src, int rows, int K, double *out)      // lmpc_model.cpp's, restated
{
    const int T = rows / 16, G = (K + 15) / 16;
    for (int t = 0; t < T; t++)
        for (int g = 0; g < G; g++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 4; e++) {
                    const int k = 4 * (4 * g + e) + (lane >> 4);
                    out[(((size_t)t * G + g) * 64 + lane) * 4 + e] = k < K ? src[(size_t)k * rows + 16 * t + (lane & 15)] : 0.0;
                }
}

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

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: run_model_sens lds_limit < numbers\n"); return 2; }
    g_limit = (size_t)atoll(argv[1]);
    if (g_limit > (size_t)kLdsDoubles * 8) { fprintf(stderr, "bad limit\n"); return 2; }
    mpcx::LmpcDev M;
    memset(&M, 0, sizeof(M));
    M.nx = next_i(); M.nu = next_i(); M.ndu = next_i(); M.ny = next_i(); M.ph = next_i(); M.nz = next_i(); M.mg = next_i(); M.ldz = next_i(); M.ldg = next_i();
    M.ldy = next_i(); M.nz16 = next_i(); M.active_words = next_i(); M.n_soft = next_i(); M.m_ref = next_i(); M.adaptive_rho = next_i();
    const int batch = next_i(), reduce = next_i();
    int want[7];
    for (int &w : want) w = next_i();
    if (M.nx < 1 || M.nu < 1 || M.ndu < 0 || M.ny < 1 || M.ph < 1 || M.nz < 1 || M.mg < 0 || M.ldz < M.nz || M.ldg < M.mg || M.ldy != M.ldz + M.ldg || batch < 1 ||
        M.nz16 < M.nz || M.nz16 % 16 || M.m_ref < 1 || M.m_ref > 32 * M.active_words) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const int nx = M.nx, nu = M.nu, ndu = M.ndu, ny = M.ny, ph = M.ph;
    const int rows16 = (nx * ph + 15) / 16 * 16;
    const int nc = MPCX_LINEAR_NC(M);
    const std::vector<double> Y = read_d((long)M.ldy * M.ldy), Xq = read_d((long)rows16 * M.nz);
    const std::vector<double> A = read_d(nx * nx), Bm = read_d(nx * nu), Cm = read_d(ny * nx);
    const std::vector<double> Wy = read_d((ph + 1) * ny + (MPCX_HAS_TERMINAL(M) ? mpcx::lmpc_terminal_len(nx, ny, ndu) : 0)), Wu = read_d((ph + 1) * nu), Wdu = read_d(ph * nu);
    const std::vector<double> sX = read_d(nx + nc * (nx + nu)), sU = read_d(nu), rho_g = read_d(2 * M.ldg), lg0 = read_d(M.ldg), ug0 = read_d(M.ldg);
    const std::vector<int> gkind = read_i(M.ldg), gstep = read_i(M.ldg), gcomp = read_i(M.ldg), refrow = read_i(M.ldg), bptr = read_i(M.nz + 1), bref = read_i(-1), blk = read_i(ph + 1);
    const size_t nb = (size_t)batch, aw = (size_t)M.active_words, n1 = (size_t)ph + 1;
    const std::vector<double> ald = read_d((long)(nb * aw)), aud = read_d((long)(nb * aw));
    std::vector<uint32_t> al(nb * aw), au(nb * aw);                  // (words up to 2^32 - 1: through a wider integer)
    for (size_t i = 0; i < al.size(); ++i) { al[i] = (uint32_t)(long long)ald[i]; au[i] = (uint32_t)(long long)aud[i]; }
    const std::vector<double> statd = read_opt((long)nb);
    const std::vector<int32_t> status(statd.begin(), statd.end());
    const std::vector<double> sc = read_opt((long)(nb * nu)), si = read_opt((long)(nb * n1 * nu));
    const std::vector<double> u0 = read_d((long)(nb * nu)), sx = read_d((long)(nb * n1 * nx)), so = read_d((long)(nb * n1 * ny)), sq = read_d((long)(nb * n1 * nu));
    const std::vector<double> yr = read_d((long)(nb * ph * ny)), ur = read_d((long)(nb * ph * nu)), dr = read_d((long)(nb * ph * nu)), dm = read_d((long)(nb * ph * ndu));
    M.Y = Y.data(); M.A = A.data(); M.B = Bm.data(); M.C = Cm.data(); M.Wy = Wy.data(); M.Wu = Wu.data(); M.Wdu = Wdu.data(); M.sX = sX.data(); M.sU = sU.data();
    M.rho_g = rho_g.data(); M.lg0 = lg0.data(); M.ug0 = ug0.data();
    M.g_kind = gkind.data(); M.g_step = gstep.data(); M.g_comp = gcomp.data(); M.g_refrow = refrow.data();
    M.boxrow_ptr = bptr.data(); M.boxrow_ref = bref.data(); M.blk = blk.data();
    std::vector<double> Xqp(mpcx::lmpc_packed_len(rows16, M.nz));
    mpcx::lmpc_pack_mfma_tiles(Xq.data(), rows16, M.nz, Xqp.data());
    const size_t lead = reduce ? 1 : nb;
    std::vector<double> gA(lead * nx * nx + kPad, kGuard), gB(lead * nx * nu + kPad, kGuard), gC(lead * ny * nx + kPad, kGuard);
    std::vector<double> gBd(lead * nx * ndu + kPad, kGuard), gDd(lead * ny * ndu + kPad, kGuard);
    std::vector<int32_t> flags(nb + kPad, kGuardI), n_used(1 + kPad, kGuardI);
    const size_t plen = mpcx::lmpc_model_sens_partials(M, batch);
    std::vector<double> part(plen + kPad, kGuard);
    for (double &v : mpcx::smem) v = kGuard;
    mpcx::LmpcModelSensArgs a{};
    a.batch = batch; a.reduce = reduce != 0; a.active_lower = al.data(); a.active_upper = au.data();
    a.status = status.empty() ? nullptr : status.data();
    a.seed_cmd = sc.empty() ? nullptr : sc.data(); a.seed_input = si.empty() ? nullptr : si.data();
    a.u0 = u0.data(); a.seq_state = sx.data(); a.seq_output = so.data(); a.seq_input = sq.data();
    a.yref = yr.data(); a.yref_bs = (long)ph * ny; a.yref_ks = ny;
    a.uref = ur.data(); a.uref_bs = (long)ph * nu; a.uref_ks = nu;
    a.duref = dr.data(); a.duref_bs = (long)ph * nu; a.duref_ks = nu;
    a.dmeas = ndu ? dm.data() : nullptr; a.dmeas_bs = (long)ph * ndu; a.dmeas_ks = ndu;
    a.d_A = want[0] ? gA.data() : nullptr; a.d_B = want[1] ? gB.data() : nullptr; a.d_C = want[2] ? gC.data() : nullptr;
    a.d_Bd = want[3] ? gBd.data() : nullptr; a.d_Dd = want[4] ? gDd.data() : nullptr;
    a.flags = want[5] ? flags.data() : nullptr; a.n_used = want[6] ? n_used.data() : nullptr;
    a.partials = reduce ? part.data() : nullptr;
    const int rc = mpcx::lmpc_model_sens_launch(M, &M, Xqp.data(), a, nullptr);
    for (size_t i = g_limit / 8; i < sizeof(mpcx::smem) / sizeof(double); ++i)
        if (mpcx::smem[i] != kGuard) { fprintf(stderr, "LDS behind the limit was written (double %zu)\n", i); return 4; }
    for (size_t i = plen; i < part.size(); ++i)
        if (part[i] != kGuard) { fprintf(stderr, "the partials buffer was written behind its end\n"); return 5; }
    printf("{\"rc\": %d, ", rc);
    put("d_A", gA); put("d_B", gB); put("d_C", gC); put("d_Bd", gBd); put("d_Dd", gDd);
    printf("\"flags\": [");
    for (size_t i = 0; i < flags.size(); ++i) printf("%s%d", i ? ", " : "", (int)flags[i]);
    printf("], \"n_used\": [");
    for (size_t i = 0; i < n_used.size(); ++i) printf("%s%d", i ? ", " : "", (int)n_used[i]);
    printf("]}\n");
    return 0;
}
