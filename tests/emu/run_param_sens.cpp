// TEST INFRASTRUCTURE -- runs the parameter-sensitivity kernels (libmpc_amd/csrc/lmpc_param_sens.hip, compiled unchanged: lmpc_param_sens_launch,
// lmpc_param_sensitivity, lmpc_sens_reduce) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of
// libmpcx.so.  Compiled with clang++ (the kernel's helpers name the components of an ext_vector_type).
//
//   run_param_sens <lds_limit bytes> < numbers
//   stdin, whitespace separated: nx nu ny ph nz mg ldz ldg ldy nz16 active_words n_soft m_ref batch reduce has_status has_seed_cmd has_seed_input
//   want_ow want_uw want_duw want_lower want_upper want_flags want_n_used nboxref, then Y [ldy ldy], Cq [rows16 nz] (both column-major, as
//   mpcx_lmpc_debug_get returns them), g_refrow [mg], boxrow_ptr [nz + 1], boxrow_ref [nboxref], blk [ph + 1], active_lower, active_upper
//   [batch active_words], status [batch], seed_cmd [batch nu], seed_input [batch (ph + 1) nu] (the optional ones only where announced), u0 [batch nu],
//   seq_output [batch (ph + 1) ny], seq_input [batch (ph + 1) nu], yref [batch ph ny], uref, duref [batch ph nu] (per-step arrays)
//   stdout: one JSON object: rc (what lmpc_param_sens_launch returned), d_oweight, d_uweight, d_duweight, d_lower, d_upper, flags, n_used
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

#include "../../libmpc_amd/csrc/lmpc_param_sens.hip"

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
static std::vector<double> read_d(size_t n) { std::vector<double> v(n); for (double &x : v) x = next_d(); return v; }
static std::vector<int> read_i(size_t n) { std::vector<int> v(n); for (int &x : v) x = next_i(); return v; }
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
    if (argc < 2) { fprintf(stderr, "usage: run_param_sens lds_limit < numbers\n"); return 2; }
    g_limit = (size_t)atoll(argv[1]);
    if (g_limit > (size_t)kLdsDoubles * 8) { fprintf(stderr, "bad limit\n"); return 2; }
    mpcx::LmpcDev M;
    memset(&M, 0, sizeof(M));
    M.nx = next_i(); M.nu = next_i(); M.ny = next_i(); M.ph = next_i(); M.nz = next_i(); M.mg = next_i(); M.ldz = next_i(); M.ldg = next_i(); M.ldy = next_i();
    M.nz16 = next_i(); M.active_words = next_i(); M.n_soft = next_i(); M.m_ref = next_i();
    const int batch = next_i(), reduce = next_i(), has_status = next_i(), has_sc = next_i(), has_si = next_i();
    int want[7];
    for (int &w : want) w = next_i();
    const int nboxref = next_i();
    if (M.nx < 1 || M.nu < 1 || M.ny < 1 || M.ph < 1 || M.nz < 1 || M.mg < 0 || M.ldz < M.nz || M.ldg < M.mg || M.ldy != M.ldz + M.ldg || batch < 1 ||
        M.nz16 < M.nz || M.nz16 % 16 || nboxref < 0 || M.m_ref < 1 || M.m_ref > 32 * M.active_words) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const int rows16 = (M.ny * M.ph + 15) / 16 * 16;
    const std::vector<double> Y = read_d((size_t)M.ldy * M.ldy), Cq = read_d((size_t)rows16 * M.nz);
    const std::vector<int> refrow = read_i(M.mg), bptr = read_i(M.nz + 1), bref = read_i(nboxref), blk = read_i(M.ph + 1);
    const size_t nb = (size_t)batch, aw = (size_t)M.active_words, n1 = (size_t)M.ph + 1;
    std::vector<uint32_t> al(nb * aw), au(nb * aw);                  // (words up to 2^32 - 1: through a wider integer)
    for (uint32_t &w : al) w = (uint32_t)(long long)next_d();
    for (uint32_t &w : au) w = (uint32_t)(long long)next_d();
    const std::vector<int> status = has_status ? read_i(nb) : std::vector<int>();
    const std::vector<double> sc = has_sc ? read_d(nb * M.nu) : std::vector<double>(), si = has_si ? read_d(nb * n1 * M.nu) : std::vector<double>();
    const std::vector<double> u0 = read_d(nb * M.nu), so = read_d(nb * n1 * M.ny), sq = read_d(nb * n1 * M.nu);
    const std::vector<double> yr = read_d(nb * M.ph * M.ny), ur = read_d(nb * M.ph * M.nu), dr = read_d(nb * M.ph * M.nu);
    M.Y = Y.data(); M.g_refrow = refrow.data(); M.boxrow_ptr = bptr.data(); M.boxrow_ref = bref.data(); M.blk = blk.data();
    std::vector<double> Cqp(mpcx::lmpc_packed_len(rows16, M.nz));
    mpcx::lmpc_pack_mfma_tiles(Cq.data(), rows16, M.nz, Cqp.data());
    const size_t lead = reduce ? 1 : nb, mr = (size_t)M.m_ref;
    std::vector<double> gow(lead * M.ny * M.ph + kPad, kGuard), guw(lead * M.nu * M.ph + kPad, kGuard), gdw(lead * M.nu * M.ph + kPad, kGuard);
    std::vector<double> glo(lead * mr + kPad, kGuard), gup(lead * mr + kPad, kGuard);
    std::vector<int32_t> flags(nb + kPad, kGuardI), n_used(1 + kPad, kGuardI);
    const size_t plen = mpcx::lmpc_param_sens_partials(M, batch);
    std::vector<double> part(plen + kPad, kGuard);
    for (double &v : mpcx::smem) v = kGuard;
    mpcx::LmpcParamSensArgs a{};
    a.batch = batch; a.reduce = reduce != 0; a.active_lower = al.data(); a.active_upper = au.data();
    a.status = has_status ? reinterpret_cast<const int32_t *>(status.data()) : nullptr;
    a.seed_cmd = has_sc ? sc.data() : nullptr; a.seed_input = has_si ? si.data() : nullptr;
    a.u0 = u0.data(); a.seq_output = so.data(); a.seq_input = sq.data();
    a.yref = yr.data(); a.yref_bs = (long)M.ph * M.ny; a.yref_ks = M.ny;
    a.uref = ur.data(); a.uref_bs = (long)M.ph * M.nu; a.uref_ks = M.nu;
    a.duref = dr.data(); a.duref_bs = (long)M.ph * M.nu; a.duref_ks = M.nu;
    a.d_oweight = want[0] ? gow.data() : nullptr; a.d_uweight = want[1] ? guw.data() : nullptr; a.d_duweight = want[2] ? gdw.data() : nullptr;
    a.d_lower = want[3] ? glo.data() : nullptr; a.d_upper = want[4] ? gup.data() : nullptr;
    a.flags = want[5] ? flags.data() : nullptr; a.n_used = want[6] ? n_used.data() : nullptr;
    a.partials = reduce ? part.data() : nullptr;
    const int rc = mpcx::lmpc_param_sens_launch(M, &M, Cqp.data(), a, nullptr);
    for (size_t i = g_limit / 8; i < sizeof(mpcx::smem) / sizeof(double); ++i)
        if (mpcx::smem[i] != kGuard) { fprintf(stderr, "LDS behind the limit was written (double %zu)\n", i); return 4; }
    for (size_t i = plen; i < part.size(); ++i)
        if (part[i] != kGuard) { fprintf(stderr, "the partials buffer was written behind its end\n"); return 5; }
    printf("{\"rc\": %d, ", rc);
    put("d_oweight", gow); put("d_uweight", guw); put("d_duweight", gdw); put("d_lower", glo); put("d_upper", gup);
    printf("\"flags\": [");
    for (size_t i = 0; i < flags.size(); ++i) printf("%s%d", i ? ", " : "", (int)flags[i]);
    printf("], \"n_used\": [");
    for (size_t i = 0; i < n_used.size(); ++i) printf("%s%d", i ? ", " : "", (int)n_used[i]);
    printf("]}\n");
    return 0;
}
