// TEST INFRASTRUCTURE -- runs the bank's sensitivity kernel (libmpc_amd/csrc/lmpc_bank_sens.hip, compiled unchanged: lmpc_bank_sens_launch,
// lmpc_bank_sensitivity) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so.  Compiled with
// clang++ (the kernel's helpers name the components of an ext_vector_type).
//
//   run_bank_sens <lds_limit bytes> < numbers
//   stdin, whitespace separated: nx nu ny ph nz mg ldz ldg ldy active_words n_soft has_terminal terminal_len nlin K batch jacobian(0|1) has_index has_status
//   has_seed_cmd has_seed_input want_x0 want_u0 want_yref want_flags nboxref, then the structure the controllers share: g_kind, g_step, g_comp, g_refrow
//   [mg each], boxrow_ptr [nz + 1], boxrow_ref [nboxref], blk [ph + 1]; then for each of the K controllers Y [ldy ldy], model [nx nx + nx nu + ny nx]
//   (A | B | C), wOutput [(ph + 1) ny], terminal [terminal_len], wDeltaU [ph nu], scalar [nx + nlin (nx + nu)], sU [nu] (column-major, as
//   mpcx_lmpc_debug_get returns them); then model_index [batch], active_lower, active_upper [batch active_words], status [batch], seed_cmd [batch nu],
//   seed_input [batch (ph + 1) nu] (the optional ones only where announced)
//   stdout: one JSON object: rc (what lmpc_bank_sens_launch returned), d_x0, d_u0, d_yref, flags
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

#include "../../libmpc_amd/csrc/lmpc_bank_sens.hip"

size_t mpcx::lmpc_lds_limit() { return g_limit; }
int mpcx::lmpc_raise_dynamic_lds(LmpcLdsCache &, std::initializer_list<const void *>, size_t bytes) { return bytes <= g_limit ? 0 : -3; }

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

struct Controller { std::vector<double> Y, model, wy, wdu, scalar, sU; };

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: run_bank_sens lds_limit < numbers\n"); return 2; }
    g_limit = (size_t)atoll(argv[1]);
    if (g_limit > (size_t)kLdsDoubles * 8) { fprintf(stderr, "bad limit\n"); return 2; }
    mpcx::LmpcDev M;
    memset(&M, 0, sizeof(M));
    M.nx = next_i(); M.nu = next_i(); M.ny = next_i(); M.ph = next_i(); M.nz = next_i(); M.mg = next_i(); M.ldz = next_i(); M.ldg = next_i(); M.ldy = next_i();
    M.active_words = next_i(); M.n_soft = next_i();
    const int has_term = next_i(), term_len = next_i(), nlin = next_i(), K = next_i();
    const int batch = next_i(), jac = next_i(), has_index = next_i(), has_status = next_i(), has_sc = next_i(), has_si = next_i();
    const int want_x0 = next_i(), want_u0 = next_i(), want_yref = next_i(), want_flags = next_i(), nboxref = next_i();
    if (M.nx < 1 || M.nu < 1 || M.ny < 1 || M.ph < 1 || M.nz < 1 || M.mg < 0 || M.ldz < M.nz || M.ldg < M.mg || M.ldy != M.ldz + M.ldg || (M.ldy & 1) || batch < 1 ||
        K < 1 || nlin < 0 || nlin > 63 || term_len < 0 || (!has_term && term_len) || nboxref < 0 || (!has_index && batch != K)) { fprintf(stderr, "bad dimensions\n"); return 2; }
    M.adaptive_rho = (has_term ? 2 : 0) | (nlin << 2);
    const std::vector<int> kind = read_i(M.mg), step = read_i(M.mg), comp = read_i(M.mg), refrow = read_i(M.mg);
    const std::vector<int> bptr = read_i(M.nz + 1), bref = read_i(nboxref), blk = read_i(M.ph + 1);
    M.g_kind = kind.data(); M.g_step = step.data(); M.g_comp = comp.data(); M.g_refrow = refrow.data();
    M.boxrow_ptr = bptr.data(); M.boxrow_ref = bref.data(); M.blk = blk.data();
    std::vector<Controller> ctl((size_t)K);
    std::vector<mpcx::LmpcDev> models((size_t)K, M);
    for (int k = 0; k < K; ++k) {
        Controller &c = ctl[(size_t)k];
        c.Y = read_d((size_t)M.ldy * M.ldy);
        c.model = read_d((size_t)M.nx * M.nx + (size_t)M.nx * M.nu + (size_t)M.ny * M.nx);
        c.wy = read_d((size_t)(M.ph + 1) * M.ny);
        const std::vector<double> t = read_d((size_t)term_len);
        c.wy.insert(c.wy.end(), t.begin(), t.end());               // the terminal block rides behind the output weights (MPCX_TERMINAL)
        c.wdu = read_d((size_t)M.ph * M.nu);
        c.scalar = read_d((size_t)M.nx + (size_t)nlin * (M.nx + M.nu));      // sX, then the linear rows (MPCX_LINEAR_F)
        c.sU = read_d(M.nu);
        mpcx::LmpcDev &D = models[(size_t)k];
        D.Y = c.Y.data(); D.A = c.model.data(); D.B = D.A + (size_t)M.nx * M.nx; D.C = D.B + (size_t)M.nx * M.nu;
        D.Wy = c.wy.data(); D.Wdu = c.wdu.data(); D.sX = c.scalar.data(); D.sU = c.sU.data();
    }
    const size_t nb = (size_t)batch, aw = (size_t)M.active_words;
    const std::vector<int> index = has_index ? read_i(nb) : std::vector<int>();
    std::vector<uint32_t> al(nb * aw), au(nb * aw);                  // (words up to 2^32 - 1: through a wider integer)
    for (uint32_t &w : al) w = (uint32_t)(long long)next_d();
    for (uint32_t &w : au) w = (uint32_t)(long long)next_d();
    const std::vector<int> status = has_status ? read_i(nb) : std::vector<int>();
    const std::vector<double> sc = has_sc ? read_d(nb * M.nu) : std::vector<double>(), si = has_si ? read_d(nb * (M.ph + 1) * M.nu) : std::vector<double>();
    const size_t R = jac ? (size_t)M.nu : 1;
    std::vector<double> dx(nb * R * M.nx + kPad, kGuard), du(nb * R * M.nu + kPad, kGuard), dy(nb * R * M.ny + kPad, kGuard);
    std::vector<int32_t> flags(nb + kPad, kGuardI);
    for (double &v : mpcx::smem) v = kGuard;
    mpcx::LmpcBankSensArgs a{};
    a.s.batch = batch; a.s.jacobian = jac != 0; a.s.active_lower = al.data(); a.s.active_upper = au.data();
    a.s.status = has_status ? reinterpret_cast<const int32_t *>(status.data()) : nullptr;
    a.s.seed_cmd = has_sc ? sc.data() : nullptr; a.s.seed_input = has_si ? si.data() : nullptr;
    a.s.d_x0 = want_x0 ? dx.data() : nullptr; a.s.d_u0 = want_u0 ? du.data() : nullptr; a.s.d_yref = want_yref ? dy.data() : nullptr;
    a.s.flags = want_flags ? flags.data() : nullptr;
    a.models = models.data(); a.model_index = has_index ? reinterpret_cast<const int32_t *>(index.data()) : nullptr; a.n_models = K;
    const int rc = mpcx::lmpc_bank_sens_launch(models[0], a, nullptr);
    for (size_t i = g_limit / 8; i < sizeof(mpcx::smem) / sizeof(double); ++i)
        if (mpcx::smem[i] != kGuard) { fprintf(stderr, "LDS behind the limit was written (double %zu)\n", i); return 4; }
    printf("{\"rc\": %d, ", rc);
    put("d_x0", dx); put("d_u0", du); put("d_yref", dy);
    printf("\"flags\": [");
    for (size_t i = 0; i < flags.size(); ++i) printf("%s%d", i ? ", " : "", (int)flags[i]);
    printf("]}\n");
    return 0;
}
