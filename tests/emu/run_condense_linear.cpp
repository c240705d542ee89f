// TEST INFRASTRUCTURE -- run_condense.cpp for controllers with linear rows: runs the bank's condensing kernel
// (libmpc_amd/csrc/lmpc_hetero.hip, compiled unchanged: lmpc_condense_launch and lmpc_condense_models in both forms) through the lock-step
// interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so.  Compiled with clang++ (the kernel's helpers name the
// components of an ext_vector_type).  The input is run_condense's with `nc, Fx [nc nx], Fu [nc nu]` (column-major) behind sU: the runner lays the
// coefficients out behind sX as the device reads them (MPCX_LINEAR_F: row c as Fx(c, :), Fu(c, :)) and files nc in the flag word (MPCX_LINEAR_NC).
//
//   run_condense_linear <count> < numbers
//   stdin, whitespace separated, per controller: nx nu ny ph nz mg ldz ldg ldy flags (LmpcDev::adaptive_rho: bit 0 adaptive, bit 1 terminal) rho_user
//   sigma, then A [nx nx], B [nx nu], C [ny nx] column-major, Wy [(ph + 1) ny] and with the terminal bit [P nx nx | xT nx | Tx nx ny] behind it,
//   Wu [(ph + 1) nu], Wdu [ph nu], sX [nx], sU [nu], blk [ph + 1], g_kind, g_step, g_comp [ldg], lw, uw [ldz], lg0, ug0, g_soft [ldg]
//   stdout: one JSON object: rc (what lmpc_condense_launch returned), lds (bytes of the plan), big (doubles of a scratch block, 0: the LDS form) and
//   per controller H, Kinv, Gr, Gc, Y, rho_b, rho_g (the step sizes and g_soft behind them), cost_direct, cond_status
// Every output array starts as the host lays it out (zeros; ones for rho_g) and is followed by a guard of kPad elements that must come back
// untouched (the test checks them).  The kernel's LDS is one array of the size of the limit and a guard: whatever lies behind the plan's bytes must
// come back untouched too (exit status 4); the interpreter's hipFree checks the guard behind the scratch blocks.  With MPCX_CONDENSE_GRID_LDS /
// MPCX_CONDENSE_GRID_BIG defined on the command line a workgroup condenses more than one controller.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

// static and dynamic LDS of the kernel: the fibres of a workgroup are one thread, so thread storage is what they share
#undef __shared__
#define __shared__ thread_local

constexpr int kPad = 64, kLdsDoubles = 160 * 1024 / 8;
constexpr double kGuard = -7.25e300;

// the kernel's `extern __shared__ double smem[]`: a block-scope declaration, so a member of the namespace around the kernel
namespace mpcx { namespace { alignas(64) thread_local double smem[kLdsDoubles + kPad]; } }

#include "../../libmpc_amd/csrc/lmpc_hetero.hip"

size_t mpcx::lmpc_lds_limit() { return (size_t)kLdsDoubles * 8; }

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

struct Controller {
    std::vector<double> A, B, C, Wy, Wu, Wdu, sX, sU, lw, uw, lg0, ug0;
    std::vector<int> blk, kind, step, comp;
    std::vector<double> H, Kinv, Gr, Gc, Y, rho_b, rho_g;
};

static std::vector<double> out_array(size_t n, double fill) { std::vector<double> v(n + kPad, kGuard); std::fill(v.begin(), v.begin() + n, fill); return v; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: run_condense_linear count < numbers\n"); return 2; }
    const int count = atoi(argv[1]);
    if (count < 1) { fprintf(stderr, "bad count\n"); return 2; }
    std::vector<std::unique_ptr<Controller>> cs;
    std::vector<mpcx::LmpcDev> models((size_t)count);
    for (int k = 0; k < count; ++k) {
        mpcx::LmpcDev &M = models[k];
        memset(&M, 0, sizeof(M));
        M.nx = next_i(); M.nu = next_i(); M.ny = next_i(); M.ph = next_i(); M.nz = next_i(); M.mg = next_i(); M.ldz = next_i(); M.ldg = next_i(); M.ldy = next_i();
        M.adaptive_rho = next_i(); M.rho_user = next_d(); M.sigma = next_d();
        if (M.nx < 1 || M.nu < 1 || M.ny < 1 || M.ph < 1 || M.nz < 1 || M.mg < 0 || M.ldz < M.nz || M.ldg < M.mg || M.ldy != M.ldz + M.ldg) { fprintf(stderr, "bad dimensions\n"); return 2; }
        cs.emplace_back(new Controller);
        Controller &c = *cs.back();
        const size_t nx = M.nx, nu = M.nu, ny = M.ny, ph = M.ph, ldz = M.ldz, ldg = M.ldg, ldy = M.ldy;
        c.A = read_d(nx * nx); c.B = read_d(nx * nu); c.C = read_d(ny * nx);
        c.Wy = read_d((ph + 1) * ny + (MPCX_HAS_TERMINAL(M) ? nx * nx + nx + nx * ny : 0));
        c.Wu = read_d((ph + 1) * nu); c.Wdu = read_d(ph * nu); c.sX = read_d(nx); c.sU = read_d(nu);
        {
            const int nc = next_i();
            if (nc < 0 || nc > 63 || (M.adaptive_rho >> 2) != 0) { fprintf(stderr, "bad nc\n"); return 2; }
            const std::vector<double> Fx = read_d((size_t)nc * nx), Fu = read_d((size_t)nc * nu);
            for (int r = 0; r < nc; ++r) {
                for (size_t a = 0; a < nx; ++a) c.sX.push_back(Fx[r + a * nc]);
                for (size_t j = 0; j < nu; ++j) c.sX.push_back(Fu[r + j * nc]);
            }
            M.adaptive_rho |= nc << 2;
        }
        c.blk = read_i(ph + 1); c.kind = read_i(ldg); c.step = read_i(ldg); c.comp = read_i(ldg);
        c.lw = read_d(ldz); c.uw = read_d(ldz); c.lg0 = read_d(ldg); c.ug0 = read_d(ldg);
        const std::vector<double> soft = read_d(ldg);
        c.H = out_array(ldz * ldz, 0.0); c.Kinv = out_array(ldz * ldz, 0.0); c.Gr = out_array(ldg * ldz, 0.0); c.Gc = out_array(ldz * ldg, 0.0);
        c.Y = out_array(ldy * ldy, 0.0); c.rho_b = out_array(ldz, 0.0); c.rho_g = out_array(2 * ldg, 1.0);
        std::copy(soft.begin(), soft.end(), c.rho_g.begin() + ldg);
        M.A = c.A.data(); M.B = c.B.data(); M.C = c.C.data(); M.Wy = c.Wy.data(); M.Wu = c.Wu.data(); M.Wdu = c.Wdu.data(); M.sX = c.sX.data(); M.sU = c.sU.data();
        M.blk = c.blk.data(); M.g_kind = c.kind.data(); M.g_step = c.step.data(); M.g_comp = c.comp.data();
        M.lw = c.lw.data(); M.uw = c.uw.data(); M.lg0 = c.lg0.data(); M.ug0 = c.ug0.data();
        M.H = c.H.data(); M.Kinv = c.Kinv.data(); M.Gr = c.Gr.data(); M.Gc = c.Gc.data(); M.Y = c.Y.data(); M.rho_b = c.rho_b.data(); M.rho_g = c.rho_g.data();
        M.cost_direct = -1; M.cond_status = -1;
    }
    for (double &v : mpcx::smem) v = kGuard;
    int NP = 0, NQ = 0;
    size_t big = 0;
    const size_t lds = mpcx::lmpc_condense_lds(models[0], &NP, &NQ, &big);
    const int rc = mpcx::lmpc_condense_launch(models.data(), models[0], count, nullptr);
    for (size_t i = rc == 0 ? (lds + 7) / 8 : 0; i < sizeof(mpcx::smem) / sizeof(double); ++i)
        if (mpcx::smem[i] != kGuard) { fprintf(stderr, "LDS behind the kernel's plan was written (double %zu of %zu)\n", i, lds / 8); return 4; }
    printf("{\"rc\": %d, \"lds\": %zu, \"big\": %zu, \"controllers\": [", rc, lds, big);
    for (int k = 0; k < count; ++k) {
        const Controller &c = *cs[k];
        printf("%s{", k ? ", " : "");
        put("H", c.H); put("Kinv", c.Kinv); put("Gr", c.Gr); put("Gc", c.Gc); put("Y", c.Y); put("rho_b", c.rho_b); put("rho_g", c.rho_g);
        printf("\"cost_direct\": %d, \"cond_status\": %d}", models[k].cost_direct, models[k].cond_status);
    }
    printf("]}\n");
    return 0;
}
