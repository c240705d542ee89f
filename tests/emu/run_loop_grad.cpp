// TEST INFRASTRUCTURE -- runs the begin, adjoint and finish kernels of the closed loop's backward pass (libmpc_amd/csrc/lmpc_loop_grad.hip, compiled
// unchanged) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so.  The launches between two
// adjoint kernels (re-solve, vector-Jacobian products) are not run: their per-tick outputs gx, gu, gy are read from the input, as the reference
// computed them.  Compiled with clang++ (address_space, __hip_atomic_*).
//
//   run_loop_grad < numbers
//   stdin, whitespace separated: nx nu ndu ny ph batch ticks plants(0|1) has_seed_x has_seed_u, then the plant -- plants = 0: [A_p | B_p | Bd_p]
//   each row-major; plants = 1: the packed block, tiles x terms x ipw x nx --, traj_x [(ticks + 1) B nx], traj_u [ticks B nu], u0 [B nu],
//   d [ticks B ndu], seed_x, seed_u (where announced), and per tick k = ticks - 1 .. 0: gx [B nx], gu [B nu], gy [B ny], flags [B]
//   stdout: one JSON object: d_x0, d_u0, d_yref, d_noise, d_plant, c [ticks B nu] (row k: c_k as the replay of tick k read it), x, u (as staged
//   for the last replay), flags, tick (the counter at the end)
// Every output array is followed by a guard of kPad elements that must come back untouched (the test checks them); the kernels' LDS is an array of
// exactly the launch's size and a guard behind it (exit 4).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#undef __shared__
#define __shared__ thread_local

constexpr int kPad = 64, kLdsDoubles = 160 * 1024 / 8;
constexpr double kGuard = -7.25e300;
constexpr int kGuardI = -77;

inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline void __threadfence() {}
// (fibres run one at a time: the counter's atomics are plain accesses)
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __hip_atomic_store(p, v, order, scope) (*(p) = (v))

namespace mpcx { namespace { alignas(64) thread_local double lds[kLdsDoubles + kPad]; alignas(64) thread_local double smem[8]; } }

#include "../../libmpc_amd/csrc/lmpc_loop_grad.hip"

size_t mpcx::lmpc_lds_limit() { return (size_t)kLdsDoubles * 8; }

static double next_d()
{
    double v;
    if (scanf("%lf", &v) != 1) { fprintf(stderr, "input ended early\n"); exit(3); }
    return v;
}
static int next_i() { return (int)next_d(); }
static std::vector<double> read_d(size_t n) { std::vector<double> v(n); for (double &x : v) x = next_d(); return v; }
static void put(const char *name, const std::vector<double> &v, bool last = false)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) {
        if (std::isnan(v[i])) printf("%sNaN", i ? ", " : "");
        else if (std::isinf(v[i])) printf("%s%sInfinity", i ? ", " : "", v[i] < 0 ? "-" : "");
        else printf("%s%.17g", i ? ", " : "", v[i]);
    }
    printf("]%s", last ? "" : ", ");
}

int main()
{
    mpcx::LmpcLoopGradDev G;
    memset(&G, 0, sizeof(G));
    G.nx = next_i(); G.nu = next_i(); G.ndu = next_i(); G.ny = next_i(); G.ph = next_i(); G.batch = next_i(); G.ticks = next_i();
    const int plants = next_i(), has_sx = next_i(), has_su = next_i();
    if (G.nx < 1 || G.nx > 64 || G.nu < 1 || G.ndu < 0 || G.ny < 1 || G.batch < 1 || G.ticks < 1) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const size_t B = (size_t)G.batch, T = (size_t)G.ticks, nx = G.nx, nu = G.nu, ndu = G.ndu, ny = G.ny, npl = nx + nu + ndu;
    G.ipw = G.nx < 64 ? 64 / G.nx : 1;
    mpcx::lmpc_loop_grad_plan_lds(G);
    const size_t tiles = (B + G.ipw - 1) / G.ipw;
    const std::vector<double> plant = read_d(plants ? tiles * npl * G.ipw * nx : nx * npl);
    const std::vector<double> tx = read_d((T + 1) * B * nx), tu = read_d(T * B * nu), u0 = read_d(B * nu), d = read_d(T * B * ndu);
    const std::vector<double> sx = has_sx ? read_d((T + 1) * B * nx) : std::vector<double>(), su = has_su ? read_d(T * B * nu) : std::vector<double>();
    if (plants) G.pk = plant.data(); else G.plant = plant.data();
    G.traj_x = tx.data(); G.traj_u = tu.data(); G.u0 = u0.data();
    G.dmeas = d.data(); G.d_bs = (long)ndu; G.d_tick = (long)(B * ndu);      // d_k of instance b at d[k B ndu + b ndu]
    G.seed_x = has_sx ? sx.data() : nullptr; G.seed_u = has_su ? su.data() : nullptr;
    auto guarded = [](size_t n) { return std::vector<double>(n + kPad, kGuard); };
    std::vector<double> x = guarded(B * nx), u = guarded(B * nu), lam = guarded(B * nx), mu = guarded(B * nu), c = guarded(B * nu);
    std::vector<double> gx = guarded(B * nx), gu = guarded(B * nu), gy = guarded(B * ny);
    std::vector<double> dx0 = guarded(B * nx), du0 = guarded(B * nu), dyref = guarded(B * ny), dnoise = guarded(T * B * nx), dplant = guarded(B * nx * npl);
    std::vector<int32_t> tflags(B + kPad, kGuardI), flags(B + kPad, kGuardI);
    int state[2 + kPad];
    for (int &v : state) v = kGuardI;
    G.x = x.data(); G.u = u.data(); G.lam = lam.data(); G.mu = mu.data(); G.c = c.data();
    G.gx = gx.data(); G.gu = gu.data(); G.gy = gy.data(); G.tflags = tflags.data(); G.ntf = 1;
    G.a_yref = dyref.data(); G.a_plant = dplant.data(); G.d_noise = dnoise.data(); G.d_x0 = dx0.data(); G.d_u0 = du0.data();
    G.flags = flags.data(); G.state = state;
    for (double &v : mpcx::lds) v = kGuard;
    const size_t lds_doubles = (size_t)(plants ? G.ipw : 64) * G.sg;
    if (mpcx::lmpc_loop_grad_prepare(G) != 0 || lds_doubles > (size_t)kLdsDoubles) { fprintf(stderr, "LDS plan\n"); return 2; }
    if (mpcx::lmpc_loop_grad_begin(G, nullptr) != 0) return 5;
    std::vector<double> clog(T * B * nu);
    for (size_t r = 0; r < T; ++r) {
        const int k = state[0];
        if (k != (int)(T - 1 - r)) { fprintf(stderr, "tick counter %d at replay %zu\n", k, r); return 6; }
        memcpy(&clog[(size_t)k * B * nu], c.data(), B * nu * sizeof(double));
        for (size_t i = 0; i < B * nx; ++i) gx[i] = next_d();
        for (size_t i = 0; i < B * nu; ++i) gu[i] = next_d();
        for (size_t i = 0; i < B * ny; ++i) gy[i] = next_d();
        for (size_t i = 0; i < B; ++i) tflags[i] = next_i();
        if (mpcx::lmpc_loop_grad_adjoint(G, nullptr) != 0) return 5;
    }
    const int tick = state[0];
    if (mpcx::lmpc_loop_grad_adjoint(G, nullptr) != 0) return 5;           // a replay past tick 0 stores nothing
    if (mpcx::lmpc_loop_grad_finish(G, nullptr) != 0) return 5;
    for (size_t i = lds_doubles; i < sizeof(mpcx::lds) / sizeof(double); ++i)
        if (mpcx::lds[i] != kGuard) { fprintf(stderr, "LDS behind the launch's size was written (double %zu)\n", i); return 4; }
    for (int i = 2; i < 2 + kPad; ++i)
        if (state[i] != kGuardI) { fprintf(stderr, "state guard\n"); return 4; }
    printf("{\"tick\": %d, \"after\": %d, ", tick, state[0]);
    put("d_x0", dx0); put("d_u0", du0); put("d_yref", dyref); put("d_noise", dnoise); put("d_plant", dplant); put("c", clog);
    put("x", x); put("u", u); put("lam", lam); put("mu", mu);
    printf("\"flags\": [");
    for (size_t i = 0; i < flags.size(); ++i) printf("%s%d", i ? ", " : "", (int)flags[i]);
    printf("]}\n");
    return 0;
}
