// TEST INFRASTRUCTURE -- runs the observed advance body of include/mpcx/nlmpc_ekf.hpp (the extended Kalman filter in the closed loop around the
// NLMPC solve) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so, no solve -- the
// commands and the solve's per-instance results of every tick are read from stdin.  The interpreter has no integer atomics and no fence, so the
// __global__ wrappers here pass the tick as an argument where the library's read a counter in device memory.  The unobserved body
// (mpcx/nlmpc_loop.hpp) runs on the same inputs beside it: its states are what the observed body's truth rows are compared with.
//
//   run_nlmpc_ekf <model> <Ts> <substeps> <B> <ticks> <ny> <noise 0|1> <params 0|1> <plant_params 0|1> <meas_noise 0|1> <xhat0 0|1> < numbers
//     model: vanderpol | ugv | osc6 | osc8
//   stdin, whitespace separated: the controller's parameters [np] (np = max(1, NPARAMS)), x0 [B nx], u0 [B nu], per tick cmd [B nu] cost [B]
//     status [B] solver_status [B] is_feasible [B] iterations [B], Cm [ny nx] Q [nx nx] R [ny ny] P0 [nx nx] (column-major), then noise [ticks B nx],
//     params [B np], plant_params [B np], meas_noise [ticks B ny], xhat0 [B nx] where switched on
//   stdout: one JSON object; every array is followed by a guard of kPad elements that must come back untouched (doubles kGuard, ints kGuardI)
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "mpcx/nlmpc_ekf.hpp"

namespace mpcx { namespace engine {
alignas(64) double smem[64];
extern double lds_base[] __attribute__((alias("_ZN4mpcx6engine4smemE")));
} }

using namespace mpcx;

constexpr int kPad = 64;
constexpr double kGuard = -7.25e300;
constexpr int kGuardI = -777;

template <class Mdl>
__global__ void ekf_advance_with_tick(const NlmpcDev M, const NlmpcLoopDev L, const NlmpcEkfDev E, const int k)
{
    static double lds[engine::EkfLay<Mdl::NX>::DOUBLES + kPad];       // (one array for the fibres of a block, as LDS is; the guard is checked by main)
    static bool fresh = true;
    if (fresh) { fresh = false; for (double &v : lds) v = kGuard; }
    engine::ekf_advance_tile<Mdl>(M, L, E, k, lds);
    if (threadIdx.x == 63)
        for (int i = 0; i < kPad; ++i)
            if (lds[engine::EkfLay<Mdl::NX>::DOUBLES + i] != kGuard) { fprintf(stderr, "the guard behind the LDS slices was written\n"); exit(4); }
}
template <class Mdl>
__global__ void advance_with_tick(const NlmpcDev M, const NlmpcLoopDev L, const int k)
{
    engine::loop_advance_tile<Mdl>(M, L, k);
}

static double next_d()
{
    double v;
    if (scanf("%lf", &v) != 1) { fprintf(stderr, "input ended early\n"); exit(3); }
    return v;
}
static std::vector<double> read_d(size_t n) { std::vector<double> v(n); for (double &x : v) x = next_d(); return v; }
static void put(const char *name, const std::vector<double> &v, bool last = false)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%.17g", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}
static void put(const char *name, const std::vector<int> &v, bool last = false)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}

template <class Mdl>
static int run(char **argv)
{
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NP = Mdl::NPARAMS > 0 ? Mdl::NPARAMS : 1;
    const double Ts = atof(argv[2]);
    const int substeps = atoi(argv[3]), B = atoi(argv[4]), ticks = atoi(argv[5]), ny = atoi(argv[6]);
    const bool with_noise = atoi(argv[7]) != 0, with_params = atoi(argv[8]) != 0, with_plant = atoi(argv[9]) != 0, with_meas = atoi(argv[10]) != 0,
               with_xhat0 = atoi(argv[11]) != 0;
    if (ny < 1 || ny > NX) { fprintf(stderr, "ny out of range\n"); return 2; }
    const size_t nb = (size_t)B, m = (size_t)ny;
    NlmpcDev M{};
    M.nx = NX; M.nu = NU; M.Ts = Ts;
    const std::vector<double> prm = read_d(NP), x0 = read_d(nb * NX), u0 = read_d(nb * NU);
    M.params = prm.data();
    std::vector<std::vector<double>> cmd(ticks), cost(ticks);
    std::vector<std::vector<int>> ints(ticks);
    for (int k = 0; k < ticks; ++k) {
        cmd[k] = read_d(nb * NU); cost[k] = read_d(nb);
        for (double v : read_d(4 * nb)) ints[k].push_back((int)v);
    }
    const size_t ncb = m * NX + NX * NX + m * m + NX * NX;
    auto guarded = [](size_t n) { return std::vector<double>(n + kPad, kGuard); };
    auto guarded_i = [](size_t n) { return std::vector<int>(n + kPad, kGuardI); };
    std::vector<double> cb = guarded(ncb);
    { const std::vector<double> c = read_d(ncb); std::copy(c.begin(), c.end(), cb.begin()); }
    std::vector<double> noise, params, plant, meas, xhat0;
    if (with_noise) noise = read_d((size_t)ticks * nb * NX);
    if (with_params) params = read_d(nb * NP);
    if (with_plant) plant = read_d(nb * NP);
    if (with_meas) meas = read_d((size_t)ticks * nb * m);
    if (with_xhat0) xhat0 = read_d(nb * NX);

    const size_t T1 = (size_t)ticks + 1, T = (size_t)ticks;
    std::vector<double> x = guarded(nb * NX), xt = guarded(nb * NX), u = guarded(nb * NU), P = guarded(nb * NX * NX), tx = guarded(T1 * nb * NX), tu = guarded(T * nb * NU),
                        tc = guarded(T * nb), txh = guarded(T1 * nb * NX), ty = guarded(T * nb * m), tP = guarded(T1 * nb * NX * NX), cmd_d(nb * NU), cost_d(nb);
    std::vector<double> px = guarded(nb * NX), pu = guarded(nb * NU), ptx = guarded(T1 * nb * NX), ptu = guarded(T * nb * NU);      // the unobserved body's
    std::vector<int> ts = guarded_i(T * nb), tss = guarded_i(T * nb), tf = guarded_i(T * nb), ti = guarded_i(T * nb), flags = guarded_i(nb), ints_d(4 * nb);
    // what the library's begin kernels do
    const std::vector<double> &xh0 = with_xhat0 ? xhat0 : x0;
    std::copy(x0.begin(), x0.end(), xt.begin()); std::copy(x0.begin(), x0.end(), tx.begin()); std::copy(u0.begin(), u0.end(), u.begin());
    std::copy(xh0.begin(), xh0.end(), x.begin()); std::copy(xh0.begin(), xh0.end(), txh.begin());
    for (size_t b = 0; b < nb; ++b)
        for (size_t i = 0; i < (size_t)NX * NX; ++i) P[b * NX * NX + i] = tP[b * NX * NX + i] = cb[m * NX + NX * NX + m * m + i];
    std::fill(flags.begin(), flags.begin() + B, 0);
    std::copy(x0.begin(), x0.end(), px.begin()); std::copy(x0.begin(), x0.end(), ptx.begin()); std::copy(u0.begin(), u0.end(), pu.begin());

    NlmpcLoopDev L{};
    L.batch = B; L.ticks = ticks; L.substeps = substeps; L.nparams = NP;
    L.params = with_params ? params.data() : nullptr; L.plant_params = with_plant ? plant.data() : nullptr; L.noise = with_noise ? noise.data() : nullptr;
    L.x = x.data(); L.u = u.data(); L.cmd = cmd_d.data(); L.cost = cost_d.data();
    L.status = ints_d.data(); L.solver_status = ints_d.data() + nb; L.is_feasible = ints_d.data() + 2 * nb; L.iterations = ints_d.data() + 3 * nb;
    L.traj_x = tx.data(); L.traj_u = tu.data(); L.traj_cost = tc.data();
    L.traj_status = ts.data(); L.traj_solver_status = tss.data(); L.traj_is_feasible = tf.data(); L.traj_iterations = ti.data();
    NlmpcEkfDev E{};
    E.ny = ny; E.cb = cb.data(); E.meas_noise = with_meas ? meas.data() : nullptr;
    E.xt = xt.data(); E.P = P.data(); E.traj_xhat = txh.data(); E.traj_y = ty.data(); E.traj_P = tP.data(); E.flags = flags.data();
    NlmpcLoopDev Lp = L;                    // the unobserved loop on the same commands: only the states and commands are kept
    Lp.x = px.data(); Lp.u = pu.data(); Lp.traj_x = ptx.data(); Lp.traj_u = ptu.data();
    Lp.traj_cost = nullptr; Lp.traj_status = Lp.traj_solver_status = Lp.traj_is_feasible = Lp.traj_iterations = nullptr;
    constexpr int ipw = engine::EkfLay<NX>::IPW;
    for (int k = 0; k < ticks; ++k) {
        cmd_d = cmd[k]; cost_d = cost[k]; ints_d = ints[k];      // (assignments of equal length: the buffers stay where they are)
        hipLaunchKernelGGL(ekf_advance_with_tick<Mdl>, dim3((B + ipw - 1) / ipw), dim3(64), 0, nullptr, M, L, E, k);
        hipLaunchKernelGGL(advance_with_tick<Mdl>, dim3((B + engine::kLoopTile - 1) / engine::kLoopTile), dim3(engine::kLoopTile), 0, nullptr, M, Lp, k);
    }
    printf("{");
    put("x", x); put("xt", xt); put("u", u); put("P", P); put("cb", cb); put("traj_x", tx); put("traj_u", tu); put("traj_cost", tc);
    put("traj_xhat", txh); put("traj_y", ty); put("traj_P", tP); put("flags", flags); put("plain_traj_x", ptx);
    put("traj_status", ts); put("traj_solver_status", tss); put("traj_is_feasible", tf); put("traj_iterations", ti, true);
    printf("}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 12) { fprintf(stderr, "usage: run_nlmpc_ekf model Ts substeps B ticks ny noise params plant_params meas_noise xhat0\n"); return 2; }
    const std::string m = argv[1];
    using namespace mpcx::models;
    if (m == "vanderpol") return run<VanDerPol>(argv);
    if (m == "ugv") return run<Ugv>(argv);
    if (m == "osc6") return run<Oscillators<6>>(argv);
    if (m == "osc8") return run<Oscillators<8>>(argv);
    fprintf(stderr, "unknown model %s\n", m.c_str());
    return 2;
}
