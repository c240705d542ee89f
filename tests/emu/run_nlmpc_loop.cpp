// TEST INFRASTRUCTURE -- runs the advance body of include/mpcx/nlmpc_loop.hpp (the closed loop around the NLMPC solve) through the lock-step
// interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so, no solve -- the commands and the solve's per-instance
// results of every tick are read from stdin.  The interpreter has no integer atomics and no fence, so the __global__ wrapper here passes the
// tick as an argument where the library's reads a counter in device memory.
//
//   run_nlmpc_loop <model> <Ts> <substeps> <B> <ticks> <noise 0|1> <params 0|1> <plant_params 0|1> < numbers
//     model: vanderpol | ugv | osc6
//   stdin, whitespace separated: the controller's parameters [np] (np = max(1, NPARAMS)), x0 [B nx], u0 [B nu], per tick cmd [B nu] cost [B]
//     status [B] solver_status [B] is_feasible [B] iterations [B], then noise [ticks B nx], params [B np], plant_params [B np] where switched on
//   stdout: one JSON object; every array is followed by a guard of kPad elements that must come back untouched (doubles kGuard, ints kGuardI)
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "mpcx/nlmpc_loop.hpp"

namespace mpcx { namespace engine {
alignas(64) double smem[64];
extern double lds_base[] __attribute__((alias("_ZN4mpcx6engine4smemE")));
} }

using namespace mpcx;

constexpr int kPad = 64;
constexpr double kGuard = -7.25e300;
constexpr int kGuardI = -777;

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
    const int substeps = atoi(argv[3]), B = atoi(argv[4]), ticks = atoi(argv[5]);
    const bool with_noise = atoi(argv[6]) != 0, with_params = atoi(argv[7]) != 0, with_plant = atoi(argv[8]) != 0;
    const size_t nb = (size_t)B;
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
    std::vector<double> noise, params, plant;
    if (with_noise) noise = read_d((size_t)ticks * nb * NX);
    if (with_params) params = read_d(nb * NP);
    if (with_plant) plant = read_d(nb * NP);

    auto guarded = [](size_t n) { return std::vector<double>(n + kPad, kGuard); };
    auto guarded_i = [](size_t n) { return std::vector<int>(n + kPad, kGuardI); };
    std::vector<double> x = guarded(nb * NX), u = guarded(nb * NU), tx = guarded((size_t)(ticks + 1) * nb * NX), tu = guarded((size_t)ticks * nb * NU),
                        tc = guarded((size_t)ticks * nb), cmd_d(nb * NU), cost_d(nb);
    std::vector<int> ts = guarded_i((size_t)ticks * nb), tss = guarded_i((size_t)ticks * nb), tf = guarded_i((size_t)ticks * nb), ti = guarded_i((size_t)ticks * nb),
                     ints_d(4 * nb);
    // what the library's begin kernel does
    std::copy(x0.begin(), x0.end(), x.begin()); std::copy(x0.begin(), x0.end(), tx.begin()); std::copy(u0.begin(), u0.end(), u.begin());

    NlmpcLoopDev L{};
    L.batch = B; L.ticks = ticks; L.substeps = substeps; L.nparams = NP;
    L.params = with_params ? params.data() : nullptr; L.plant_params = with_plant ? plant.data() : nullptr; L.noise = with_noise ? noise.data() : nullptr;
    L.x = x.data(); L.u = u.data(); L.cmd = cmd_d.data(); L.cost = cost_d.data();
    L.status = ints_d.data(); L.solver_status = ints_d.data() + nb; L.is_feasible = ints_d.data() + 2 * nb; L.iterations = ints_d.data() + 3 * nb;
    L.traj_x = tx.data(); L.traj_u = tu.data(); L.traj_cost = tc.data();
    L.traj_status = ts.data(); L.traj_solver_status = tss.data(); L.traj_is_feasible = tf.data(); L.traj_iterations = ti.data();
    const int blocks = (B + engine::kLoopTile - 1) / engine::kLoopTile;
    for (int k = 0; k < ticks; ++k) {
        cmd_d = cmd[k]; cost_d = cost[k]; ints_d = ints[k];      // (assignments of equal length: the buffers stay where they are)
        hipLaunchKernelGGL(advance_with_tick<Mdl>, dim3(blocks), dim3(engine::kLoopTile), 0, nullptr, M, L, k);
    }
    printf("{");
    put("x", x); put("u", u); put("traj_x", tx); put("traj_u", tu); put("traj_cost", tc);
    put("traj_status", ts); put("traj_solver_status", tss); put("traj_is_feasible", tf); put("traj_iterations", ti, true);
    printf("}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: run_nlmpc_loop model Ts substeps B ticks noise params plant_params\n"); return 2; }
    const std::string m = argv[1];
    using namespace mpcx::models;
    if (m == "vanderpol") return run<VanDerPol>(argv);
    if (m == "ugv") return run<Ugv>(argv);
    if (m == "osc6") return run<Oscillators<6>>(argv);
    fprintf(stderr, "unknown model %s\n", m.c_str());
    return 2;
}
