// TEST INFRASTRUCTURE -- runs the target-map kernel and the target product (libmpc_amd/csrc/target_kernels.hip, compiled unchanged: target_map_launch,
// target_map, target_apply_launch, target_apply) through the lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of
// libmpcx.so.
//
//   run_target map <nx> <nu> <ndu> <ny> <batch> <want_x 0|1> <want_flags 0|1> <lds_limit bytes> < numbers
//     stdin, whitespace separated, column-major per instance as mpcx_target_map_batch takes them: A [batch nx nx], B [batch nx nu], Bd [batch nx ndu],
//     C [batch ny nx], Dd [batch ny ndu]
//     stdout: one JSON object: rc (what target_map_launch returned), map_u, map_x, flags
//   run_target apply <nu> <ndu> <ny> <batch> <map_per_instance 0|1> < numbers
//     stdin: map_u [batch nu nrhs] or [nu nrhs], r [batch ny], dhat [batch ndu], ubar [batch nu];  stdout: rc, us
// Each output array is followed by a guard of kPad elements that must come back untouched (the test checks them).  The kernel's LDS is one array of
// the size of the limit and a guard: whatever lies behind the nk (nk + nrhs) doubles of this call must come back untouched too (exit status 4).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

constexpr int kPad = 64, kLdsDoubles = 160 * 1024 / 8;
constexpr double kGuard = -7.25e300;
constexpr int kGuardI = -77;

// the kernel's `extern __shared__ double sm[]`: a block-scope declaration, so a member of the namespace around the kernel
namespace mpcx { namespace { alignas(64) double sm[kLdsDoubles + kPad]; } }

#include "../../libmpc_amd/csrc/target_kernels.hip"

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
    for (size_t i = 0; i < v.size(); ++i) {
        if (std::isnan(v[i])) printf("%sNaN", i ? ", " : "");
        else if (std::isinf(v[i])) printf("%s%sInfinity", i ? ", " : "", v[i] < 0 ? "-" : "");
        else printf("%s%.17g", i ? ", " : "", v[i]);
    }
    printf("]%s", last ? "" : ", ");
}
static void put(const char *name, const std::vector<int> &v, bool last)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}

int main(int argc, char **argv)
{
    if (argc >= 7 && !strcmp(argv[1], "apply")) {
        const int nu = atoi(argv[2]), ndu = atoi(argv[3]), ny = atoi(argv[4]), batch = atoi(argv[5]), per = atoi(argv[6]) != 0;
        if (nu < 1 || ndu < 0 || ny < 1 || batch < 1) { fprintf(stderr, "bad dimensions\n"); return 2; }
        const size_t nb = (size_t)batch, len = (size_t)nu * (ny + ndu + nu);
        const std::vector<double> T = read_d(per ? nb * len : len), r = read_d(nb * ny), d = read_d(nb * ndu), ub = read_d(nb * nu);
        std::vector<double> us(nb * nu + kPad, kGuard);
        const int rc = mpcx::target_apply_launch(nu, ndu, ny, batch, T.data(), per, r.data(), d.data(), ub.data(), us.data(), nullptr);
        printf("{\"rc\": %d, ", rc);
        put("us", us, true);
        printf("}\n");
        return 0;
    }
    if (argc < 10 || strcmp(argv[1], "map")) { fprintf(stderr, "usage: run_target map nx nu ndu ny batch want_x want_flags lds_limit | run_target apply nu ndu ny batch map_per_instance\n"); return 2; }
    const int nx = atoi(argv[2]), nu = atoi(argv[3]), ndu = atoi(argv[4]), ny = atoi(argv[5]), batch = atoi(argv[6]), want_x = atoi(argv[7]) != 0,
              want_flags = atoi(argv[8]) != 0;
    const size_t limit = (size_t)atoll(argv[9]);
    if (nx < 1 || nu < 1 || ndu < 0 || ny < 1 || batch < 1 || limit > (size_t)kLdsDoubles * 8) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const size_t nb = (size_t)batch, nrhs = (size_t)ny + ndu + nu, nk = (size_t)2 * nx + nu + ny;
    const std::vector<double> A = read_d(nb * nx * nx), B = read_d(nb * nx * nu), Bd = read_d(nb * nx * ndu), C = read_d(nb * ny * nx),
                              Dd = read_d(nb * ny * ndu);
    std::vector<double> Tu(nb * nu * nrhs + kPad, kGuard), Tx(nb * nx * nrhs + kPad, kGuard);
    std::vector<int> flags(nb + kPad, kGuardI);
    for (double &v : mpcx::sm) v = kGuard;
    const int rc = mpcx::target_map_launch(nx, nu, ndu, ny, batch, A.data(), B.data(), Bd.data(), C.data(), Dd.data(), Tu.data(),
                                           want_x ? Tx.data() : nullptr, want_flags ? flags.data() : nullptr, limit, nullptr);
    for (size_t i = rc == 0 ? nk * (nk + nrhs) : 0; i < sizeof(mpcx::sm) / sizeof(double); ++i)
        if (mpcx::sm[i] != kGuard) { fprintf(stderr, "LDS behind the kernel's matrix was written (double %zu)\n", i); return 4; }
    printf("{\"rc\": %d, ", rc);
    put("map_u", Tu); put("map_x", Tx); put("flags", flags, true);
    printf("}\n");
    return 0;
}
