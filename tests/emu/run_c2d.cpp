// TEST INFRASTRUCTURE -- runs the discretisation kernel (libmpc_amd/csrc/c2d_kernels.hip, compiled unchanged: c2d_launch and c2d_expm) through the
// lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so.
//
//   run_c2d <nx> <nu> <batch> <ts_per_instance 0|1> < numbers
//   stdin, whitespace separated: A [batch nx nx], B [batch nx nu] (column-major per instance, as mpcx_discretize_batch takes them), Ts [batch] or [1]
//   stdout: one JSON object: rc (what c2d_launch returned), Ad, Bd -- each array followed by a guard of kPad elements that must come back untouched.
//   With nu = 0 the kernel gets null B and Bd, as the C ABI allows.  The kernel's LDS is one array of 4 * 48^2 doubles and a guard: whatever lies
//   behind the 4 n^2 doubles of this call must come back untouched too (exit status 4).
#include <hip/hip_runtime.h>

#include <vector>

constexpr int kPad = 64, kMaxN = 48;
constexpr double kGuard = -7.25e300;

// the kernel's `extern __shared__ double sm[]`: a block-scope declaration, so a member of the namespace around the kernel
namespace mpcx { namespace { alignas(64) double sm[4 * kMaxN * kMaxN + kPad]; } }

#include "../../libmpc_amd/csrc/c2d_kernels.hip"

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

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: run_c2d nx nu batch ts_per_instance\n"); return 2; }
    const int nx = atoi(argv[1]), nu = atoi(argv[2]), batch = atoi(argv[3]), per = atoi(argv[4]) != 0;
    if (nx < 1 || nu < 0 || batch < 1) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const size_t nb = (size_t)batch, n = (size_t)nx + nu;
    const std::vector<double> A = read_d(nb * nx * nx), B = read_d(nb * nx * nu), Ts = read_d(per ? nb : 1);
    std::vector<double> Ad(nb * nx * nx + kPad, kGuard), Bd(nb * nx * nu + kPad, kGuard);
    for (double &v : mpcx::sm) v = kGuard;
    const int rc = mpcx::c2d_launch(nx, nu, batch, A.data(), nu ? B.data() : nullptr, Ts.data(), per ? 1 : 0, Ad.data(), nu ? Bd.data() : nullptr, nullptr);
    if (n <= (size_t)kMaxN)
        for (size_t i = 4 * n * n; i < sizeof(mpcx::sm) / sizeof(double); ++i)
            if (mpcx::sm[i] != kGuard) { fprintf(stderr, "LDS behind the kernel's four matrices was written (double %zu)\n", i); return 4; }
    printf("{\"rc\": %d, ", rc);
    put("Ad", Ad); put("Bd", Bd, true);
    printf("}\n");
    return 0;
}
