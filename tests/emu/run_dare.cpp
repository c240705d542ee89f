// TEST INFRASTRUCTURE -- runs the Riccati kernel (libmpc_amd/csrc/dare_kernels.hip, compiled unchanged: dare_launch and dare_sda) through the
// lock-step interpreter of tests/emu/hip/hip_runtime.h on the host: no GPU, nothing of libmpcx.so.
//
//   run_dare <form 0|1> <n> <m> <batch> <q_per_instance 0|1> <r_per_instance 0|1> <product 0|1|2> < numbers
//   stdin, whitespace separated, column-major per instance as mpcx_dare_batch takes them: A [batch n n], BorC [batch n m], Q [batch n n] or
//   [n n], R [batch m m] or [m m]
//   stdout: one JSON object: rc (what dare_launch returned), X, gain, flags, iterations -- each array followed by a guard of kPad elements that
//   must come back untouched.  The kernel's LDS is one array of the size of the limits and a guard: whatever lies behind the
//   6 n^2 + m^2 + 2 m n doubles of this call must come back untouched too (exit status 4).
#include <hip/hip_runtime.h>

#include <vector>

constexpr int kPad = 64, kMaxN = 32;
constexpr double kGuard = -7.25e300;
constexpr int kGuardI = -77;

// the kernel's `extern __shared__ double sm[]`: a block-scope declaration, so a member of the namespace around the kernel
namespace mpcx { namespace { alignas(64) double sm[9 * kMaxN * kMaxN + kPad]; } }

#include "../../libmpc_amd/csrc/dare_kernels.hip"

static double next_d()
{
    double v;
    if (scanf("%lf", &v) != 1) { fprintf(stderr, "input ended early\n"); exit(3); }
    return v;
}
static std::vector<double> read_d(size_t n) { std::vector<double> v(n); for (double &x : v) x = next_d(); return v; }
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
static void put(const char *name, const std::vector<int> &v, bool last)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}

int main(int argc, char **argv)
{
    if (argc < 8) { fprintf(stderr, "usage: run_dare form n m batch q_per_instance r_per_instance product\n"); return 2; }
    const int form = atoi(argv[1]), n = atoi(argv[2]), m = atoi(argv[3]), batch = atoi(argv[4]), qper = atoi(argv[5]) != 0, rper = atoi(argv[6]) != 0,
              product = atoi(argv[7]);
    if (n < 1 || m < 1 || batch < 1) { fprintf(stderr, "bad dimensions\n"); return 2; }
    const size_t nb = (size_t)batch, nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    const std::vector<double> A = read_d(nb * nn), B = read_d(nb * nm), Q = read_d(qper ? nb * nn : nn), R = read_d(rper ? nb * mm : mm);
    std::vector<double> X(nb * nn + kPad, kGuard), G(nb * nm + kPad, kGuard);
    std::vector<int> flags(nb + kPad, kGuardI), iters(nb + kPad, kGuardI);
    for (double &v : mpcx::sm) v = kGuard;
    const int rc = mpcx::dare_launch(form, n, m, batch, A.data(), B.data(), Q.data(), R.data(), qper, rper, X.data(), G.data(), flags.data(),
                                     iters.data(), product, nullptr);
    if (n <= kMaxN && m <= kMaxN)
        for (size_t i = 6 * nn + mm + 2 * nm; i < sizeof(mpcx::sm) / sizeof(double); ++i)
            if (mpcx::sm[i] != kGuard) { fprintf(stderr, "LDS behind the kernel's matrices was written (double %zu)\n", i); return 4; }
    printf("{\"rc\": %d, ", rc);
    put("X", X); put("gain", G); put("flags", flags, false); put("iterations", iters, true);
    printf("}\n");
    return 0;
}
