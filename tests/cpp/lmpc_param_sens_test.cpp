// C++ front-end test of mpc::LMPC<>::parameterSensitivities() (include/mpcx/LMPC.hpp): "api" runs without a GPU (MPCX_DEVICE=-1: the call is
// refused before any solve), "solve" on one: the double integrator with an input box, once unconstrained -- central differences of optimize()
// under a changed weight matrix (h = 1e-4: error h^2 times a third derivative of order one, bound 1e-6) -- and once with the first move on its
// bound, where cmd moves with that bound alone.
#include <mpc/LMPC.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>

static int failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

constexpr int kPh = 10;

template <int NY, int NU, int PH>
struct Weights {
    mpc::mat<NY, PH> ow{1, kPh};
    mpc::mat<NU, PH> uw{1, kPh}, duw{1, kPh};
    Weights() { for (int i = 0; i < kPh; ++i) { ow(0, i) = 10 + 0.3 * i; uw(0, i) = 0.01 + 0.002 * i; duw(0, i) = 0.1 + 0.01 * i; } }
};

template <class Controller, int NX, int NU, int NY, int PH>
void configure(Controller &c, double box, const Weights<NY, NU, PH> &w)
{
    const double dt = 0.1;
    c.setLoggerLevel(mpc::Logger::LogLevel::NONE);
    mpc::mat<NX, NX> A(2, 2); mpc::mat<NX, NU> B(2, 1); mpc::mat<NY, NX> C(1, 2);
    A(0, 0) = 1; A(0, 1) = dt; A(1, 0) = 0; A(1, 1) = 1; B(0, 0) = 0.5 * dt * dt; B(1, 0) = dt; C(0, 0) = 1; C(0, 1) = 0;
    REQUIRE(c.setStateSpaceModel(A, B, C));
    mpc::cvec<NY> yr(1, 1); mpc::cvec<NU> lo(1, 1), hi(1, 1), zero(1, 1);
    lo(0) = -box; hi(0) = box; yr(0) = 1.0; zero(0) = 0;
    REQUIRE(c.setObjectiveWeights(w.ow, w.uw, w.duw));
    REQUIRE(c.setInputBounds(lo, hi, {0, kPh}));
    REQUIRE(c.setReferences(yr, zero, zero, {0, kPh}));
}

template <class Controller, int NX, int NU, int NY, int PH>
void solve_case(Controller &c)
{
    Weights<NY, NU, PH> w;
    configure<Controller, NX, NU, NY, PH>(c, 100.0, w);
    mpc::cvec<NX> x0(2, 1); mpc::cvec<NU> u0(1, 1), seed(1, 1);
    x0(0) = 0.2; x0(1) = -0.1; u0(0) = 0.05; seed(0) = 1.5;
    auto r = c.optimize(x0, u0);
    REQUIRE(r.status == mpc::ResultStatus::SUCCESS);
    const auto s = c.parameterSensitivities(seed);
    REQUIRE(s.flag == 0);
    for (double v : s.dLower) REQUIRE(v == 0.0);
    for (double v : s.dUpper) REQUIRE(v == 0.0);
    const double h = 1e-4;
    double largest = 0;
    for (int which = 0; which < 3; ++which)
        for (int i : {0, 3, kPh - 1}) {
            auto cmd_at = [&](double dv) {
                Weights<NY, NU, PH> w2 = w;
                (which == 0 ? w2.ow(0, i) : (which == 1 ? w2.uw(0, i) : w2.duw(0, i))) += dv;
                REQUIRE(c.setObjectiveWeights(w2.ow, w2.uw, w2.duw));
                return c.optimize(x0, u0).cmd(0);
            };
            const double fd = seed(0) * (cmd_at(h) - cmd_at(-h)) / (2 * h);
            const double g = which == 0 ? s.dOWeight(0, i) : (which == 1 ? s.dUWeight(0, i) : s.dDeltaUWeight(0, i));
            REQUIRE(std::fabs(fd - g) <= 1e-6 * (1.0 + std::fabs(g)));
            largest = std::fmax(largest, std::fabs(g));
        }
    REQUIRE(largest > 1e-4);
    // the first move on its upper bound: cmd = hi, so it moves with that bound alone
    configure<Controller, NX, NU, NY, PH>(c, 0.5, w);
    x0(0) = -5.0;
    r = c.optimize(x0, u0);
    REQUIRE(r.status == mpc::ResultStatus::SUCCESS && std::fabs(r.cmd(0) - 0.5) <= 1e-9);
    const auto t = c.parameterSensitivities(seed);
    REQUIRE(t.flag == 0);
    for (int i = 0; i < kPh; ++i) REQUIRE(std::fabs(t.dOWeight(0, i)) <= 1e-12 && std::fabs(t.dUWeight(0, i)) <= 1e-12 && std::fabs(t.dDeltaUWeight(0, i)) <= 1e-12);
    const size_t row = (size_t)(kPh + 1) * 3 + 3 + 2;          // the input row of step 1 behind the equality rows: neq + na + nx
    REQUIRE(t.dUpper.size() > row && std::fabs(t.dUpper[row] - seed(0)) <= 1e-12);
    for (double v : t.dLower) REQUIRE(v == 0.0);
    // a change of the controller: refused until the next solve
    REQUIRE(c.setObjectiveWeights(w.ow, w.uw, w.duw));
    bool threw = false;
    try { (void)c.parameterSensitivities(seed); } catch (const std::exception &e) { threw = std::strstr(e.what(), "parameterSensitivities") != nullptr; }
    REQUIRE(threw);
}

template <class Controller, int NX, int NU, int NY, int PH>
void api_case(Controller &c)
{
    configure<Controller, NX, NU, NY, PH>(c, 1.0, Weights<NY, NU, PH>());
    mpc::cvec<NU> seed(1, 1);
    seed(0) = 1.0;
    bool threw = false;
    try { (void)c.parameterSensitivities(seed); } catch (const std::exception &e) { threw = std::strstr(e.what(), "parameterSensitivities") != nullptr; }
    REQUIRE(threw);                   // nothing solved yet (and a host-only handle solves nothing)
}

int main(int argc, char **argv)
{
    const bool solve = argc > 1 && !std::strcmp(argv[1], "solve");
    {
        mpc::LMPC<2, 1, 0, 1, kPh, kPh> c;
        if (solve) solve_case<decltype(c), 2, 1, 1, kPh>(c); else api_case<decltype(c), 2, 1, 1, kPh>(c);
    }
    {
        mpc::LMPC<> c(2, 1, 0, 1, kPh, kPh);
        if (solve) solve_case<decltype(c), -1, -1, -1, -1>(c); else api_case<decltype(c), -1, -1, -1, -1>(c);
    }
    std::printf(failures ? "%d failure(s)\n" : "all C++ parameter-sensitivity checks passed\n", failures);
    return failures ? 1 : 0;
}
