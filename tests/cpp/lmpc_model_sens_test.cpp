// C++ front-end test of mpc::LMPC<>::modelSensitivities() (include/mpcx/LMPC.hpp): "api" runs without a GPU (MPCX_DEVICE=-1: the call is refused
// before any solve), "solve" on one: the double integrator with an input box far away, central differences of optimize() under a moved model
// entry, every entry of A, B and C.  cmd is a rational function of high degree in a model entry (the horizon's powers of A), so the quotient's
// error is not known in advance: it is estimated without the gradient, as tests/test_lmpc_model_sens.py does, from the quotients at h = 1e-4
// and 2 h -- where truncation decides, their distance is three times the error at h -- and the bound is ten times that distance plus 1e-7
// for the rounding of two solves divided by 2 h.  At least half the entries must exceed a hundred times their bound, so that a wrong sign,
// factor or stage cannot pass.
#include <mpc/LMPC.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>

static int failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

constexpr int kPh = 10;

template <int NX, int NU, int NY>
struct Model {
    mpc::mat<NX, NX> A{2, 2};
    mpc::mat<NX, NU> B{2, 1};
    mpc::mat<NY, NX> C{1, 2};
    Model()
    {
        const double dt = 0.1;
        A(0, 0) = 1; A(0, 1) = dt; A(1, 0) = 0; A(1, 1) = 1; B(0, 0) = 0.5 * dt * dt; B(1, 0) = dt; C(0, 0) = 1; C(0, 1) = 0;
    }
};

template <class Controller, int NX, int NU, int NY, int PH>
void configure(Controller &c, const Model<NX, NU, NY> &m)
{
    c.setLoggerLevel(mpc::Logger::LogLevel::NONE);
    REQUIRE(c.setStateSpaceModel(m.A, m.B, m.C));
    mpc::mat<NY, PH> ow(1, kPh);
    mpc::mat<NU, PH> uw(1, kPh), duw(1, kPh);
    for (int i = 0; i < kPh; ++i) { ow(0, i) = 10 + 0.3 * i; uw(0, i) = 0.01 + 0.002 * i; duw(0, i) = 0.1 + 0.01 * i; }
    mpc::cvec<NY> yr(1, 1); mpc::cvec<NU> lo(1, 1), hi(1, 1), zero(1, 1);
    lo(0) = -100.0; hi(0) = 100.0; yr(0) = 1.0; zero(0) = 0;
    REQUIRE(c.setObjectiveWeights(ow, uw, duw));
    REQUIRE(c.setInputBounds(lo, hi, {0, kPh}));
    REQUIRE(c.setReferences(yr, zero, zero, {0, kPh}));
}

template <class Controller, int NX, int NU, int NY, int PH>
void solve_case(Controller &c)
{
    Model<NX, NU, NY> m;
    configure<Controller, NX, NU, NY, PH>(c, m);
    mpc::cvec<NX> x0(2, 1); mpc::cvec<NU> u0(1, 1), seed(1, 1);
    x0(0) = 0.2; x0(1) = -0.1; u0(0) = 0.05; seed(0) = 1.5;
    auto r = c.optimize(x0, u0);
    REQUIRE(r.status == mpc::ResultStatus::SUCCESS);
    const auto s = c.modelSensitivities(seed);
    REQUIRE(s.flag == 0);
    REQUIRE(s.dBd.size() == 0 && s.dDd.size() == 0);
    const double h = 1e-4;
    double largest = 0;
    int strong = 0, total = 0;
    for (int which = 0; which < 3; ++which)
        for (int e = 0; e < (which == 0 ? 4 : 2); ++e) {
            const int row = which == 0 ? e % 2 : (which == 1 ? e : 0), col = which == 0 ? e / 2 : (which == 1 ? 0 : e);
            auto cmd_at = [&](double dv) {
                Model<NX, NU, NY> m2 = m;
                (which == 0 ? m2.A(row, col) : (which == 1 ? m2.B(row, col) : m2.C(row, col))) += dv;
                REQUIRE(c.setStateSpaceModel(m2.A, m2.B, m2.C));
                return c.optimize(x0, u0).cmd(0);
            };
            const double fd = seed(0) * (cmd_at(h) - cmd_at(-h)) / (2 * h), fd2 = seed(0) * (cmd_at(2 * h) - cmd_at(-2 * h)) / (4 * h);
            const double g = which == 0 ? s.dA(row, col) : (which == 1 ? s.dB(row, col) : s.dC(row, col));
            const double bound = 1e-7 + 10.0 * std::fabs(fd - fd2);
            std::printf("%c(%d, %d): gradient %.9e, quotient %.9e, at 2 h %.9e, bound %.2e\n", "ABC"[which], row, col, g, fd, fd2, bound);
            REQUIRE(std::fabs(fd - g) <= bound);
            largest = std::fmax(largest, std::fabs(g));
            ++total;
            strong += std::fabs(g) >= 100.0 * bound;
        }
    REQUIRE(largest > 1e-4 && total == 8 && 2 * strong >= total);
    // a change of the controller: refused until the next solve
    REQUIRE(c.setStateSpaceModel(m.A, m.B, m.C));
    bool threw = false;
    try { (void)c.modelSensitivities(seed); } catch (const std::exception &e) { threw = std::strstr(e.what(), "modelSensitivities") != nullptr; }
    REQUIRE(threw);
}

template <class Controller, int NX, int NU, int NY, int PH>
void api_case(Controller &c)
{
    configure<Controller, NX, NU, NY, PH>(c, Model<NX, NU, NY>());
    mpc::cvec<NU> seed(1, 1);
    seed(0) = 1.0;
    bool threw = false;
    try { (void)c.modelSensitivities(seed); } catch (const std::exception &e) { threw = std::strstr(e.what(), "modelSensitivities") != nullptr; }
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
    std::printf(failures ? "%d failure(s)\n" : "all C++ model-sensitivity checks passed\n", failures);
    return failures ? 1 : 0;
}
