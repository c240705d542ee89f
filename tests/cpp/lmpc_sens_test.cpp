// C++ front-end test of mpc::LMPC<>::sensitivities() (include/mpcx/LMPC.hpp): "api" runs without a GPU (MPCX_DEVICE=-1: the call is refused
// before any solve), "solve" on one: the double integrator with an input box, once unconstrained -- the solution is affine in x0 there, so
// central differences of optimize() itself are exact up to rounding -- and once with the first move on its bound, where the gain is zero.
#include <mpc/LMPC.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>

static int failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <class Controller, int NX, int NU, int NY>
void configure(Controller &c, double box)
{
    const int ph = 10;
    const double dt = 0.1;
    c.setLoggerLevel(mpc::Logger::LogLevel::NONE);
    mpc::mat<NX, NX> A(2, 2); mpc::mat<NX, NU> B(2, 1); mpc::mat<NY, NX> C(1, 2);
    A(0, 0) = 1; A(0, 1) = dt; A(1, 0) = 0; A(1, 1) = 1; B(0, 0) = 0.5 * dt * dt; B(1, 0) = dt; C(0, 0) = 1; C(0, 1) = 0;
    REQUIRE(c.setStateSpaceModel(A, B, C));
    mpc::cvec<NY> ow(1, 1), yr(1, 1); mpc::cvec<NU> uw(1, 1), duw(1, 1), lo(1, 1), hi(1, 1), zero(1, 1);
    ow(0) = 10; uw(0) = 0.01; duw(0) = 0.1; lo(0) = -box; hi(0) = box; yr(0) = 1.0; zero(0) = 0;
    REQUIRE(c.setObjectiveWeights(ow, uw, duw, {0, ph}));
    REQUIRE(c.setInputBounds(lo, hi, {0, ph}));
    REQUIRE(c.setReferences(yr, zero, zero, {0, ph}));
}

template <class Controller, int NX, int NU, int NY>
void solve_case(Controller &c)
{
    configure<Controller, NX, NU, NY>(c, 100.0);
    mpc::cvec<NX> x0(2, 1); mpc::cvec<NU> u0(1, 1);
    x0(0) = 0.2; x0(1) = -0.1; u0(0) = 0.05;
    auto r = c.optimize(x0, u0);
    REQUIRE(r.status == mpc::ResultStatus::SUCCESS);
    auto s = c.sensitivities();
    REQUIRE(s.flag == 0);
    const double h = 1e-4;
    for (int j = 0; j < 2; ++j) {
        mpc::cvec<NX> xp = x0, xm = x0;
        xp(j) += h; xm(j) -= h;
        const double up = c.optimize(xp, u0).cmd(0), um = c.optimize(xm, u0).cmd(0);
        REQUIRE(std::fabs((up - um) / (2 * h) - s.Kx(0, j)) <= 1e-7 * (1.0 + std::fabs(s.Kx(0, j))));
    }
    {
        mpc::cvec<NU> vp = u0, vm = u0;
        vp(0) += h; vm(0) -= h;
        const double up = c.optimize(x0, vp).cmd(0), um = c.optimize(x0, vm).cmd(0);
        REQUIRE(std::fabs((up - um) / (2 * h) - s.Ku(0, 0)) <= 1e-7 * (1.0 + std::fabs(s.Ku(0, 0))));
    }
    REQUIRE(std::fabs(s.Kx(0, 0)) > 1e-3 && std::fabs(s.Ky(0, 0)) > 1e-3);
    // the first move on its bound: it does not move with anything
    configure<Controller, NX, NU, NY>(c, 0.5);
    x0(0) = -5.0;
    r = c.optimize(x0, u0);
    REQUIRE(r.status == mpc::ResultStatus::SUCCESS && std::fabs(r.cmd(0) - 0.5) <= 1e-9);
    s = c.sensitivities();
    REQUIRE(s.flag == 0 && std::fabs(s.Kx(0, 0)) <= 1e-12 && std::fabs(s.Kx(0, 1)) <= 1e-12 && std::fabs(s.Ku(0, 0)) <= 1e-12 && std::fabs(s.Ky(0, 0)) <= 1e-12);
}

template <class Controller, int NX, int NU, int NY>
void api_case(Controller &c)
{
    configure<Controller, NX, NU, NY>(c, 1.0);
    bool threw = false;
    try { (void)c.sensitivities(); } catch (const std::exception &e) { threw = std::strstr(e.what(), "sensitivities") != nullptr; }
    REQUIRE(threw);                   // nothing solved yet (and a host-only handle solves nothing)
}

int main(int argc, char **argv)
{
    const bool solve = argc > 1 && !std::strcmp(argv[1], "solve");
    {
        mpc::LMPC<2, 1, 0, 1, 10, 10> c;
        if (solve) solve_case<decltype(c), 2, 1, 1>(c); else api_case<decltype(c), 2, 1, 1>(c);
    }
    {
        mpc::LMPC<> c(2, 1, 0, 1, 10, 10);
        if (solve) solve_case<decltype(c), -1, -1, -1>(c); else api_case<decltype(c), -1, -1, -1>(c);
    }
    std::printf(failures ? "%d failure(s)\n" : "all C++ sensitivity checks passed\n", failures);
    return failures ? 1 : 0;
}
