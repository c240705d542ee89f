// C++ front-end test of the input-rate bounds (setInputRateBounds, include/mpcx/LMPC.hpp): a double integrator with an input box and a
// slew limit, once with compile-time and once with run-time sizes.  Mode "api": return values of the matrix and slice overloads (runs
// without a GPU, MPCX_DEVICE=-1).  Mode "solve": one solve on the GPU; the first move is printed as a hexadecimal float on a line
// "cmd <value>" so that the Python suite can compare it bit for bit with its own front end's.
#include <mpc/LMPC.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

static int failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <class Controller, int Tnx, int Tnu, int Tndu, int Tny, int Tph, int Tch>
void integrator_case(Controller &c, bool solve, const char *label)
{
    const int ph = 10;
    const double dt = 0.1, rate = 0.1;
    c.setLoggerLevel(mpc::Logger::LogLevel::NONE);
    mpc::mat<Tnx, Tnx> A(2, 2);
    A(0, 0) = 1.0; A(0, 1) = dt; A(1, 1) = 1.0;
    mpc::mat<Tnx, Tnu> B(2, 1);
    B(0, 0) = 0.5 * dt * dt; B(1, 0) = dt;
    mpc::mat<Tny, Tnx> C(1, 2);
    C(0, 0) = 1.0;
    REQUIRE(c.setStateSpaceModel(A, B, C));
    mpc::mat<Tny, Tph> OW(1, ph);
    mpc::mat<Tnu, Tph> UW(1, ph), DUW(1, ph);
    OW.setConstant(10.0); UW.setConstant(0.01); DUW.setConstant(0.1);
    REQUIRE(c.setObjectiveWeights(OW, UW, DUW));
    mpc::cvec<Tnu> umin(1, 1), umax(1, 1);
    umin(0) = -1.0; umax(0) = 1.0;
    REQUIRE(c.setInputBounds(umin, umax, {0, ph}));

    // the matrix overload, then the slice overload on top of it
    mpc::mat<Tnu, Tph> dlo(1, ph), dhi(1, ph);
    dlo.setConstant(-5.0); dhi.setConstant(5.0);
    REQUIRE(c.setInputRateBounds(dlo, dhi));
    mpc::cvec<Tnu> lo(1, 1), hi(1, 1);
    lo(0) = -rate; hi(0) = rate;
    REQUIRE(c.setInputRateBounds(lo, hi, {0, ph}));
    REQUIRE(c.setInputRateBounds(lo, hi, {-1, -1}));
    REQUIRE(!c.setInputRateBounds(lo, hi, {0, ph + 1}));         // not a prediction-horizon slice
    REQUIRE(!c.setInputRateBounds(lo, hi, {3, 3}));
    REQUIRE(!c.setInputRateBounds(hi, lo, {0, 1}));              // dumin > dumax
    mpc::cvec<Tnu> bad(1, 1);
    bad(0) = std::numeric_limits<double>::quiet_NaN();
    REQUIRE(!c.setInputRateBounds(bad, hi, {0, 1}));
    dlo(0, 2) = 1.0; dhi(0, 2) = -1.0;
    REQUIRE(!c.setInputRateBounds(dlo, dhi));
    lo(0) = -mpc::inf;                                           // one-sided
    REQUIRE(c.setInputRateBounds(lo, hi, {ph - 1, ph}));

    mpc::cvec<Tny> yref(1, 1);
    yref(0) = 1.0;
    mpc::cvec<Tnu> zu(1, 1);
    REQUIRE(c.setReferences(yref, zu, zu, {0, ph}));
    mpc::LParameters params;
    params.maximum_iteration = 4000;
    c.setOptimizerParameters(params);
    if (!solve) return;

    mpc::cvec<Tnx> x0(2, 1);
    mpc::cvec<Tnu> u0(1, 1);
    u0(0) = 0.3;
    auto res = c.optimize(x0, u0);
    REQUIRE(res.status == mpc::ResultStatus::SUCCESS);
    REQUIRE(res.is_feasible);
    REQUIRE(std::fabs(res.cmd(0) - u0(0)) <= rate * (1.0 + 1e-5));
    REQUIRE(std::fabs(res.cmd(0) - u0(0)) >= rate * (1.0 - 1e-5));     // the step reference pulls harder than the slew limit allows
    std::printf("cmd %s %a\n", label, res.cmd(0));
}

int main(int argc, char **argv)
{
    const bool solve = argc > 1 && std::strcmp(argv[1], "solve") == 0;
    {
        mpc::LMPC<2, 1, 0, 1, 10, 10> c;
        integrator_case<decltype(c), 2, 1, 0, 1, 10, 10>(c, solve, "static");
    }
    {
        mpc::LMPC<> c(2, 1, 0, 1, 10, 10);
        integrator_case<decltype(c), -1, -1, -1, -1, -1, -1>(c, solve, "dynamic");
    }
    std::printf(failures ? "%d failure(s)\n" : "all C++ rate-bound checks passed\n", failures);
    return failures ? 1 : 0;
}
