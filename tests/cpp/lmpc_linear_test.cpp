// C++ front-end test of the linear rows (setLinearConstraints, include/mpcx/LMPC.hpp): a double integrator with an input box and the coupled row
// |x_2 + 0.5 v| <= 0.25 from step 1 on, once with compile-time and once with run-time sizes.  Mode "api": return values of the whole-horizon and
// slice forms and of the weights (runs without a GPU, MPCX_DEVICE=-1).  Mode "solve": one solve on the GPU; the first move is printed as a
// hexadecimal float on a line "cmd <label> <value>" so that the Python suite can compare it bit for bit with its own front end's.
#include <mpc/LMPC.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <class Controller, int Tnx, int Tnu, int Tndu, int Tny, int Tph, int Tch>
void integrator_case(Controller &c, bool solve, const char *label)
{
    const int ph = 10;
    const double dt = 0.1, lim = 0.25, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
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

    // two rows over the whole horizon, then one row through the slice form: nc may change only while no other step holds a bound
    const double Fx2[4] = {0.0, 1.0, 1.0, 0.0}, Fu2[2] = {0.5, 0.0};       // column-major [2 x 2], [2 x 1]: rows (0, 1 | 0.5) and (1, 0 | 0)
    std::vector<double> lo2(2 * (ph + 1), -5.0), hi2(2 * (ph + 1), 5.0);
    REQUIRE(c.setLinearConstraints(2, Fx2, Fu2, lo2.data(), hi2.data()));
    const double Fx[2] = {0.0, 1.0}, Fu[1] = {0.5}, lo[1] = {-lim}, hi[1] = {lim};
    REQUIRE(!c.setLinearConstraints(1, Fx, Fu, lo, hi, {1, ph}));            // step 0 and 1 still hold bounds of two rows
    REQUIRE(c.setLinearConstraints(0, nullptr, nullptr, nullptr, nullptr)); // the rows taken back
    REQUIRE(c.setLinearConstraints(1, Fx, Fu, lo, hi, {1, ph}));             // steps 2 .. ph
    REQUIRE(c.setLinearConstraints(1, Fx, Fu, lo, hi, {-1, -1}));
    REQUIRE(!c.setLinearConstraints(1, Fx, Fu, lo, hi, {0, ph + 1}));        // not a prediction-horizon slice
    REQUIRE(!c.setLinearConstraints(1, Fx, Fu, hi, lo, {0, 1}));             // lo > hi
    const double bad[1] = {nan}, big[1] = {inf};
    REQUIRE(!c.setLinearConstraints(1, Fx, Fu, bad, hi, {0, 1}));
    REQUIRE(!c.setLinearConstraints(1, Fx, big, lo, hi, {0, 1}));            // an infinite coefficient
    REQUIRE(!c.setLinearConstraints(MPCX_MAX_LINEAR_ROWS + 1, Fx, Fu, lo, hi));
    const double w[1] = {50.0}, hard[1] = {inf}, zero[1] = {0.0};
    REQUIRE(c.setLinearConstraintWeights(w));
    REQUIRE(!c.setLinearConstraintWeights(zero));
    REQUIRE(c.setLinearConstraintWeights(hard, {0, ph}));
    // the case of the solve: the row from step 1 on (step 0 free: lastU = 0.3 and a velocity are data)
    std::vector<double> L(ph + 1, -lim), H(ph + 1, lim);
    L[0] = -inf; H[0] = inf;
    REQUIRE(c.setLinearConstraints(1, Fx, Fu, L.data(), H.data()));

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
    // the row of step 1 reads the velocity dt cmd of x_1 and v_1 = cmd: (dt + 0.5) |cmd| <= lim, and the step reference pulls harder than that
    REQUIRE(std::fabs(res.cmd(0)) * (dt + 0.5) <= lim * (1.0 + 1e-5));
    REQUIRE(std::fabs(res.cmd(0)) * (dt + 0.5) >= lim * (1.0 - 1e-5));
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
    std::printf(failures ? "%d failure(s)\n" : "all C++ linear-row checks passed\n", failures);
    return failures ? 1 : 0;
}
