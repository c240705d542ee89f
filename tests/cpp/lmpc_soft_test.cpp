// C++ front-end test of the soft-constraint weights (setSoftConstraintWeights, include/mpcx/LMPC.hpp): the three overloads, once with
// compile-time and once with run-time sizes; return values only (runs without a GPU, MPCX_DEVICE=-1).
#include <mpc/LMPC.hpp>

#include <cstdio>
#include <limits>

static int failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <class Controller, int Tnx, int Tny>
void api_case(Controller &c)
{
    const int ph = 10;
    c.setLoggerLevel(mpc::Logger::LogLevel::NONE);
    mpc::cvec<Tnx> xw(2, 1);
    mpc::cvec<Tny> yw(1, 1);
    xw(0) = mpc::inf; xw(1) = 10.0; yw(0) = 100.0;
    REQUIRE(c.setSoftConstraintWeights(xw, yw, 5.0));
    REQUIRE(c.setSoftConstraintWeights(xw, yw, mpc::inf));
    REQUIRE(c.setSoftConstraintWeights(xw, yw, 5.0, {0, ph}));
    REQUIRE(c.setSoftConstraintWeights(xw, yw, 5.0, {-1, -1}));
    REQUIRE(!c.setSoftConstraintWeights(xw, yw, 5.0, {0, ph + 1}));       // not a prediction-horizon slice
    REQUIRE(!c.setSoftConstraintWeights(xw, yw, 5.0, {3, 3}));
    REQUIRE(!c.setSoftConstraintWeights(xw, yw, 0.0));                    // zero, negative, NaN
    REQUIRE(!c.setSoftConstraintWeights(xw, yw, -1.0));
    mpc::cvec<Tnx> bad(2, 1);
    bad(0) = 1.0; bad(1) = std::numeric_limits<double>::quiet_NaN();
    REQUIRE(!c.setSoftConstraintWeights(bad, yw, 5.0));
    // the pointer form: a null pointer leaves that kind of row as it is
    const double sw = 7.0, neg = -7.0;
    REQUIRE(c.setSoftConstraintWeights(nullptr, nullptr, nullptr));
    REQUIRE(c.setSoftConstraintWeights(xw.data(), nullptr, nullptr));
    REQUIRE(c.setSoftConstraintWeights(nullptr, yw.data(), &sw, {2, 5}));
    REQUIRE(!c.setSoftConstraintWeights(nullptr, nullptr, &neg));
    REQUIRE(!c.setSoftConstraintWeights(bad.data(), nullptr, nullptr, {0, 1}));
}

int main()
{
    {
        mpc::LMPC<2, 1, 0, 1, 10, 10> c;
        api_case<decltype(c), 2, 1>(c);
    }
    {
        mpc::LMPC<> c(2, 1, 0, 1, 10, 10);
        api_case<decltype(c), -1, -1>(c);
    }
    std::printf(failures ? "%d failure(s)\n" : "all C++ soft-constraint checks passed\n", failures);
    return failures ? 1 : 0;
}
