// What the two kernels that differentiate a bank's solved batch (lmpc_bank_sens.hip, lmpc_bank_grad.hip) have in common beyond
// lmpc_sens_common.hpp: the roll-out of a direction through the instance's own model in LDS.  A bank has no operand that its instances share, so
// the products of the single-controller kernels with Cq and Xq are this chain.
#pragma once
#include "lmpc_sens_common.hpp"

namespace mpcx {

namespace {

__host__ __device__ inline int bank_even(int n) { return (n + 1) & ~1; }

// the direction's roll-out through the instance's own model (As, Bs, Cs column-major and blk in LDS): dx [(ph + 1) x nx] by the chain of ph steps,
// then the outputs of every step at once, do[(i - 1) ny + j] = Wy_i (C dx_i)[j] for i = 1 .. ph
__device__ inline void bank_rollout(const double *As, const double *Bs, const double *Cs, gdp Wy, const int *blk, const double *q, int nx, int nu, int ny,
                                    int ph, int lane, double *dx, double *dov)
{
    for (int a = lane; a < nx; a += 64) dx[a] = 0.0;
    wave_sync();
    for (int i = 1; i <= ph; ++i) {
        const double *dv = q + blk[i] * nu, *xp = dx + (size_t)(i - 1) * nx;
        for (int a = lane; a < nx; a += 64) {
            double s = 0.0;
#pragma unroll 4
            for (int c = 0; c < nx; ++c) s = fma(As[a + (size_t)c * nx], xp[c], s);
#pragma unroll 4
            for (int j = 0; j < nu; ++j) s = fma(Bs[a + (size_t)j * nx], dv[j], s);
            dx[(size_t)i * nx + a] = s;
        }
        wave_sync();
    }
    for (int t = lane; t < ph * ny; t += 64) {
        const int i = t / ny + 1, j = t - (i - 1) * ny;
        const double *xi = dx + (size_t)i * nx;
        double s = 0.0;
#pragma unroll 4
        for (int c = 0; c < nx; ++c) s = fma(Cs[j + (size_t)c * ny], xi[c], s);
        dov[t] = Wy[j + (size_t)i * ny] * s;
    }
    wave_sync();
}

}  // namespace

}  // namespace mpcx
