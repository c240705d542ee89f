// The closed loop around the batched NLMPC solve (mpcx_nlmpc_loop_*, include/mpcx.h): what runs between two solves of a receding-horizon
// run -- the caller's loop of the reference examples (examples/vanderpol_ex.cpp:76-85, ugv_ex.cpp) -- on the device, so that a tick is
// "solve, advance" with no host work in between.
//
//   loop_plant_reg<Mdl>     the noise-free step from registers to registers (shared with mpcx/nlmpc_ekf.hpp)
//   loop_plant_lane<Mdl>    the plant step of one instance in registers: x <- f(x, cmd, p) for a discrete model, `substeps` forward-Euler
//                           steps x <- x + (Ts / substeps) f(x, cmd, p) for a continuous one, then x += w
//   loop_advance_tile<Mdl>  tick k of a tile of 64 instances, lane <-> instance: the plant step, u <- cmd, row k + 1 of traj_x, row k of
//                           traj_u and of the per-instance logs
//   loop_plant_tile<Mdl>    the same plant step without a loop around it (mpcx_nlmpc_plant_step_batch)
//
// The bodies take the tick as an argument and use no atomics and no fences: where the tick comes from (a counter in device memory, moved on
// by the last block) is the business of the __global__ wrappers in libmpc_amd/csrc/nlmpc_loop.hip, and the bodies run unchanged in the
// lock-step interpreter of tests/emu.  They are templates over the model type and go through engine::call_f / engine::is_ct, so that an
// instantiation for hook models needs no change here.  NX and NU are compile-time constants: a lane's x, u and dx are register arrays
// (every subscript a constant after unrolling), there is no scratch and no LDS; a lane reads and writes its own instance's rows, NX and
// NU contiguous doubles.  The Mapping scalings play no part: states and commands are in physical units on both sides of a solve.
#pragma once

#include "nlmpc_engine.hpp"

namespace mpcx {

struct NlmpcLoopDev {
    int batch, ticks, substeps;
    int nparams;                            // row length of params / plant_params
    const double *x0, *u0;                  // the caller's [B x nx], [B x nu]: read by the begin kernel of every run
    const double *params, *plant_params;    // [B x nparams] or null
    const double *noise;                    // [ticks x B x nx] or null
    double *x, *u;                          // the loop's state and last command: the solve's x0 and u0
    const double *cmd, *cost;               // the solve's results ...
    const int *status, *solver_status, *is_feasible, *iterations;
    double *traj_x, *traj_u, *traj_cost;    // ... and where the tick's rows of them go (tick-major; the logs may be null)
    int *traj_status, *traj_solver_status, *traj_is_feasible, *traj_iterations;
    int *state;                             // [tick, blocks through]
};

namespace engine {

constexpr int kLoopTile = 64;               // instances per block = lanes of its one wavefront

template <class T> __device__ __forceinline__ const T __attribute__((address_space(1))) *loop_gin(const T *p)
{
    return (const T __attribute__((address_space(1))) *)p;
}
template <class T> __device__ __forceinline__ T __attribute__((address_space(1))) *loop_gout(T *p)
{
    return (T __attribute__((address_space(1))) *)p;
}

// x [NX] <- the noise-free step of the plant from x, with the command u [NU], both in registers: f for a discrete model, `substeps`
// forward-Euler steps for a continuous one (the Euler update is spelled as the fused multiply-add the compiler would make of it, so
// that no instantiation rounds differently from another).  Shared by the lane <-> instance kernels below and by the extended Kalman
// filter of mpcx/nlmpc_ekf.hpp, whose lanes each evaluate it at a point of their own
template <class Mdl>
__device__ __forceinline__ void loop_plant_reg(const NlmpcDev &M, const double *p, const int substeps, double (&x)[Mdl::NX], const double (&u)[Mdl::NU])
{
    constexpr int NX = Mdl::NX;
    double dx[NX];
    if (is_ct<Mdl>(M)) {
        const double h = M.Ts / (double)substeps;
        for (int s = 0; s < substeps; ++s) {
            call_f<Mdl>(dx, x, u, p, 0);
#pragma unroll
            for (int j = 0; j < NX; ++j) x[j] = fma(h, dx[j], x[j]);
        }
    } else {
        call_f<Mdl>(dx, x, u, p, 0);
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = dx[j];
    }
}

// x [NX] <- the plant's next state from xin [NX], u [NU] <- uin [NU]; w: the instance's process disturbance [NX] or null.  One function
// for the loop and for the stand-alone step: the two agree bit for bit
template <class Mdl>
__device__ __forceinline__ void loop_plant_lane(const NlmpcDev &M, const double *xin, const double *uin, const double *p, const double *w,
                                                const int substeps, double (&x)[Mdl::NX], double (&u)[Mdl::NU])
{
    constexpr int NX = Mdl::NX, NU = Mdl::NU;
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = loop_gin(xin)[j];
#pragma unroll
    for (int j = 0; j < NU; ++j) u[j] = loop_gin(uin)[j];
    loop_plant_reg<Mdl>(M, p, substeps, x, u);
    if (w) {
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] += loop_gin(w)[j];
    }
}

// tick k of the block's tile: the caller has made sure that k < L.ticks
template <class Mdl>
__device__ __forceinline__ void loop_advance_tile(const NlmpcDev &M, const NlmpcLoopDev &L, const int k)
{
    constexpr int NX = Mdl::NX, NU = Mdl::NU;
    const int b = (int)blockIdx.x * kLoopTile + (int)threadIdx.x;
    if (b >= L.batch) return;
    const size_t B = (size_t)L.batch, at = (size_t)k * B + b;
    const double *p = L.plant_params ? L.plant_params + (size_t)b * L.nparams : L.params ? L.params + (size_t)b * L.nparams : M.params;
    double x[NX], u[NU];
    loop_plant_lane<Mdl>(M, L.x + (size_t)b * NX, L.cmd + (size_t)b * NU, p, L.noise ? L.noise + at * NX : nullptr, L.substeps, x, u);
    double __attribute__((address_space(1))) *xo = loop_gout(L.x) + (size_t)b * NX, *tx = loop_gout(L.traj_x) + (at + B) * NX;
    double __attribute__((address_space(1))) *uo = loop_gout(L.u) + (size_t)b * NU, *tu = loop_gout(L.traj_u) + at * NU;
#pragma unroll
    for (int j = 0; j < NX; ++j) { xo[j] = x[j]; tx[j] = x[j]; }
#pragma unroll
    for (int j = 0; j < NU; ++j) { uo[j] = u[j]; tu[j] = u[j]; }      // lastU of the next tick: the command as it is
    if (L.traj_cost) loop_gout(L.traj_cost)[at] = loop_gin(L.cost)[b];
    if (L.traj_status) loop_gout(L.traj_status)[at] = loop_gin(L.status)[b];
    if (L.traj_solver_status) loop_gout(L.traj_solver_status)[at] = loop_gin(L.solver_status)[b];
    if (L.traj_is_feasible) loop_gout(L.traj_is_feasible)[at] = loop_gin(L.is_feasible)[b];
    if (L.traj_iterations) loop_gout(L.traj_iterations)[at] = loop_gin(L.iterations)[b];
}

// x_next <- plant(x, u) for the block's tile (x_next may be x: a lane has read its row before it writes it)
template <class Mdl>
__device__ __forceinline__ void loop_plant_tile(const NlmpcDev &M, const int batch, const double *xin, const double *uin, const double *params,
                                                const int nparams, const double *noise, const int substeps, double *x_next)
{
    constexpr int NX = Mdl::NX, NU = Mdl::NU;
    const int b = (int)blockIdx.x * kLoopTile + (int)threadIdx.x;
    if (b >= batch) return;
    const double *p = params ? params + (size_t)b * nparams : M.params;
    double x[NX], u[NU];
    loop_plant_lane<Mdl>(M, xin + (size_t)b * NX, uin + (size_t)b * NU, p, noise ? noise + (size_t)b * NX : nullptr, substeps, x, u);
    double __attribute__((address_space(1))) *xo = loop_gout(x_next) + (size_t)b * NX;
#pragma unroll
    for (int j = 0; j < NX; ++j) xo[j] = x[j];
}

}  // namespace engine
}  // namespace mpcx
