// One row of a steady-state target: us_i = sum_j T(i, j) [r; dhat; ubar]_j with T(i, j) = T[j * stride].  The one definition of the sum -- from 0,
// by fma, by ascending column: Tr, then Td, then Tu -- that the loop's kernels (lmpc_loop.hip) and the stand-alone product
// (mpcx_target_apply_batch, target_kernels.hip) share, so that the two agree bit for bit.  The pointers are of whatever address space the caller has.
#pragma once

#include <cstddef>

namespace mpcx {

template <typename TP, typename RP, typename DP, typename UP>
__device__ __forceinline__ double target_us_row(TP T, const size_t stride, RP r, const int ny, DP d, const int ndu, UP ub, const int nu)
{
    double acc = 0.0;
    for (int j = 0; j < ny; ++j) acc = fma(T[j * stride], r[j], acc);
    T += (size_t)ny * stride;
    for (int j = 0; j < ndu; ++j) acc = fma(T[j * stride], d[j], acc);
    T += (size_t)ndu * stride;
    for (int j = 0; j < nu; ++j) acc = fma(T[j * stride], ub[j], acc);
    return acc;
}

}  // namespace mpcx
