// What the two solve kernels of the dense Cholesky factor share (kernels_forces_newton.hip: k_fnewton_solve;
// kernels_forces_newton_wide.hip: k_fnewton_solve_wide): a lane's value in every lane, and the diagonal tile in LDS.
#pragma once

#include "tile64.hpp"

namespace bioen {

// lane `src`'s value in every lane, src wave-uniform: two scalar lane reads, no trip through LDS as __shfl takes (the
// substitutions below are chains of these)
__device__ __forceinline__ double fnewton_lane(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// The solve's diagonal tile at j0 (nb rows) into t11, the identity beyond nb, and dinv <- 1 / its diagonal: one division
// per unknown, outside the chain.  1024 threads, four loads each; ends with a barrier.
__device__ __forceinline__ void fnewton_solve_tile(double (*t11)[kT64 + 1], double* dinv, const double* L, int ldl, int j0, int nb) {
#pragma unroll
    for (int it = 0; it < kT64 * kT64 / 1024; ++it) {
        const int e = threadIdx.x + 1024 * it;
        const int r = e / kT64, s = e % kT64;
        const double v = (r < nb && s <= r) ? L[(size_t)(j0 + r) * ldl + j0 + s] : (r == s ? 1.0 : 0.0);
        t11[r][s] = v;
        if (r == s) dinv[r] = 1.0 / v;
    }
    __syncthreads();
}

}  // namespace bioen
