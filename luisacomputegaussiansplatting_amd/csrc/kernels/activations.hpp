// activations.hpp -- the 3DGS parameterisation's activations as ONE set of device expressions: what the optimiser step
// (train.hip) rewrites after every update is what the density control (densify.hip) and the point-cloud initialisation
// (init.hip) write for new rows, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

namespace lcgs
{

__device__ __forceinline__ float act_exp(float x) { return expf(x); }
__device__ __forceinline__ float act_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float4 act_unit(const float4& x)
{
    const float n2 = 1.0f / sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
    return make_float4(x.x * n2, x.y * n2, x.z * n2, x.w * n2);
}

} // namespace lcgs
