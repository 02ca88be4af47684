// Device helpers shared by the GraphMixer kernels: graphmixer.hip (eval forward, explanation-weight backward) and
// graphmixer_train.hip (training forward / backward).
#pragma once
#include "common.h"

namespace tmk {

__host__ __device__ inline int32_t gm_r16(int32_t x) { return (x + 15) & ~15; }

// exact (erf) GELU, as nn.GELU(), and its derivative
__device__ __forceinline__ float gm_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gm_gelu_d(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

// sum over the 64 lanes of a wave
__device__ __forceinline__ float gm_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace tmk
