// The ReLU of every kernel in this library, with torch.relu's handling of NaN: fmaxf(v, 0) and `v > 0` both treat a NaN as "not
// positive" and turn it into a finite 0 (and its gradient into 0), after which no later check -- the optimizer's non-finite guard
// included -- can see that the activation was broken.  torch.relu(NaN) = NaN, threshold_backward passes the gradient at a NaN
// output, and max_pool2d returns NaN for a window holding one.  For every other input, +-Inf included, these return bit for bit
// what fmaxf / `v > 0` returned.
#pragma once
#include <hip/hip_runtime.h>

namespace mono {

// v for v > 0 and for NaN, +0 otherwise
__device__ __forceinline__ float relu_f(float v) { return v <= 0.f ? 0.f : v; }
// the ReLU's mask bit / gradient switch: 1 where relu_f passes v through (v > 0 or NaN)
__device__ __forceinline__ int relu_on(float v) { return !(v <= 0.f); }
// running maximum of a pooling window (at::native max_pool2d: `val > max || isnan(val)`)
__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

}  // namespace mono
