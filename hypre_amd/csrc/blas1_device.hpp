// hypre_amd — device helpers the BLAS-1 kernel files share (kernels.hip, mass_kernels.hip): the grid-stride loop over
// pairs of doubles, the 64-lane sum and the per-pair term of a dot product.  Kernels that promise the bits of
// launch_dot (the fused PCG update, the batched dots) must walk the vector and fold the lanes exactly like
// dot_partial_kernel; these are the pieces they walk and fold with.
#pragma once
#include "internal.hpp"

namespace hamd {

__device__ __forceinline__ double wave_sum(double v)
{
   // 64-lane butterfly; __shfl_xor lowers to ds_swizzle / DPP on gfx950
#pragma unroll
   for (int off = 32; off > 0; off >>= 1) { v += __shfl_xor(v, off, 64); }
   return v;
}

// All BLAS-1 kernels are grid-stride with two doubles (16 B) per lane per step.
static inline int vec_grid(size_t n)
{
   size_t g = (n / 2 + 255) / 256;
   if (g > 2048) { g = 2048; }
   if (g < 1) { g = 1; }
   return (int) g;
}

#define VEC_LOOP_BEGIN                                                                   \
   const size_t n2 = n >> 1;                                                             \
   const size_t stride = (size_t) gridDim.x * blockDim.x;                                \
   for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
#define VEC_LOOP_END }

// workgroups of a dot product: each leaves one partial, one more workgroup folds them in a fixed order
constexpr int DOT_BLOCKS = 1024;

// What one pair of elements adds to a lane's share of <a, b>, and what the odd last element adds: the roundings are
// spelled out (one product, one fused multiply-add; one fused multiply-add), so that every kernel that accumulates a
// dot product rounds alike whatever the compiler would contract around it.
__device__ __forceinline__ double dot_pair(const double2 a, const double2 b) { return __fma_rn(a.x, b.x, __dmul_rn(a.y, b.y)); }
__device__ __forceinline__ double dot_last(double a, double b, double acc) { return __fma_rn(a, b, acc); }

}  // namespace hamd
