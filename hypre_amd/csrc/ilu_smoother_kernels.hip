// hypre_amd — the conjugate-gradient acceleration around ILU as a BoomerAMG level smoother (smooth_type 15,
// par_cycle.c:300-319, 388-393, 614-636) without a host read-back.
//
// One accelerated sweep of a level visit is, behind the ILU applications that give Z from R,
//    gammaold = gamma; gamma = <R, Z>;  P = Z (first sweep) or Z + (gamma / gammaold) P;  V = A P;
//    alfa = gamma / <P, V>;  U += alfa P;  R -= alfa V
// The reference reads both inner products back to form beta and alfa on the host.  Here the two sums stay in a block of
// four doubles in device memory (gamma, gammaold, <P, V>, stop flag), the quotients are formed by the kernels that use
// them, and the exit at gamma == 0 (a zero right-hand side: the reference divides and fills U with NaN) is a flag in that
// block which turns every later kernel of the visit into a no-op.
//
// Streaming kernels: grid-stride, two doubles per lane per step (blas1_device.hpp), no LDS beyond the fold of a dot
// product.  The sums walk and fold like dot_partial_kernel / dot_final_kernel (kernels.hip), so they have the bits of
// launch_dot: a fixed tree, no floating-point atomics.  The roundings of the updates are spelled out — one fused
// multiply-add each, what axpy_kernel rounds to — and the unfused path (hypre_ParVectorAxpy, launch_ilu_cg_direction with
// beta by value) rounds the same, so both paths give the same bits.
#include "amg_internal.hpp"
#include "blas1_device.hpp"

namespace hamd {

namespace {
inline int dot_grid(size_t n)
{
   const int nb = vec_grid(n);
   return nb > DOT_BLOCKS ? DOT_BLOCKS : nb;
}
}  // namespace

// this workgroup's share of <x, y>, as dot_partial_kernel leaves it
__global__ __launch_bounds__(256)
void ilu_cg_dot_partial_kernel(const double *__restrict__ x, const double *__restrict__ y, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[4];
   double acc = 0.0;
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      const double2 yv = reinterpret_cast<const double2 *>(y)[i];
      acc += dot_pair(xv, yv);
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { acc = dot_last(x[n - 1], y[n - 1], acc); }
   acc = wave_sum(acc);
   if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = acc; }
   __syncthreads();
   if (threadIdx.x == 0) { partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]); }
}

// the fold of dot_final_kernel, the sum left in the scalar block: which == 0: gammaold = gamma, gamma = sum, and the stop
// flag raised when the sum is exactly 0; which == 1: <P, V> = sum.  A raised flag leaves the block as it is.
__global__ __launch_bounds__(256)
void ilu_cg_dot_final_kernel(const double *__restrict__ partial, int m, double *__restrict__ sc, int which)
{
   __shared__ double wsum[4];
   double acc = 0.0;
   for (int i = threadIdx.x; i < m; i += 256) { acc += partial[i]; }
   acc = wave_sum(acc);
   if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = acc; }
   __syncthreads();
   if (threadIdx.x == 0 && sc[ILU_CG_STOP] == 0.0)
   {
      const double sum = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
      if (which == 0)
      {
         sc[ILU_CG_GAMMAOLD] = sc[ILU_CG_GAMMA];
         sc[ILU_CG_GAMMA] = sum;
         if (sum == 0.0) { sc[ILU_CG_STOP] = 1.0; }
      }
      else { sc[ILU_CG_PV] = sum; }
   }
}

// P = Z + beta P, one fused multiply-add
__device__ __forceinline__ double ilu_cg_direction(double beta, double p, double z) { return __fma_rn(beta, p, z); }

// P = Z on the first sweep, else P = Z + (gamma / gammaold) P with the two sums read from the scalar block
__global__ void ilu_cg_direction_kernel(const double *__restrict__ sc, int first, const double *__restrict__ z, double *__restrict__ p, size_t n)
{
   if (sc[ILU_CG_STOP] != 0.0) { return; }
   const double beta = first ? 0.0 : __ddiv_rn(sc[ILU_CG_GAMMA], sc[ILU_CG_GAMMAOLD]);
   VEC_LOOP_BEGIN
      const double2 zv = reinterpret_cast<const double2 *>(z)[i];
      if (first) { reinterpret_cast<double2 *>(p)[i] = zv; }
      else
      {
         const double2 pv = reinterpret_cast<double2 *>(p)[i];
         reinterpret_cast<double2 *>(p)[i] = make_double2(ilu_cg_direction(beta, pv.x, zv.x), ilu_cg_direction(beta, pv.y, zv.y));
      }
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { p[n - 1] = first ? z[n - 1] : ilu_cg_direction(beta, p[n - 1], z[n - 1]); }
}

// the same update with beta handed in: the unfused path, where the host formed the quotient
__global__ void ilu_cg_direction_value_kernel(double beta, const double *__restrict__ z, double *__restrict__ p, size_t n)
{
   VEC_LOOP_BEGIN
      const double2 zv = reinterpret_cast<const double2 *>(z)[i];
      const double2 pv = reinterpret_cast<double2 *>(p)[i];
      reinterpret_cast<double2 *>(p)[i] = make_double2(ilu_cg_direction(beta, pv.x, zv.x), ilu_cg_direction(beta, pv.y, zv.y));
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { p[n - 1] = ilu_cg_direction(beta, p[n - 1], z[n - 1]); }
}

// alfa = gamma / <P, V>;  U += alfa P;  R -= alfa V, one fused multiply-add each (-alfa is exact);  Z = 0 when another
// sweep follows.  The four vectors are distinct; z may be null.
__global__ void ilu_cg_update_kernel(const double *__restrict__ sc, const double *__restrict__ p, const double *__restrict__ v,
                                     double *__restrict__ u, double *__restrict__ r, double *__restrict__ z, size_t n)
{
   if (sc[ILU_CG_STOP] != 0.0) { return; }
   const double alfa = __ddiv_rn(sc[ILU_CG_GAMMA], sc[ILU_CG_PV]), nalfa = -alfa;
   VEC_LOOP_BEGIN
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      const double2 vv = reinterpret_cast<const double2 *>(v)[i];
      const double2 uv = reinterpret_cast<double2 *>(u)[i];
      const double2 rv = reinterpret_cast<double2 *>(r)[i];
      reinterpret_cast<double2 *>(u)[i] = make_double2(__fma_rn(alfa, pv.x, uv.x), __fma_rn(alfa, pv.y, uv.y));
      reinterpret_cast<double2 *>(r)[i] = make_double2(__fma_rn(nalfa, vv.x, rv.x), __fma_rn(nalfa, vv.y, rv.y));
      if (z) { reinterpret_cast<double2 *>(z)[i] = make_double2(0.0, 0.0); }
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      u[n - 1] = __fma_rn(alfa, p[n - 1], u[n - 1]);
      r[n - 1] = __fma_rn(nalfa, v[n - 1], r[n - 1]);
      if (z) { z[n - 1] = 0.0; }
   }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
// sc[which] = <x, y> with the bits of launch_dot (which == 0 also moves gamma to gammaold and raises the stop flag at 0)
void launch_ilu_cg_dot(const double *x, const double *y, size_t n, double *sc, int which, hipStream_t s)
{
   account_bytes(16.0 * n);
   const int nb = dot_grid(n);
   double *partial = reduce_scratch(DOT_BLOCKS + 16) + 16;
   hipLaunchKernelGGL(ilu_cg_dot_partial_kernel, dim3(nb), dim3(256), 0, s, x, y, n, partial);
   HIP_CHECK(hipGetLastError());
   hipLaunchKernelGGL(ilu_cg_dot_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, sc, which);
   HIP_CHECK(hipGetLastError());
}

void launch_ilu_cg_direction(const double *sc, int first, const double *z, double *p, size_t n, hipStream_t s)
{
   account_bytes((first ? 16.0 : 24.0) * n);
   if (!n) { return; }
   hipLaunchKernelGGL(ilu_cg_direction_kernel, dim3(vec_grid(n)), dim3(256), 0, s, sc, first, z, p, n);
   HIP_CHECK(hipGetLastError());
}

void launch_ilu_cg_direction_value(double beta, const double *z, double *p, size_t n, hipStream_t s)
{
   account_bytes(24.0 * n);
   if (!n) { return; }
   hipLaunchKernelGGL(ilu_cg_direction_value_kernel, dim3(vec_grid(n)), dim3(256), 0, s, beta, z, p, n);
   HIP_CHECK(hipGetLastError());
}

void launch_ilu_cg_update(const double *sc, const double *p, const double *v, double *u, double *r, double *z, size_t n, hipStream_t s)
{
   account_bytes((z ? 56.0 : 48.0) * n);
   if (!n) { return; }
   hipLaunchKernelGGL(ilu_cg_update_kernel, dim3(vec_grid(n)), dim3(256), 0, s, sc, p, v, u, r, z, n);
   HIP_CHECK(hipGetLastError());
}

void preload_ilu_smoother_kernels() { hipFuncAttributes at; (void) hipFuncGetAttributes(&at, (const void *) ilu_cg_update_kernel); (void) hipGetLastError(); }

}  // namespace hamd
