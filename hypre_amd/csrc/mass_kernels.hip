// hypre_amd — batched vector kernels for gfx950 (CDNA4): many dot products against one vector, and one vector updated
// with many, in one pass over HBM each.  They are what the classical Gram-Schmidt of COGMRES (par_gmres.cpp) is built
// on: step i of a restart cycle needs <p_i, p_j> for all j < i and p_i -= sum_j h_j p_j, which as separate dots and
// axpys is 5 i vector passes and i read-backs; batched it is 2 i + 2 passes and one read-back.
//
// Beside them the fused vector passes of the other Krylov callers: the Gram-Schmidt step of FlexGMRES, the end of an
// LGMRES cycle, the two-sum passes and the direction update of BiCGSTAB (par_bicgstab.cpp), and the step of diagonally
// scaled CG: update, scaling and both sums in one pass over a packed diagonal (par_pcg.cpp).
//
// Replaces (behaviourally) the host loops of
//   seq_mv/vector_batched.c   hypre_SeqVectorMassInnerProd / MassDotpTwo / MassAxpy (and their 4- and 8-fold unrollings)
//
// Pure streaming work: 16-byte loads, K + 1 (K + 2) loads in flight per lane, no LDS beyond the wave-sum slots.  The
// vectors' addresses and the coefficients travel by value in the kernel arguments, and K is a template parameter with
// fully unrolled loops, so the accumulators stay in registers.  Every result has the bits the one-at-a-time kernels of
// kernels.hip give: same grid, same walk, same per-pair term, same fold.

#include "amg_internal.hpp"
#include "blas1_device.hpp"

namespace hamd {

template <int K> struct MassVectors { const double *p[K]; };
template <int K> struct MassCoefficients { double a[K]; };

// a workgroup's partial of accumulator j, folded like dot_partial_kernel folds its one
#define MASS_FOLD(acc, wsum, J)                                                          \
   _Pragma("unroll")                                                                     \
   for (int j = 0; j < (J); j++)                                                         \
   {                                                                                     \
      const double v = wave_sum(acc[j]);                                                 \
      if ((threadIdx.x & 63) == 0) { wsum[j][threadIdx.x >> 6] = v; }                    \
   }                                                                                     \
   __syncthreads();                                                                      \
   if (threadIdx.x < (J))                                                                \
   {                                                                                     \
      const int j = threadIdx.x;                                                         \
      partial[(size_t) j * DOT_BLOCKS + blockIdx.x] = (wsum[j][0] + wsum[j][1]) + (wsum[j][2] + wsum[j][3]); \
   }

// partial[j * DOT_BLOCKS + block] = this workgroup's share of <x, y_j>, j < K
template <int K>
__global__ __launch_bounds__(256)
void mass_dot_kernel(const double *__restrict__ x, const MassVectors<K> y, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[K][4];
   double acc[K];
#pragma unroll
   for (int j = 0; j < K; j++) { acc[j] = 0.0; }
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      double2 yv[K];
#pragma unroll
      for (int j = 0; j < K; j++) { yv[j] = reinterpret_cast<const double2 *>(y.p[j])[i]; }
#pragma unroll
      for (int j = 0; j < K; j++) { acc[j] += dot_pair(xv, yv[j]); }
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
#pragma unroll
      for (int j = 0; j < K; j++) { acc[j] = dot_last(x[n - 1], y.p[j][n - 1], acc[j]); }
   }
   MASS_FOLD(acc, wsum, K)
}

// the same for two vectors at once: accumulators j < K hold <x, z_j>, accumulators K + j hold <y, z_j>
template <int K>
__global__ __launch_bounds__(256)
void mass_dot_two_kernel(const double *__restrict__ x, const double *__restrict__ y, const MassVectors<K> z, size_t n,
                         double *__restrict__ partial)
{
   __shared__ double wsum[2 * K][4];
   double acc[2 * K];
#pragma unroll
   for (int j = 0; j < 2 * K; j++) { acc[j] = 0.0; }
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      const double2 yv = reinterpret_cast<const double2 *>(y)[i];
      double2 zv[K];
#pragma unroll
      for (int j = 0; j < K; j++) { zv[j] = reinterpret_cast<const double2 *>(z.p[j])[i]; }
#pragma unroll
      for (int j = 0; j < K; j++)
      {
         acc[j] += dot_pair(xv, zv[j]);
         acc[K + j] += dot_pair(yv, zv[j]);
      }
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
#pragma unroll
      for (int j = 0; j < K; j++)
      {
         acc[j] = dot_last(x[n - 1], z.p[j][n - 1], acc[j]);
         acc[K + j] = dot_last(y[n - 1], z.p[j][n - 1], acc[K + j]);
      }
   }
   MASS_FOLD(acc, wsum, 2 * K)
}

// workgroup b folds the m partials of accumulator b exactly as dot_final_kernel folds those of one dot product; the
// first `split` accumulators land in out_a, the others in out_b
__global__ __launch_bounds__(256)
void mass_dot_final_kernel(const double *__restrict__ partial, int m, int split, double *__restrict__ out_a, double *__restrict__ out_b)
{
   __shared__ double wsum[4];
   const int b = blockIdx.x;
   partial += (size_t) b * DOT_BLOCKS;
   double acc = 0.0;
   for (int i = threadIdx.x; i < m; i += 256) { acc += partial[i]; }
   acc = wave_sum(acc);
   if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = acc; }
   __syncthreads();
   if (threadIdx.x == 0)
   {
      const double r = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
      if (b < split) { out_a[b] = r; } else { out_b[b - split] = r; }
   }
}

// y += a_0 x_0, then += a_1 x_1, ... in that order, each step rounded like axpy_kernel rounds its one (a fused
// multiply-add); y is read and written once.  No restrict: an x_j may be y, as for axpy_kernel.
template <int K>
__global__ void mass_axpy_kernel(const MassCoefficients<K> alpha, const MassVectors<K> x, double *y, size_t n)
{
   VEC_LOOP_BEGIN
      double2 t = reinterpret_cast<double2 *>(y)[i];
      double2 xv[K];
#pragma unroll
      for (int j = 0; j < K; j++) { xv[j] = reinterpret_cast<const double2 *>(x.p[j])[i]; }
#pragma unroll
      for (int j = 0; j < K; j++)
      {
         t.x = __fma_rn(alpha.a[j], xv[j].x, t.x);
         t.y = __fma_rn(alpha.a[j], xv[j].y, t.y);
      }
      reinterpret_cast<double2 *>(y)[i] = t;
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      double t = y[n - 1];
#pragma unroll
      for (int j = 0; j < K; j++) { t = __fma_rn(alpha.a[j], x.p[j][n - 1], t); }
      y[n - 1] = t;
   }
}

// One step of modified Gram-Schmidt in one pass (par_gmres.cpp): y += a x, rounded like axpy_kernel rounds it (the
// same expression under the same contraction rule), and this workgroup's share of <z, y> of the updated y, walked and
// folded like dot_partial_kernel walks and folds <z, y>: the grid of a dot product, the same trips, the same per-pair
// term, the same fold.  SELF: z is y (the last step of a column takes the squared norm), and y is read once.  No
// restrict on the vectors: z may be y.
template <bool SELF>
__global__ __launch_bounds__(256)
void mgs_step_kernel(double a, const double *x, double *y, const double *z, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[4];
   double acc = 0.0;
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      double2 t = reinterpret_cast<double2 *>(y)[i];
      double2 zv;
      if (!SELF) { zv = reinterpret_cast<const double2 *>(z)[i]; }
      t.x += a * xv.x; t.y += a * xv.y;
      reinterpret_cast<double2 *>(y)[i] = t;
      acc += dot_pair(SELF ? t : zv, t);
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      double t = y[n - 1];
      t += a * x[n - 1];
      y[n - 1] = t;
      acc = dot_last(SELF ? t : z[n - 1], t, acc);
   }
   acc = wave_sum(acc);
   if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = acc; }
   __syncthreads();
   if (threadIdx.x == 0) { partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]); }
}

// The end of an LGMRES restart cycle (par_gmres.cpp, lgmres_core.hpp), each of the two in one pass.
//
// y = x and this workgroup's share of <x, x>: the copy of copy_kernel, and the partials dot_partial_kernel leaves for
// <y, y> of the copy (the grid of a dot product, the same trips, the same per-pair term, the same fold).
__global__ __launch_bounds__(256)
void copy_norm2_kernel(const double *__restrict__ x, double *__restrict__ y, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[4];
   double acc = 0.0;
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      reinterpret_cast<double2 *>(y)[i] = xv;
      acc += dot_pair(xv, xv);
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      const double t = x[n - 1];
      y[n - 1] = t;
      acc = dot_last(t, t, acc);
   }
   acc = wave_sum(acc);
   if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = acc; }
   __syncthreads();
   if (threadIdx.x == 0) { partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]); }
}

// z = (y - x) na, two roundings spelled out so that nothing is contracted: what copy (z = x), scale by -1, axpy with
// coefficient 1 (z = y - x, one rounding whether or not the product with 1 is fused) and scale by na leave.  The caller
// hands na = -a for z = a (x - y); the difference is taken as y - x so that equal elements give the zero of that sequence.
__global__ void scaled_diff_kernel(double na, const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ z, size_t n)
{
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      const double2 yv = reinterpret_cast<const double2 *>(y)[i];
      reinterpret_cast<double2 *>(z)[i] = make_double2(__dmul_rn(__dsub_rn(yv.x, xv.x), na), __dmul_rn(__dsub_rn(yv.y, xv.y), na));
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { z[n - 1] = __dmul_rn(__dsub_rn(y[n - 1], x[n - 1]), na); }
}

// The vector work of a BiCGSTAB iteration outside its two preconditioner applications and two products with A
// (par_bicgstab.cpp, krylov/bicgstab.c:473-560), three kernels.
//
// <x, y> and <y, y> in one pass over x and y: the partials dot_partial_kernel leaves for each (accumulator 0 and 1), y
// read once.
__global__ __launch_bounds__(256)
void dot_with_norm2_kernel(const double *__restrict__ x, const double *__restrict__ y, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[2][4];
   double acc[2] = {0.0, 0.0};
   VEC_LOOP_BEGIN
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      const double2 yv = reinterpret_cast<const double2 *>(y)[i];
      acc[0] += dot_pair(xv, yv);
      acc[1] += dot_pair(yv, yv);
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      acc[0] = dot_last(x[n - 1], y[n - 1], acc[0]);
      acc[1] = dot_last(y[n - 1], y[n - 1], acc[1]);
   }
   MASS_FOLD(acc, wsum, 2)
}

// x += a v and r += b s, each rounded like axpy_kernel rounds it (the same expression under the same contraction rule),
// and the partials of <r, r> (accumulator 0) and <r0, r> (accumulator 1) of the updated r, walked and folded like
// dot_partial_kernel walks and folds them.  The six vectors are distinct.
__global__ __launch_bounds__(256)
void bicgstab_update_kernel(double a, const double *__restrict__ v, double *__restrict__ x, double b, const double *__restrict__ s,
                            double *__restrict__ r, const double *__restrict__ r0, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[2][4];
   double acc[2] = {0.0, 0.0};
   VEC_LOOP_BEGIN
      const double2 vv = reinterpret_cast<const double2 *>(v)[i];
      const double2 sv = reinterpret_cast<const double2 *>(s)[i];
      const double2 zv = reinterpret_cast<const double2 *>(r0)[i];
      double2 xv = reinterpret_cast<double2 *>(x)[i];
      double2 rv = reinterpret_cast<double2 *>(r)[i];
      xv.x += a * vv.x; xv.y += a * vv.y;
      rv.x += b * sv.x; rv.y += b * sv.y;
      reinterpret_cast<double2 *>(x)[i] = xv;
      reinterpret_cast<double2 *>(r)[i] = rv;
      acc[0] += dot_pair(rv, rv);
      acc[1] += dot_pair(zv, rv);
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      x[n - 1] += a * v[n - 1];
      double t = r[n - 1];
      t += b * s[n - 1];
      r[n - 1] = t;
      acc[0] = dot_last(t, t, acc[0]);
      acc[1] = dot_last(r0[n - 1], t, acc[1]);
   }
   MASS_FOLD(acc, wsum, 2)
}

// p = r + c (p + g q), three roundings spelled out so that nothing is contracted across them: the fused multiply-add of
// axpy_kernel for p + g q, the product of scale_kernel, the sum axpy_kernel leaves for a coefficient of 1.  c == 0 is
// the shortcut of hypre_SeqVectorScale (zero whatever p + g q holds); at c == 1, its other one, the product is exact.
__device__ __forceinline__ double bicgstab_direction(double g, double q, double c, double r, double p)
{
   const double t = __fma_rn(g, q, p);
   return __dadd_rn(c == 0.0 ? 0.0 : __dmul_rn(t, c), r);
}
__global__ void bicgstab_direction_kernel(double g, const double *__restrict__ q, double c, const double *__restrict__ r,
                                          double *__restrict__ p, size_t n)
{
   VEC_LOOP_BEGIN
      const double2 qv = reinterpret_cast<const double2 *>(q)[i];
      const double2 rv = reinterpret_cast<const double2 *>(r)[i];
      const double2 pv = reinterpret_cast<double2 *>(p)[i];
      reinterpret_cast<double2 *>(p)[i] = make_double2(bicgstab_direction(g, qv.x, c, rv.x, pv.x), bicgstab_direction(g, qv.y, c, rv.y, pv.y));
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { p[n - 1] = bicgstab_direction(g, q[n - 1], c, r[n - 1], p[n - 1]); }
}

// The vector work of a diagonally scaled CG iteration between the product with A and the direction update (par_pcg.cpp,
// krylov/pcg.c:716-760 behind HYPRE_ParCSRDiagScale), one kernel.  On entry s holds A p.
//
// x += a p and r += na s with the expressions of pcg_update_kernel, s = r ./ d with the division of
// diag_first_scale_kernel, and the partials of <r, r> (accumulator 0, the term of pcg_update_kernel) and of <r, s>
// (accumulator 1, the term of dot_partial_kernel), walked and folded like those two walk and fold them.  d is the packed
// diagonal; the five vectors are distinct.
__global__ __launch_bounds__(256)
void dscg_step_kernel(double a, double na, const double *__restrict__ p, const double *__restrict__ d, double *__restrict__ s,
                      double *__restrict__ x, double *__restrict__ r, size_t n, double *__restrict__ partial)
{
   __shared__ double wsum[2][4];
   double acc[2] = {0.0, 0.0};
   VEC_LOOP_BEGIN
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      const double2 dv = reinterpret_cast<const double2 *>(d)[i];
      double2 sv = reinterpret_cast<double2 *>(s)[i];
      double2 xv = reinterpret_cast<double2 *>(x)[i];
      double2 rv = reinterpret_cast<double2 *>(r)[i];
      xv.x += a * pv.x; xv.y += a * pv.y;
      rv.x += na * sv.x; rv.y += na * sv.y;
      sv.x = rv.x / dv.x; sv.y = rv.y / dv.y;
      reinterpret_cast<double2 *>(x)[i] = xv;
      reinterpret_cast<double2 *>(r)[i] = rv;
      reinterpret_cast<double2 *>(s)[i] = sv;
      acc[0] += rv.x * rv.x + rv.y * rv.y;
      acc[1] += dot_pair(rv, sv);
   VEC_LOOP_END
   if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
   {
      x[n - 1] += a * p[n - 1];
      const double rl = r[n - 1] + na * s[n - 1];
      const double sl = rl / d[n - 1];
      r[n - 1] = rl;
      s[n - 1] = sl;
      acc[0] += rl * rl;
      acc[1] = dot_last(rl, sl, acc[1]);
   }
   MASS_FOLD(acc, wsum, 2)
}

// d[i] = the first entry of row i of the local block, which is its diagonal (par_csr_matop.c:6479-6575), where the row
// has one; a row without entries gets 1 and raises the flag: the caller then keeps to the plain diagonal scaling
__global__ void pack_first_entries_kernel(const int *__restrict__ Ai, const double *__restrict__ Aa, double *__restrict__ d, size_t n,
                                          int *__restrict__ flag)
{
   for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
   {
      const int k = Ai[i];
      if (k < Ai[i + 1]) { d[i] = Aa[k]; }
      else { d[i] = 1.0; *flag = 1; }
   }
}

// ---------------------------------------------------------------------------
// launchers: k vectors in chunks of MASS_CHUNK, one kernel instance per chunk length
// ---------------------------------------------------------------------------
namespace {
inline int dot_grid(size_t n)
{
   const int nb = vec_grid(n);
   return nb > DOT_BLOCKS ? DOT_BLOCKS : nb;
}
// device scratch of a batched dot: room for `results` sums in front (a multiple of 16 doubles), the partials of one chunk behind
inline double *mass_scratch(int results, double **partial)
{
   const size_t front = ((size_t) results + 15) & ~(size_t) 15;
   double *base = reduce_scratch(front + 2 * (size_t) MASS_CHUNK * DOT_BLOCKS);
   *partial = base + front;
   return base;
}

template <int K>
void mass_dot_chunk(const double *x, const double *const *y, size_t n, int nb, double *partial, hipStream_t s)
{
   MassVectors<K> v;
   for (int j = 0; j < K; j++) { v.p[j] = y[j]; }
   hipLaunchKernelGGL(mass_dot_kernel<K>, dim3(nb), dim3(256), 0, s, x, v, n, partial);
}
template <int K>
void mass_dot_two_chunk(const double *x, const double *y, const double *const *z, size_t n, int nb, double *partial, hipStream_t s)
{
   MassVectors<K> v;
   for (int j = 0; j < K; j++) { v.p[j] = z[j]; }
   hipLaunchKernelGGL(mass_dot_two_kernel<K>, dim3(nb), dim3(256), 0, s, x, y, v, n, partial);
}
template <int K>
void mass_axpy_chunk(const double *alpha, const double *const *x, double *y, size_t n, hipStream_t s)
{
   MassCoefficients<K> a;
   MassVectors<K> v;
   for (int j = 0; j < K; j++) { a.a[j] = alpha[j]; v.p[j] = x[j]; }
   hipLaunchKernelGGL(mass_axpy_kernel<K>, dim3(vec_grid(n)), dim3(256), 0, s, a, v, y, n);
}
}  // namespace

#define MASS_DISPATCH(kk, CALL)                                                          \
   switch (kk)                                                                           \
   {                                                                                     \
      case 1: CALL(1); break;                                                            \
      case 2: CALL(2); break;                                                            \
      case 3: CALL(3); break;                                                            \
      case 4: CALL(4); break;                                                            \
      case 5: CALL(5); break;                                                            \
      case 6: CALL(6); break;                                                            \
      case 7: CALL(7); break;                                                            \
      default: CALL(8); break;                                                           \
   }
static_assert(MASS_CHUNK == 8, "the dispatch lists the chunk lengths 1 .. 8");

double *launch_mass_dot(const double *x, const double *const *y, int k, size_t n, hipStream_t s)
{
   double *partial;
   double *out = mass_scratch(k, &partial);
   const int nb = dot_grid(n);
   for (int c = 0; c < k; c += MASS_CHUNK)
   {
      const int kk = k - c < MASS_CHUNK ? k - c : MASS_CHUNK;
      account_bytes(8.0 * (kk + 1) * n);
#define CALL(K) mass_dot_chunk<K>(x, y + c, n, nb, partial, s)
      MASS_DISPATCH(kk, CALL)
#undef CALL
      hipLaunchKernelGGL(mass_dot_final_kernel, dim3(kk), dim3(256), 0, s, partial, nb, kk, out + c, out + c);
   }
   return out;
}

double *launch_mass_dot_two(const double *x, const double *y, const double *const *z, int k, size_t n, hipStream_t s)
{
   double *partial;
   double *out = mass_scratch(2 * k, &partial);
   const int nb = dot_grid(n);
   for (int c = 0; c < k; c += MASS_CHUNK)
   {
      const int kk = k - c < MASS_CHUNK ? k - c : MASS_CHUNK;
      account_bytes(8.0 * (kk + 2) * n);
#define CALL(K) mass_dot_two_chunk<K>(x, y, z + c, n, nb, partial, s)
      MASS_DISPATCH(kk, CALL)
#undef CALL
      hipLaunchKernelGGL(mass_dot_final_kernel, dim3(2 * kk), dim3(256), 0, s, partial, nb, kk, out + c, out + k + c);
   }
   return out;
}

void launch_mass_axpy(const double *alpha, const double *const *x, double *y, int k, size_t n, hipStream_t s)
{
   if (!n) { return; }
   for (int c = 0; c < k; c += MASS_CHUNK)
   {
      const int kk = k - c < MASS_CHUNK ? k - c : MASS_CHUNK;
      account_bytes(8.0 * (kk + 2) * n);
#define CALL(K) mass_axpy_chunk<K>(alpha + c, x + c, y, n, s)
      MASS_DISPATCH(kk, CALL)
#undef CALL
   }
}

// y += a x and d_out[0] = <z, y> of the updated y (this rank's part): the bits of launch_axpy(a, x, y) followed by
// launch_dot(z, y), in 32 n bytes instead of 40 n (24 n instead of 40 n when z is y) and one launch less
void launch_axpy_dot(double a, const double *x, double *y, const double *z, size_t n, double *d_out, hipStream_t s)
{
   const bool self = z == y;
   account_bytes((self ? 24.0 : 32.0) * n);
   const int nb = dot_grid(n);
   double *partial = reduce_scratch(DOT_BLOCKS + 16) + 16;
   if (self) { hipLaunchKernelGGL(mgs_step_kernel<true>, dim3(nb), dim3(256), 0, s, a, x, y, z, n, partial); }
   else { hipLaunchKernelGGL(mgs_step_kernel<false>, dim3(nb), dim3(256), 0, s, a, x, y, z, n, partial); }
   launch_dot_final(partial, nb, d_out, s);
}

// y = x and d_out[0] = <x, x> (this rank's part): the bits of launch_copy(y, x) followed by launch_dot(y, y), in 16 n
// bytes instead of 32 n
void launch_copy_norm2(const double *x, double *y, size_t n, double *d_out, hipStream_t s)
{
   account_bytes(16.0 * n);
   const int nb = dot_grid(n);
   double *partial = reduce_scratch(DOT_BLOCKS + 16) + 16;
   hipLaunchKernelGGL(copy_norm2_kernel, dim3(nb), dim3(256), 0, s, x, y, n, partial);
   launch_dot_final(partial, nb, d_out, s);
}

// z = a (x - y); z is neither x nor y.  The bits of launch_copy(z, x), launch_scale(z, -1), launch_axpy(1, y, z),
// launch_scale(z, -a), in 24 n bytes instead of 72 n
void launch_scaled_diff(double a, const double *x, const double *y, double *z, size_t n, hipStream_t s)
{
   account_bytes(24.0 * n);
   if (n) { hipLaunchKernelGGL(scaled_diff_kernel, dim3(vec_grid(n)), dim3(256), 0, s, -a, x, y, z, n); }
}

// d_out[0] = <x, y>, d_out[1] = <y, y> (this rank's part): the bits of launch_dot(x, y) and launch_dot(y, y), in 16 n
// bytes instead of 32 n; returns d_out, in device scratch and valid until the next reduction
double *launch_dot_with_norm2(const double *x, const double *y, size_t n, hipStream_t s)
{
   account_bytes(16.0 * n);
   double *partial;
   double *out = mass_scratch(2, &partial);
   const int nb = dot_grid(n);
   hipLaunchKernelGGL(dot_with_norm2_kernel, dim3(nb), dim3(256), 0, s, x, y, n, partial);
   HIP_CHECK(hipGetLastError());
   hipLaunchKernelGGL(mass_dot_final_kernel, dim3(2), dim3(256), 0, s, partial, nb, 2, out, out);
   HIP_CHECK(hipGetLastError());
   return out;
}

// x += a v, r += b s, d_out[0] = <r, r>, d_out[1] = <r0, r> of the updated r (this rank's part): the bits of
// launch_axpy(a, v, x), launch_axpy(b, s, r), launch_dot(r, r), launch_dot(r0, r), in 56 n bytes instead of 80 n and 2
// launches instead of 6; returns d_out as above
double *launch_bicgstab_update(double a, const double *v, double *x, double b, const double *sv, double *r, const double *r0, size_t n,
                               hipStream_t s)
{
   account_bytes(56.0 * n);
   double *partial;
   double *out = mass_scratch(2, &partial);
   const int nb = dot_grid(n);
   hipLaunchKernelGGL(bicgstab_update_kernel, dim3(nb), dim3(256), 0, s, a, v, x, b, sv, r, r0, n, partial);
   HIP_CHECK(hipGetLastError());
   hipLaunchKernelGGL(mass_dot_final_kernel, dim3(2), dim3(256), 0, s, partial, nb, 2, out, out);
   HIP_CHECK(hipGetLastError());
   return out;
}

// p = r + c (p + g q); p is neither q nor r.  The bits of launch_axpy(g, q, p), launch_scale(p, c) with the shortcuts of
// hypre_SeqVectorScale, launch_axpy(1, r, p), in 32 n bytes instead of 64 n
void launch_bicgstab_direction(double g, const double *q, double c, const double *r, double *p, size_t n, hipStream_t s)
{
   account_bytes(32.0 * n);
   if (!n) { return; }
   hipLaunchKernelGGL(bicgstab_direction_kernel, dim3(vec_grid(n)), dim3(256), 0, s, g, q, c, r, p, n);
   HIP_CHECK(hipGetLastError());
}

// x += a p, r += na s, s = r ./ d, d_out[0] = <r, r>, d_out[1] = <r, s> (this rank's part; d_out is the caller's): the
// bits of launch_pcg_update(a, na, p, s, x, r), launch_diag_first_scale on the rows d was packed from and
// launch_dot(r, s), in 64 n bytes (p, d, s, x, r read; x, r, s written) instead of 48 n + 28 n + 16 n, the 28 with the
// row pointer and the gathered value, and 2 launches instead of 5
void launch_dscg_step(double a, double na, const double *p, const double *d, double *sv, double *x, double *r, size_t n, double *d_out,
                      hipStream_t s)
{
   account_bytes(64.0 * n);
   double *partial;
   (void) mass_scratch(2, &partial);
   const int nb = dot_grid(n);
   hipLaunchKernelGGL(dscg_step_kernel, dim3(nb), dim3(256), 0, s, a, na, p, d, sv, x, r, n, partial);
   HIP_CHECK(hipGetLastError());
   hipLaunchKernelGGL(mass_dot_final_kernel, dim3(2), dim3(256), 0, s, partial, nb, 2, d_out, d_out);
   HIP_CHECK(hipGetLastError());
}

// d[0..n) = the diagonal of the n rows (their first entries); *d_flag, a device int the caller has cleared, is raised
// when a row has no entry
void launch_pack_first_entries(const int *Ai, const double *Aa, double *d, size_t n, int *d_flag, hipStream_t s)
{
   account_bytes(20.0 * n);
   if (!n) { return; }
   size_t g = (n + 255) / 256;
   if (g > 2048) { g = 2048; }
   hipLaunchKernelGGL(pack_first_entries_kernel, dim3((unsigned) g), dim3(256), 0, s, Ai, Aa, d, n, d_flag);
   HIP_CHECK(hipGetLastError());
}

// what the tests need to know of the launch shape: the elements one pass of the dot-product grid covers
size_t dot_grid_pass_elements() { return (size_t) DOT_BLOCKS * 256 * 2; }

void preload_mass_kernels() { hipFuncAttributes at; (void) hipFuncGetAttributes(&at, (const void *) mass_dot_final_kernel); (void) hipGetLastError(); }

}  // namespace hamd
