// hypre_amd — the triangular solves of one ILU application as Jacobi sweeps (hypre_ILUSolveLUIter, par_ilu_solve.c:960-1110).
//
// A sweep is a product with a strictly triangular factor: no dependency levels, one launch whatever the grid size.  The
// factor lies in row slices of 64 rows (ilu_device.hpp: IluSlices), a wave per slice, a lane per row.  The lane walks its
// slice column by column — the wave's k-th load of indices and of values is one contiguous line — and runs the host's chain
// (ilu::solve_iter, ilu_host.hpp): the sum starts at +0.0, the products are added one by one in stored order, every product
// and every sum rounded, then rhs - sum, for U times the inverse pivot.  A short row stops at its own length; the padding
// behind it is never read.  So the result has the host's bits whatever the launch geometry.  No atomics, no shuffles, no
// LDS, no fused multiply-adds.  Sweeps are OUT OF PLACE: `in` is read by every lane of the grid, `out` / `scaled` written by
// the row's own lane, and the caller hands in distinct buffers.
//    L:  y_i = r_i - sum_k val_k in[col_k];   with scale:  z_i = dinv_i y_i   (the first upper iterate, sums of +0.0)
//    U:  z_i = dinv_i (y_i - sum_k val_k in[col_k])
//    with u:  u_i += the last of these (the scatter through the permutation is row[])
#include "ilu_device.hpp"

#pragma clang fp contract(off)

namespace hamd {

template <bool UPPER>
__global__ __launch_bounds__(ILU_SWEEP_THREADS)
void ilu_sweep_kernel(IluSweepArgs a)
{
   const int slot = (int) (blockIdx.x * blockDim.x + threadIdx.x);
   const int slice = slot >> 6;
   if (slice >= a.t.nslices) { return; }
   const int r = a.t.row[slot];
   if (r < 0) { return; }
   const double *in = a.in;
   const int len = in ? a.t.len[slot] : 0;
   const size_t first = (size_t) a.t.base[slice] + (size_t) (slot & 63);
   const int *col = a.t.col + first;
   const double *val = a.t.val + first;
   const double rhs = a.rhs[r];
   double sum = 0.0;
   int k = 0;
   // four entries' loads and gathers in flight, the additions in stored order
   for (; k + 4 <= len; k += 4)
   {
      const int c0 = col[64 * k], c1 = col[64 * (k + 1)], c2 = col[64 * (k + 2)], c3 = col[64 * (k + 3)];
      const double v0 = val[64 * k], v1 = val[64 * (k + 1)], v2 = val[64 * (k + 2)], v3 = val[64 * (k + 3)];
      const double x0 = in[c0], x1 = in[c1], x2 = in[c2], x3 = in[c3];
      sum += v0 * x0;
      sum += v1 * x1;
      sum += v2 * x2;
      sum += v3 * x3;
   }
   for (; k < len; k++) { sum += val[64 * k] * in[col[64 * k]]; }
   double x = rhs - sum;
   if (UPPER) { x = a.t.dinv[slot] * x; }
   if (a.out) { a.out[r] = x; }
   if (!UPPER && a.scale)
   {
      x = a.t.dinv[slot] * x;
      if (a.scaled) { a.scaled[r] = x; }
   }
   if (a.u) { a.u[r] = a.u[r] + x; }
}

void launch_ilu_sweep(const IluSweepArgs &a, bool upper, hipStream_t s)
{
   if (a.t.nslices <= 0) { return; }
   const int per_block = ILU_SWEEP_THREADS / 64;
   const dim3 grid((unsigned) ((a.t.nslices + per_block - 1) / per_block)), block(ILU_SWEEP_THREADS);
   if (upper) { hipLaunchKernelGGL(ilu_sweep_kernel<true>, grid, block, 0, s, a); }
   else { hipLaunchKernelGGL(ilu_sweep_kernel<false>, grid, block, 0, s, a); }
}

// loaded with the device (runtime.cpp: ensure_device), like every kernel file
void preload_ilu_iter_kernels() { hipFuncAttributes at; (void) hipFuncGetAttributes(&at, (const void *) ilu_sweep_kernel<true>); (void) hipGetLastError(); }

}  // namespace hamd
