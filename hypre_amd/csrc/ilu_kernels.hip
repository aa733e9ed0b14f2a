// hypre_amd — the two triangular solves of one ILU application (hypre_ILUSolveLU, par_ilu_solve.c:829-950) by levels.
//
// A factor lies in level order (ilu_device.hpp: IluTri): the rows of a level are independent, levels run in order.  One
// lane owns one row and runs the host's chain — start from the right-hand side, take the products away one by one in
// stored order, every product and every difference rounded — so the result has the bits of ilu::solve (ilu_host.hpp)
// whatever the launch geometry.  No atomics, no shuffles, no fused multiply-adds.
//    L:  utemp[r] = ftemp[r] - sum_k val[k] * utemp[col[k]]                       (unit diagonal; the gather of ftemp
//                                                                                   through the permutation is row[])
//    U:  utemp[r] = (utemp[r] - sum_k val[k] * utemp[col[k]]) * dinv,  u[r] += utemp[r]   (scatter and update in the write)
#include "ilu_device.hpp"

#pragma clang fp contract(off)

namespace hamd {

// what a row needs before it can gather utemp: factor data only, nothing a solve writes
struct IluRowHead { int r, s, e; double start_or_dinv; };

template <bool UPPER>
__device__ __forceinline__ IluRowHead ilu_row_head(const IluArgs &a, int slot)
{
   IluRowHead h;
   h.r = a.t.row[slot];
   h.s = a.t.ptr[slot];
   h.e = a.t.ptr[slot + 1];
   h.start_or_dinv = UPPER ? a.t.dinv[slot] : a.ftemp[h.r];
   return h;
}

template <bool UPPER>
__device__ __forceinline__ void ilu_row(const IluArgs &a, const IluRowHead &h)
{
   double *ut = a.utemp;
   double sum = UPPER ? ut[h.r] : h.start_or_dinv;
   for (int k = h.s; k < h.e; k++) { sum -= a.t.val[k] * ut[a.t.col[k]]; }
   if (UPPER)
   {
      const double x = sum * h.start_or_dinv;
      ut[h.r] = x;
      a.u[h.r] = a.u[h.r] + x;
   }
   else { ut[h.r] = sum; }
}

// one large level: a lane per row, as many workgroups as the level needs
template <bool UPPER>
__global__ __launch_bounds__(256)
void ilu_level_kernel(IluArgs a, int start, int count)
{
   const int t = (int) (blockIdx.x * blockDim.x + threadIdx.x);
   if (t >= count) { return; }
   ilu_row<UPPER>(a, ilu_row_head<UPPER>(a, start + t));
}

// A run of levels inside one workgroup: lane t takes row t of every level, a barrier closes every level.  The head of a
// lane's row in the next level (factor data) is fetched while this level gathers, so a level costs the gather's round
// trips and the barrier, not the row table's as well.
template <bool UPPER>
__global__ __launch_bounds__(ILU_RUN_THREADS)
void ilu_run_kernel(IluArgs a, int lev_begin, int lev_end)
{
   extern __shared__ int s_lev[];                  // lev_start[lev_begin .. lev_end]
   const int nl = lev_end - lev_begin, t = (int) threadIdx.x;
   for (int i = t; i <= nl; i += (int) blockDim.x) { s_lev[i] = a.t.lev_start[lev_begin + i]; }
   __syncthreads();
   IluRowHead next{0, 0, 0, 0.0};
   bool have_next = s_lev[0] + t < s_lev[1];
   if (have_next) { next = ilu_row_head<UPPER>(a, s_lev[0] + t); }
   for (int l = 0; l < nl; l++)
   {
      const IluRowHead h = next;
      const bool have = have_next;
      have_next = l + 1 < nl && s_lev[l + 1] + t < s_lev[l + 2];
      if (have_next) { next = ilu_row_head<UPPER>(a, s_lev[l + 1] + t); }
      if (have) { ilu_row<UPPER>(a, h); }
      __threadfence_block();
      __syncthreads();
   }
}

void launch_ilu_level(const IluArgs &a, bool upper, int start, int count, hipStream_t s)
{
   if (count <= 0) { return; }
   const dim3 grid((unsigned) ((count + 255) / 256)), block(256);
   if (upper) { hipLaunchKernelGGL(ilu_level_kernel<true>, grid, block, 0, s, a, start, count); }
   else { hipLaunchKernelGGL(ilu_level_kernel<false>, grid, block, 0, s, a, start, count); }
}

void launch_ilu_run(const IluArgs &a, bool upper, int lev_begin, int lev_end, hipStream_t s)
{
   if (lev_end <= lev_begin) { return; }
   const size_t lds = sizeof(int) * (size_t) (lev_end - lev_begin + 1);
   if (upper) { hipLaunchKernelGGL(ilu_run_kernel<true>, dim3(1), dim3(ILU_RUN_THREADS), lds, s, a, lev_begin, lev_end); }
   else { hipLaunchKernelGGL(ilu_run_kernel<false>, dim3(1), dim3(ILU_RUN_THREADS), lds, s, a, lev_begin, lev_end); }
}

// loaded with the device (runtime.cpp: ensure_device), like every kernel file
void preload_ilu_kernels() { hipFuncAttributes at; (void) hipFuncGetAttributes(&at, (const void *) ilu_level_kernel<true>); (void) hipGetLastError(); }

}  // namespace hamd
