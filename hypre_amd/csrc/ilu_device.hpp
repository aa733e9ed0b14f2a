// hypre_amd — what par_ilu.cpp and ilu_kernels.hip share: a triangular factor as it lies in device memory.
#pragma once
#include "internal.hpp"

namespace hamd {

// One factor (L or U) in LEVEL ORDER.  Slot s is the s-th row of the level order: the rows of a level are consecutive slots,
// their entries consecutive in col / val, every row's entries in the order the factorisation stored them.  The
// permutation is folded in once, at setup: row[s] and col[k] index the vectors of the solve (ftemp, utemp, u) directly.
// 12 bytes per entry (4 index, 8 value), per row 8 bytes of row table and, for U, 8 of inverse pivot.
struct IluTri
{
   const int    *ptr = nullptr;      // [n + 1] first entry of every slot
   const int    *row = nullptr;      // [n] vector index of the slot's row
   const int    *col = nullptr;      // [nnz] vector index of the entry's column
   const double *val = nullptr;      // [nnz]
   const double *dinv = nullptr;     // [n] inverse pivot of the slot's row (U only)
   const int    *lev_start = nullptr;   // [nlev + 1] first slot of every level
};

struct IluArgs
{
   IluTri        t;
   const double *ftemp;              // right-hand side of the L solve (read by L only)
   double       *utemp;              // L writes it, U reads and overwrites it
   double       *u;                  // U adds its result to the iterate
};

constexpr int ILU_RUN_THREADS = 1024;    // a level of at most this many rows is swept inside a run
constexpr int ILU_RUN_MAX_LEVELS = 8192; // level offsets of a run sit in LDS

// one level of more than ILU_RUN_THREADS rows: a grid of its own
void launch_ilu_level(const IluArgs &a, bool upper, int start, int count, hipStream_t s);
// levels [lev_begin, lev_end), each at most ILU_RUN_THREADS rows: one workgroup, a barrier between levels
void launch_ilu_run(const IluArgs &a, bool upper, int lev_begin, int lev_end, hipStream_t s);
void preload_ilu_kernels();

// ---- iterative triangular solves: a factor in ROW SLICES of 64 rows, one per wave (ilu_host.hpp: Slices) ----
// Entry k of lane l of a slice lies at base[slice] + 64 k + l in col / val, so a wave's k-th load is one contiguous line of
// 256 bytes (indices) or 512 (values).  Slot tables are padded to whole slices; a slot past the last row has row -1.
// Per stored (padded) entry 12 bytes, per row 16 of slot tables (length, vector index, inverse pivot), per slice 8.
struct IluSlices
{
   const long long *base = nullptr;  // [nslices] first entry of the slice
   const int       *len = nullptr;   // [64 nslices] entries of the slot's row: a short row stops here, padding is never read
   const int       *row = nullptr;   // [64 nslices] vector index of the slot's row, -1 behind the last row
   const int       *col = nullptr;   // [padded] vector index of the entry's column
   const double    *val = nullptr;   // [padded]
   const double    *dinv = nullptr;  // [64 nslices] inverse pivot of the slot's row
   int              nslices = 0;
};

// One Jacobi sweep, out of place:  x_i = rhs_i - sum_j T_ij in_j,  for U then x_i = dinv_i x_i.
struct IluSweepArgs
{
   IluSlices     t;
   const double *rhs = nullptr;      // L: the residual r; U: the last lower iterate y
   const double *in = nullptr;       // iterate k - 1; NULL: the zero iterate, no entry of the factor is read
   double       *out = nullptr;      // iterate k; NULL: not stored
   int           scale = 0;          // L only: go on with dinv_i x_i, the first upper iterate, for the two stores below
   double       *scaled = nullptr;   // L with scale: where that first upper iterate goes; NULL: not stored
   double       *u = nullptr;        // u_i += the row's final value (the last pass of an application); NULL: no update
};

constexpr int ILU_SWEEP_THREADS = 256;   // four slices a workgroup
void launch_ilu_sweep(const IluSweepArgs &a, bool upper, hipStream_t s);
void preload_ilu_iter_kernels();

}  // namespace hamd
