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

}  // namespace hamd
