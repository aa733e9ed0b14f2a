// hypre_amd — what the Krylov solvers on ParVectors share (par_pcg.cpp, par_gmres.cpp): the work vectors of Setup, the
// preconditioner an application hands to HYPRE_*SetPrecond, and how a Solve begins.
#pragma once
#include "amg_internal.hpp"

namespace hamd {

// a work vector shaped like x: as many columns as a multivector x has (`ij -nc N`), at x's memory location (CreateVector
// of krylov/pcg.c:226-260, gmres.c:204-215, cogmres.c:220-231, flexgmres.c:230-250)
inline hypre_ParVector *par_vector_like(hypre_ParCSRMatrix *A, hypre_ParVector *x)
{
   hypre_ParVector *v = hypre_ParMultiVectorCreate(A->comm, A->global_num_rows, A->row_starts, x->local_vector->num_vectors);
   hypre_ParVectorInitialize_v2(v, x->local_vector->memory_location);
   return v;
}

struct KrylovPrecond
{
   HYPRE_PtrToSolverFcn solve = nullptr, setup = nullptr;
   HYPRE_Solver data = nullptr;
   HYPRE_Int set(HYPRE_PtrToSolverFcn solve_, HYPRE_PtrToSolverFcn setup_, HYPRE_Solver data_)
   {
      solve = solve_; setup = setup_; data = data_;
      return hypre_error_flag;
   }
   // sol = M^-1 rhs, or rhs itself without a preconditioner.  The target is cleared first (ClearVector: all_zeros = 1,
   // par_vector.c:335-340; pcg.c, gmres.c:538, cogmres.c:541, flexgmres.c:549); `before` runs between the two.
   template <class Before> void apply(hypre_ParCSRMatrix *A, hypre_ParVector *rhs, hypre_ParVector *sol, Before before) const
   {
      hypre_ParVectorSetZeros(sol);
      before();
      if (solve) { solve(data, A, rhs, sol); }
      else { hypre_ParVectorCopy(rhs, sol); }
   }
   void apply(hypre_ParCSRMatrix *A, hypre_ParVector *rhs, hypre_ParVector *sol) const { apply(A, rhs, sol, [] {}); }
};

// the body of a Solve: no synchronisation after every vector call (QuietSync), and it never starts from a plan its matrix
// has moved away from
struct __attribute__((visibility("hidden"))) QuietSolve : QuietSync
{
   explicit QuietSolve(hypre_ParCSRMatrix *A) { verify_par_plans(A); }
};

}  // namespace hamd
