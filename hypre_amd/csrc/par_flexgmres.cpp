// hypre_amd — flexible GMRES: right-preconditioned restarted GMRES that keeps the preconditioned vectors, so the
// preconditioner may change from one application to the next (the reference's `ij -solver 60 | 61`).
//
// Reference: krylov/flexgmres.c:330-760 (hypre_FlexGMRESSolve) with parcsr_ls/HYPRE_parcsr_flexgmres.c and
// krylov/HYPRE_flexgmres.c for the entry points; defaults of hypre_FlexGMRESCreate (flexgmres.c:86-91): k_dim 20,
// tol 1e-6, a_tol 0, min_iter 0, max_iter 1000.  The iteration itself (Hessenberg matrix, Givens rotations, every
// decision) is flexgmres_core.hpp; this file gives it the vectors: ParVectors on the device, every inner product ending
// in one scalar read-back.  Before every preconditioner call the target is cleared and modify_pc(precond_data, iter,
// r_norm / den_norm) is called; the correction of a restart cycle is sum_j rs_j pre_vecs[j], so nothing is unwound
// through the preconditioner.  The convergence-factor exit (cf_tol) is not carried, as in par_gmres.cpp.
//
// Modified Gram-Schmidt, fused (the default): step i is one hypre_ParVectorInnerProd and i launches of
// launch_axpy_dot, each subtracting the projection on p[j] and leaving <p[j + 1], p[i]> (the last one |p[i]|^2) in the
// same pass: 32 i + 8 bytes per element in i + 1 launches, where the dot / axpy sequence of the reference moves 40 i + 8
// in 2 i + 1.  Same order of operations and same roundings, so a solve has the same bits either way
// (hypre_amd_FlexGMRESSetFusedOrthogonalization).
#include "amg_internal.hpp"
#include "flexgmres_core.hpp"
#include <cstring>
#include <vector>

using namespace hamd;

struct hypre_amd_FlexGMRESData
{
   hypre_Solver base;
   MPI_Comm comm;
   FlexGMRESParams prm;
   HYPRE_PtrToSolverFcn precond = nullptr, precond_setup = nullptr;
   HYPRE_Solver precond_data = nullptr;
   HYPRE_PtrToModifyPCFcn modify_pc = nullptr;          // nullptr: hypre_FlexGMRESModifyPCDefault, which does nothing
   hypre_ParVector *r = nullptr, *w = nullptr;
   std::vector<hypre_ParVector *> p, pre_vecs;
   HYPRE_Int num_iterations = 0, converged = 0;
   HYPRE_Real rel_residual_norm = 0.0;
   HYPRE_Int fused_steps = 0, plain_dots = 0, plain_axpys = 0;
};

namespace {
void free_vectors(hypre_amd_FlexGMRESData *d)
{
   hypre_ParVectorDestroy(d->r); hypre_ParVectorDestroy(d->w);
   d->r = d->w = nullptr;
   for (hypre_ParVector *v : d->p) { hypre_ParVectorDestroy(v); }
   for (hypre_ParVector *v : d->pre_vecs) { hypre_ParVectorDestroy(v); }
   d->p.clear(); d->pre_vecs.clear();
}

bool on_device(hypre_ParVector *v) { return v->local_vector->memory_location == HYPRE_MEMORY_DEVICE; }

// y += alpha x, then <z, y> over all ranks: the fused launch and the reduction of hypre_ParVectorInnerProd
HYPRE_Real axpy_then_inner_prod(HYPRE_Complex alpha, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z)
{
   hypre_Vector *xl = x->local_vector, *yl = y->local_vector, *zl = z->local_vector;
   double *d_out = reduce_scratch(2048);
   launch_axpy_dot(alpha, xl->data, yl->data, zl->data, (size_t) yl->size * (size_t) yl->num_vectors, d_out, stream());
   double r = 0.0;
   dev_global_sums(y->comm, d_out, 1, &r);
   return r;
}

// the vector operations flexgmres_iterate asks for
struct ParOps
{
   hypre_amd_FlexGMRESData *d;
   hypre_ParCSRMatrix *A;
   void matvec(double alpha, hypre_ParVector *x, double beta, hypre_ParVector *y) { hypre_ParCSRMatrixMatvec(alpha, A, x, beta, y); }
   double inner(hypre_ParVector *x, hypre_ParVector *y) { return hypre_ParVectorInnerProd(x, y); }
   void copy(hypre_ParVector *x, hypre_ParVector *y) { hypre_ParVectorCopy(x, y); }
   void scale(double a, hypre_ParVector *y) { hypre_ParVectorScale(a, y); }
   void axpy(double a, hypre_ParVector *x, hypre_ParVector *y) { hypre_ParVectorAxpy(a, x, y); }
   double axpy_dot(double a, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z) { return axpy_then_inner_prod(a, x, y, z); }
   void mass_axpy(double *a, hypre_ParVector **xs, hypre_ParVector *y, int k) { hypre_ParVectorMassAxpy(a, xs, y, k, 0); }
   void precond(int iter, double rel_norm, hypre_ParVector *rhs, hypre_ParVector *sol)
   {
      hypre_ParVectorSetZeros(sol);        // ClearVector (flexgmres.c:549): all_zeros = 1
      if (d->modify_pc) { d->modify_pc(d->precond_data, iter, rel_norm); }
      if (d->precond) { d->precond(d->precond_data, A, rhs, sol); }
      else { hypre_ParVectorCopy(rhs, sol); }
   }
   void solution_changed(hypre_ParVector *x) { x->all_zeros = 0; }
};
}  // namespace

extern "C" {

HYPRE_Int HYPRE_ParCSRFlexGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   hypre_amd_FlexGMRESData *d = new hypre_amd_FlexGMRESData();
   memset(&d->base, 0, sizeof(d->base));
   d->comm = comm;
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRFlexGMRESDestroy(HYPRE_Solver solver)
{
   hypre_amd_FlexGMRESData *d = (hypre_amd_FlexGMRESData *) solver;
   if (!d) { return hypre_error_flag; }
   free_vectors(d);
   delete d;
   return hypre_error_flag;
}

HYPRE_Int HYPRE_FlexGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v)
{
   if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   ((hypre_amd_FlexGMRESData *) s)->prm.k_dim = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_FlexGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_FlexGMRESData *) s)->prm.tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_FlexGMRESData *) s)->prm.a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real v)
{
   (void) s;
   if (v != 0.0)
   {
      hypre_error_in_arg(2);
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_FlexGMRESSetConvergenceFactorTol: the convergence-factor stopping test is not built (0.0 only)");
   }
   return hypre_error_flag;
}
HYPRE_Int HYPRE_FlexGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_FlexGMRESData *) s)->prm.min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_FlexGMRESData *) s)->prm.max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                    HYPRE_Solver precond_solver)
{
   hypre_amd_FlexGMRESData *d = (hypre_amd_FlexGMRESData *) s;
   d->precond = precond; d->precond_setup = precond_setup; d->precond_data = precond_solver;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_FlexGMRESGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { *precond_data_ptr = ((hypre_amd_FlexGMRESData *) s)->precond_data; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetModifyPC(HYPRE_Solver s, HYPRE_PtrToModifyPCFcn modify_pc) { ((hypre_amd_FlexGMRESData *) s)->modify_pc = modify_pc; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }       // accepted, inert
HYPRE_Int HYPRE_FlexGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_FlexGMRESData *) s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = ((hypre_amd_FlexGMRESData *) s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_FlexGMRESData *) s)->converged; return hypre_error_flag; }

HYPRE_Int hypre_amd_FlexGMRESSetFusedOrthogonalization(HYPRE_Solver s, HYPRE_Int on)
{
   if (on != 0 && on != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   ((hypre_amd_FlexGMRESData *) s)->prm.fused = on;
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_FlexGMRESGetLaunchStats(HYPRE_Solver s, HYPRE_Int *fused_steps, HYPRE_Int *plain_dots, HYPRE_Int *plain_axpys)
{
   hypre_amd_FlexGMRESData *d = (hypre_amd_FlexGMRESData *) s;
   if (fused_steps) { *fused_steps = d->fused_steps; }
   if (plain_dots) { *plain_dots = d->plain_dots; }
   if (plain_axpys) { *plain_axpys = d->plain_axpys; }
   return hypre_error_flag;
}

HYPRE_Int hypre_amd_ParVectorAxpyThenInnerProd(HYPRE_Complex alpha, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z,
                                               HYPRE_Real *result)
{
   if (!on_device(x) || !on_device(y) || !on_device(z))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorAxpyThenInnerProd: operand is not in device memory; host execution is not part of this library");
      return hypre_error_flag;
   }
   const size_t n = (size_t) y->local_vector->size * (size_t) y->local_vector->num_vectors;
   if ((size_t) x->local_vector->size * (size_t) x->local_vector->num_vectors != n ||
       (size_t) z->local_vector->size * (size_t) z->local_vector->num_vectors != n)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorAxpyThenInnerProd: the three vectors differ in length");
      return hypre_error_flag;
   }
   *result = axpy_then_inner_prod(alpha, x, y, z);
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRFlexGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_FlexGMRESData *d = (hypre_amd_FlexGMRESData *) solver;
   free_vectors(d);
   const HYPRE_MemoryLocation loc = x->local_vector->memory_location;
   // work vectors shaped like x (flexgmres.c:230-250 CreateVector / CreateVectorArray): the columns of a multivector x
   const HYPRE_Int nv = x->local_vector->num_vectors;
   auto mk = [&]() { hypre_ParVector *v = hypre_ParMultiVectorCreate(A->comm, A->global_num_rows, A->row_starts, nv); hypre_ParVectorInitialize_v2(v, loc); return v; };
   d->r = mk(); d->w = mk();
   for (HYPRE_Int i = 0; i <= d->prm.k_dim; i++) { d->p.push_back(mk()); d->pre_vecs.push_back(mk()); }
   if (d->precond_setup) { d->precond_setup(d->precond_data, A, b, x); }
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRFlexGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_FlexGMRESData *d = (hypre_amd_FlexGMRESData *) solver;
   if ((HYPRE_Int) d->p.size() != d->prm.k_dim + 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRFlexGMRESSolve: call HYPRE_ParCSRFlexGMRESSetup after HYPRE_FlexGMRESSetKDim");
      return hypre_error_flag;
   }
   if (!on_device(b) || !on_device(x) || !on_device(d->r))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRFlexGMRESSolve: operand is not in device memory; host execution is not part of this library");
      return hypre_error_flag;
   }
   d->converged = 0;
   d->fused_steps = d->plain_dots = d->plain_axpys = 0;
   const int saved_sync = handle().sync_compute;
   handle().sync_compute = 0;
   verify_par_plans(A);                    // a solve never starts from a plan its matrix has moved away from
   ParOps ops{d, A};
   const FlexGMRESResult res = flexgmres_iterate<hypre_ParVector *>(d->prm, ops, b, x, d->r, d->w, d->p.data(), d->pre_vecs.data());
   d->num_iterations = res.iterations;
   d->converged = res.converged;
   if (res.norm_set) { d->rel_residual_norm = res.rel_residual_norm; }
   d->fused_steps = (HYPRE_Int) res.fused_steps; d->plain_dots = (HYPRE_Int) res.plain_dots; d->plain_axpys = (HYPRE_Int) res.plain_axpys;
   if (res.status == FLEXGMRES_NOT_A_NUMBER) { hypre_error(HYPRE_ERROR_GENERIC); }
   if (res.status == FLEXGMRES_NOT_CONVERGED) { hypre_error(HYPRE_ERROR_CONV); }
   handle().sync_compute = saved_sync;
   maybe_sync();
   return hypre_error_flag;
}

// the spellings of parcsr_ls/HYPRE_parcsr_flexgmres.c and the generic Setup / Solve of krylov/HYPRE_flexgmres.c
HYPRE_Int HYPRE_FlexGMRESSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return HYPRE_ParCSRFlexGMRESSetup(s, A, b, x); }
HYPRE_Int HYPRE_FlexGMRESSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return HYPRE_ParCSRFlexGMRESSolve(s, A, b, x); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_FlexGMRESSetKDim(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { return HYPRE_FlexGMRESSetTol(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { return HYPRE_FlexGMRESSetAbsoluteTol(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_FlexGMRESSetMinIter(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_FlexGMRESSetMaxIter(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                          HYPRE_Solver precond_solver)
{ return HYPRE_FlexGMRESSetPrecond(s, precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_ParCSRFlexGMRESGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { return HYPRE_FlexGMRESGetPrecond(s, precond_data_ptr); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetModifyPC(HYPRE_Solver s, HYPRE_PtrToModifyPCFcn modify_pc) { return HYPRE_FlexGMRESSetModifyPC(s, modify_pc); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_FlexGMRESSetLogging(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_FlexGMRESSetPrintLevel(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { return HYPRE_FlexGMRESGetNumIterations(s, v); }
HYPRE_Int HYPRE_ParCSRFlexGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { return HYPRE_FlexGMRESGetFinalRelativeResidualNorm(s, v); }

}  // extern "C"
