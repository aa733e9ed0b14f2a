// hypre_amd — preconditioned conjugate gradients on ParVectors on the device: HYPRE_ParCSRPCG* / HYPRE_PCG*
// (krylov/pcg.c:318-1000 with the defaults flex = rel_change = 0, recompute_residual = 0, stop_crit = 0, atolf = 0,
// cf_tol = 0; parcsr_ls/HYPRE_parcsr_pcg.c).  An iteration is one SpMV, one fused update of x and r that leaves <r, r>
// on the device, the preconditioner, one dot and ONE all-reduce of two values with one read-back.
#include "krylov_common.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace hamd;

extern "C" {

struct hypre_amd_PCGData
{
   hypre_Solver base;
   MPI_Comm comm;
   HYPRE_Real tol = 1e-6, a_tol = 0.0;
   HYPRE_Int max_iter = 1000, two_norm = 0, flex = 0;
   KrylovPrecond pc;
   hypre_ParVector *p = nullptr, *s = nullptr, *r = nullptr, *r_old = nullptr;
   double *d_rr = nullptr;       // device scalar of this solver: <r,r> of the fused update survives the preconditioner call
                                 // (which may itself run a PCG: the CG smoother)
   HYPRE_Int num_iterations = 0, converged = 0;
   HYPRE_Real rel_residual_norm = 0.0;
};

HYPRE_Int HYPRE_ParCSRPCGCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   hypre_amd_PCGData *d = new hypre_amd_PCGData();
   memset(&d->base, 0, sizeof(d->base));
   d->comm = comm;
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRPCGDestroy(HYPRE_Solver solver)
{
   hypre_amd_PCGData *d = (hypre_amd_PCGData *) solver;
   if (!d) { return hypre_error_flag; }
   hypre_ParVectorDestroy(d->p); hypre_ParVectorDestroy(d->s); hypre_ParVectorDestroy(d->r); hypre_ParVectorDestroy(d->r_old);
   if (d->d_rr) { hypre_Free(d->d_rr, HYPRE_MEMORY_DEVICE); }
   delete d;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_PCGSetTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_PCGData *) s)->tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_PCGData *) s)->a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_PCGData *) s)->max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGSetTwoNorm(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_PCGData *) s)->two_norm = v; return hypre_error_flag; }
// pcg.c:339-345: Polak-Ribiere beta instead of Fletcher-Reeves, for preconditioners that change between iterations
HYPRE_Int HYPRE_PCGSetFlex(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_PCGData *) s)->flex = v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                              HYPRE_Solver precond_solver)
{ return ((hypre_amd_PCGData *) s)->pc.set(precond, precond_setup, precond_solver); }
// options of krylov/HYPRE_pcg.c an application sets routinely: logging and printing are accepted and inert (this PCG
// keeps no residual history and prints nothing); the relative-change and recomputed-residual variants are not built
HYPRE_Int HYPRE_PCGSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGSetRelChange(HYPRE_Solver s, HYPRE_Int v)
{
   (void) s;
   if (v != 0) { hypre_error_in_arg(2); hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_PCGSetRelChange: the relative-change stopping test is not built (0 only)"); }
   return hypre_error_flag;
}
HYPRE_Int HYPRE_PCGSetRecomputeResidual(HYPRE_Solver s, HYPRE_Int v)
{
   (void) s;
   if (v != 0) { hypre_error_in_arg(2); hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_PCGSetRecomputeResidual: 0 only"); }
   return hypre_error_flag;
}
HYPRE_Int HYPRE_PCGGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_PCGData *) s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = ((hypre_amd_PCGData *) s)->rel_residual_norm; return hypre_error_flag; }

HYPRE_Int HYPRE_ParCSRPCGSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_PCGData *d = (hypre_amd_PCGData *) solver;
   hypre_ParVectorDestroy(d->p); hypre_ParVectorDestroy(d->s); hypre_ParVectorDestroy(d->r); hypre_ParVectorDestroy(d->r_old);
   d->p = par_vector_like(A, x); d->s = par_vector_like(A, x); d->r = par_vector_like(A, x);
   d->r_old = d->flex ? par_vector_like(A, x) : nullptr;
   if (!d->d_rr && x->local_vector->memory_location == HYPRE_MEMORY_DEVICE) { d->d_rr = hypre_TAlloc(double, 2, HYPRE_MEMORY_DEVICE); }
   if (d->pc.setup) { d->pc.setup(d->pc.data, A, b, x); }
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRPCGSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_PCGData *d = (hypre_amd_PCGData *) solver;
   hypre_ParVector *p = d->p, *s = d->s, *r = d->r;
   const HYPRE_Real r_tol = d->tol, a_tol = d->a_tol;
   HYPRE_Real alpha, beta, gamma, gamma_old, bi_prod, eps, sdotp, i_prod = 0.0, i_prod_0 = 0.0, delta = 0.0;
   HYPRE_Int i = 0;
   d->converged = 0;
   if (d->flex && !d->r_old)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRPCGSolve: call HYPRE_ParCSRPCGSetup after HYPRE_PCGSetFlex");
      return hypre_error_flag;
   }
   // multivectors (`ij -nc N`, test/TEST_ij/vector.jobs): the reference's PCG works on whatever its vector functions take,
   // and hypre_ParVector's take every column — one Krylov iteration over the columns together.  The fused updates below
   // run over the columns' common storage, which has to be one piece.
   const HYPRE_Int nvec = x->local_vector->num_vectors;
   for (hypre_ParVector *v : {b, x, p, s, r})
   {
      const hypre_Vector *l = v->local_vector;
      if (l->num_vectors != nvec || (nvec > 1 && (l->idxstride != 1 || l->vecstride != l->size)))
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRPCGSolve: b, x and the work vectors of HYPRE_ParCSRPCGSetup must have the same number of "
                                                "columns, stored one after the other");
         return hypre_error_flag;
      }
   }
   const size_t vec_len = (size_t) r->local_vector->size * (size_t) nvec;
   QuietSolve quiet(A);
   auto precond = [&](hypre_ParVector *rhs, hypre_ParVector *sol) { d->pc.apply(A, rhs, sol); };
   if (d->two_norm) { bi_prod = hypre_ParVectorInnerProd(b, b); }
   else { precond(b, p); bi_prod = hypre_ParVectorInnerProd(p, b); }
   HYPRE_Real ieee_check = 0.;
   if (bi_prod != 0.) { ieee_check = bi_prod / bi_prod; }
   if (ieee_check != ieee_check) { hypre_error(HYPRE_ERROR_GENERIC); return hypre_error_flag; }
   eps = r_tol * r_tol;
   if (bi_prod > 0.0) { eps = std::max(r_tol * r_tol, a_tol * a_tol / bi_prod); }
   else
   {
      hypre_ParVectorCopy(b, x);
      d->num_iterations = 0; d->rel_residual_norm = 0.0;
      return hypre_error_flag;
   }
   hypre_ParVectorCopy(b, r);
   hypre_ParCSRMatrixMatvec(-1.0, A, x, 1.0, r);
   precond(r, p);
   gamma = hypre_ParVectorInnerProd(r, p);
   if (gamma != 0.) { ieee_check = gamma / gamma; }
   if (ieee_check != ieee_check) { hypre_error(HYPRE_ERROR_GENERIC); return hypre_error_flag; }
   i_prod_0 = d->two_norm ? hypre_ParVectorInnerProd(r, r) : gamma;
   while ((i + 1) <= d->max_iter)
   {
      i++;
      hypre_ParCSRMatrixMatvec(1.0, A, p, 0.0, s);
      sdotp = hypre_ParVectorInnerProd(s, p);
      if (sdotp == 0.0) { hypre_error_w_msg(HYPRE_ERROR_CONV, "Zero sdotp value in PCG"); if (i == 1) { i_prod = i_prod_0; } break; }
      alpha = gamma / sdotp;
      if (alpha <= 0.0) { hypre_error_w_msg(HYPRE_ERROR_CONV, "Negative or zero alpha value in PCG"); if (i == 1) { i_prod = i_prod_0; } break; }
      gamma_old = gamma;
      // x += alpha p ; r -= alpha s ; <r,r> of the new residual: one pass (pcg.c:716-760 makes
      // three vector calls of it; element values and the norm's summation order are unchanged)
      if (d->flex) { hypre_ParVectorCopy(r, d->r_old); }          // pcg.c:636-639
      double *d_rr = d->d_rr;
      launch_pcg_update(alpha, -alpha, p->local_vector->data, s->local_vector->data, x->local_vector->data,
                        r->local_vector->data, vec_len, d_rr, stream());
      x->all_zeros = 0; r->all_zeros = 0;
      precond(r, s);
      // gamma = <r, s> and, for the two-norm test, <r, r> (left on the device by the fused update): ONE all-reduce of
      // two values and one read-back per iteration (pcg.c:716-760 reduces them separately)
      launch_dot(r->local_vector->data, s->local_vector->data, vec_len, d_rr + 1, stream());
      {
         double sums[2];
         dev_global_sums(r->comm, d_rr, 2, sums);
         gamma = sums[1];
         i_prod = d->two_norm ? sums[0] : gamma;
      }
      if (d->flex) { delta = gamma - hypre_ParVectorInnerProd(d->r_old, s); }      // pcg.c:720-723
      if (i_prod / bi_prod < eps) { d->converged = 1; break; }
      if (gamma <= 0.0) { hypre_error_w_msg(HYPRE_ERROR_CONV, "Negative or zero gamma value in PCG"); break; }
      beta = (d->flex ? delta : gamma) / gamma_old;                 // pcg.c:957-965
      // p = beta p + s in one pass (Scale then Axpy in the reference)
      launch_pcg_direction(beta, s->local_vector->data, p->local_vector->data, vec_len, stream());
   }
   if (i >= d->max_iter && (i_prod / bi_prod) >= eps && eps > 0)
   {
      hypre_error_w_msg(HYPRE_ERROR_CONV, "Reached max iterations in PCG before convergence");
   }
   d->num_iterations = i;
   d->rel_residual_norm = std::sqrt(i_prod / bi_prod);
   quiet.restore();
   maybe_sync();
   return hypre_error_flag;
}

}  // extern "C"
