// hypre_amd — preconditioned conjugate gradients on ParVectors on the device: HYPRE_ParCSRPCG* / HYPRE_PCG*
// (krylov/pcg.c:318-1000 with the defaults flex = rel_change = 0, recompute_residual = 0, stop_crit = 0, atolf = 0;
// parcsr_ls/HYPRE_parcsr_pcg.c).  An iteration is one SpMV, one fused update of x and r that leaves <r, r>
// on the device, the preconditioner, one dot and ONE all-reduce of two values with one read-back.
//
// Behind HYPRE_ParCSRDiagScale on vectors of one column the update, the scaling and the dot are one launch
// (launch_dscg_step, mass_kernels.hip) over a copy of the diagonal that Setup packs: 64 bytes per element where the three
// move 92 (48 + 28 + 16, the 28 being r, the 4-byte row pointer, the gathered diagonal and s), the same bits.
// hypre_amd_PCGSetFusedDiagScale switches it (on by default); the packed diagonal is that of the matrix Setup saw, so
// an application that changes the values calls Setup again, as it does for any preconditioner.
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
   HYPRE_Real cf_tol = 0.0;      // pcg.c:893-950: give up when the weighted average convergence factor exceeds it (0: never)
   HYPRE_Int hybrid = 0;         // -1: the diagonally scaled phase of the hybrid solver (hypre_PCGSetHybrid)
   // the fused step of diagonally scaled CG: the switch, whether Setup found its conditions met, the packed diagonal
   // and the block it was packed from
   HYPRE_Int fused_ds = 1, fused_ds_used = 0;      // on: measured faster than the three launches
   double *d_diag = nullptr;
   size_t diag_rows = 0;
   const hypre_CSRMatrix *diag_of = nullptr;
   const HYPRE_Complex *diag_values = nullptr;
};

}  // extern "C"

namespace {
void drop_packed_diagonal(hypre_amd_PCGData *d)
{
   if (d->d_diag) { hypre_Free(d->d_diag, HYPRE_MEMORY_DEVICE); }
   d->d_diag = nullptr; d->diag_rows = 0; d->diag_of = nullptr; d->diag_values = nullptr; d->fused_ds_used = 0;
}

// the diagonal of A's local block, one double per row, on the device; false when a row has no entry (the plain scaling
// is then the caller's business, not ours)
bool pack_diagonal(hypre_CSRMatrix *diag, double *d_diag)
{
   int *d_flag = hypre_TAlloc(int, 1, HYPRE_MEMORY_DEVICE);
   int flag = 0;
   hypre_TMemcpy(d_flag, &flag, int, 1, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
   launch_pack_first_entries(diag->i, diag->data, d_diag, (size_t) diag->num_rows, d_flag, stream());
   hypre_TMemcpy(&flag, d_flag, int, 1, HYPRE_MEMORY_HOST, HYPRE_MEMORY_DEVICE);
   hypre_Free(d_flag, HYPRE_MEMORY_DEVICE);
   return flag == 0;
}
}  // namespace

extern "C" {

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
   drop_packed_diagonal(d);
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
HYPRE_Int HYPRE_PCGSetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_PCGData *) s)->cf_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_PCGGetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real *v) { *v = ((hypre_amd_PCGData *) s)->cf_tol; return hypre_error_flag; }
// pcg.c:841: set where the tolerance test passes, not at the convergence-factor exit, a breakdown or max_iter
HYPRE_Int HYPRE_PCGGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_PCGData *) s)->converged; return hypre_error_flag; }
HYPRE_Int hypre_PCGSetHybrid(HYPRE_Solver s, HYPRE_Int level) { ((hypre_amd_PCGData *) s)->hybrid = level; return hypre_error_flag; }
// one launch for update, diagonal scaling and dot behind HYPRE_ParCSRDiagScale (before Setup); the getter says, after Setup,
// whether the solves of this Setup take it
HYPRE_Int hypre_amd_PCGSetFusedDiagScale(HYPRE_Solver s, HYPRE_Int on)
{
   if (on != 0 && on != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   ((hypre_amd_PCGData *) s)->fused_ds = on;
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_PCGGetFusedDiagScaleUsed(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_PCGData *) s)->fused_ds_used; return hypre_error_flag; }
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
   // the fused step: diagonal scaling, one column, everything on the device, every row with a first entry
   drop_packed_diagonal(d);
   hypre_CSRMatrix *diag = A->diag;
   const hypre_Vector *xl = x->local_vector;
   if (d->fused_ds && d->pc.solve == (HYPRE_PtrToSolverFcn) HYPRE_ParCSRDiagScale && xl->num_vectors == 1 &&
       xl->memory_location == HYPRE_MEMORY_DEVICE && diag->memory_location == HYPRE_MEMORY_DEVICE && diag->num_rows == xl->size &&
       diag->num_rows > 0)
   {
      d->d_diag = hypre_TAlloc(double, (size_t) diag->num_rows, HYPRE_MEMORY_DEVICE);
      if (pack_diagonal(diag, d->d_diag))
      {
         d->diag_rows = (size_t) diag->num_rows; d->diag_of = diag; d->diag_values = diag->data;
         d->fused_ds_used = 1;
      }
      else { drop_packed_diagonal(d); }
   }
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRPCGSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_PCGData *d = (hypre_amd_PCGData *) solver;
   hypre_ParVector *p = d->p, *s = d->s, *r = d->r;
   const HYPRE_Real r_tol = d->tol, a_tol = d->a_tol;
   HYPRE_Real alpha, beta, gamma, gamma_old, bi_prod, eps, sdotp, i_prod = 0.0, i_prod_0 = 0.0, delta = 0.0, cf_ave_0 = 0.0, cf_ave_1 = 0.0;
   const HYPRE_Real cf_tol = d->cf_tol;
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
   // the fused step of Setup, for the matrix and the vectors Setup saw
   const bool fused_ds = d->fused_ds_used && nvec == 1 && A->diag == d->diag_of && A->diag->data == d->diag_values && vec_len == d->diag_rows &&
                         d->pc.solve == (HYPRE_PtrToSolverFcn) HYPRE_ParCSRDiagScale;
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
      if (fused_ds)
      {
         // the update, s = r ./ diag(A) and both sums in one pass
         launch_dscg_step(alpha, -alpha, p->local_vector->data, d->d_diag, s->local_vector->data, x->local_vector->data,
                          r->local_vector->data, vec_len, d_rr, stream());
         x->all_zeros = 0; r->all_zeros = 0; s->all_zeros = 0;
      }
      else
      {
         launch_pcg_update(alpha, -alpha, p->local_vector->data, s->local_vector->data, x->local_vector->data,
                           r->local_vector->data, vec_len, d_rr, stream());
         x->all_zeros = 0; r->all_zeros = 0;
         precond(r, s);
         // gamma = <r, s> and, for the two-norm test, <r, r> (left on the device by the fused update): ONE all-reduce of
         // two values and one read-back per iteration (pcg.c:716-760 reduces them separately)
         launch_dot(r->local_vector->data, s->local_vector->data, vec_len, d_rr + 1, stream());
      }
      {
         double sums[2];
         dev_global_sums(r->comm, d_rr, 2, sums);
         gamma = sums[1];
         i_prod = d->two_norm ? sums[0] : gamma;
      }
      if (d->flex) { delta = gamma - hypre_ParVectorInnerProd(d->r_old, s); }      // pcg.c:720-723
      if (i_prod / bi_prod < eps) { d->converged = 1; break; }
      if (gamma <= 0.0) { hypre_error_w_msg(HYPRE_ERROR_CONV, "Negative or zero gamma value in PCG"); break; }
      // pcg.c:893-950: is adequate progress being made?  Both numbers were read back above.
      if (cf_tol > 0.0)
      {
         cf_ave_0 = cf_ave_1;
         if (i_prod_0 <= 0.0) { hypre_error_w_msg(HYPRE_ERROR_CONV, "Negative or zero i_prod_0 value in PCG"); break; }
         cf_ave_1 = std::pow(i_prod / i_prod_0, 1.0 / (2.0 * i));
         if (convergence_factor_exceeds(cf_ave_1, cf_ave_0, cf_tol)) { break; }
      }
      beta = (d->flex ? delta : gamma) / gamma_old;                 // pcg.c:957-965
      // p = beta p + s in one pass (Scale then Axpy in the reference)
      launch_pcg_direction(beta, s->local_vector->data, p->local_vector->data, vec_len, stream());
   }
   if (i >= d->max_iter && (i_prod / bi_prod) >= eps && eps > 0 && d->hybrid != -1)
   {
      hypre_error_w_msg(HYPRE_ERROR_CONV, "Reached max iterations in PCG before convergence");
   }
   d->num_iterations = i;
   d->rel_residual_norm = std::sqrt(i_prod / bi_prod);
   quiet.restore();
   maybe_sync();
   return hypre_error_flag;
}

// The vector work of one diagonally scaled CG iteration on its own, s holding A p on entry: x += alpha p, r -= alpha s,
// s = r ./ diag(A), *rr = <r, r>, *rs = <r, s> over all ranks.  fused = 1: the diagonal is packed and launch_dscg_step
// runs; fused = 0: launch_pcg_update, hypre_ParCSRDiagScaleVector and launch_dot, the three it stands for.  The same
// bits either way.  Every row of A's local block needs a first entry.
HYPRE_Int hypre_amd_ParVectorDiagScaledCGStep(HYPRE_Int fused, HYPRE_Complex alpha, hypre_ParCSRMatrix *A, hypre_ParVector *p, hypre_ParVector *s,
                                              hypre_ParVector *x, hypre_ParVector *r, HYPRE_Real *rr, HYPRE_Real *rs)
{
   hypre_CSRMatrix *diag = A->diag;
   const size_t n = (size_t) diag->num_rows;
   for (hypre_ParVector *v : {p, s, x, r})
   {
      const hypre_Vector *l = v->local_vector;
      if (l->memory_location != HYPRE_MEMORY_DEVICE || diag->memory_location != HYPRE_MEMORY_DEVICE)
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorDiagScaledCGStep: operand is not in device memory; host execution is not part of this library");
         return hypre_error_flag;
      }
      if (l->num_vectors != 1 || (size_t) l->size != n)
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorDiagScaledCGStep: the vectors have one column of as many rows as A's local block");
         return hypre_error_flag;
      }
      int seen = 0;
      for (hypre_ParVector *w : {p, s, x, r}) { seen += w == v || w->local_vector->data == l->data; }
      if (seen != 1 && n > 0)
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorDiagScaledCGStep: p, s, x and r must be distinct");
         return hypre_error_flag;
      }
   }
   double *d_out = hypre_TAlloc(double, 2, HYPRE_MEMORY_DEVICE);
   if (fused)
   {
      double *d_diag = hypre_TAlloc(double, std::max<size_t>(n, 1), HYPRE_MEMORY_DEVICE);
      if (!pack_diagonal(diag, d_diag))
      {
         hypre_Free(d_diag, HYPRE_MEMORY_DEVICE); hypre_Free(d_out, HYPRE_MEMORY_DEVICE);
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorDiagScaledCGStep: a row of A has no entry");
         return hypre_error_flag;
      }
      launch_dscg_step(alpha, -alpha, p->local_vector->data, d_diag, s->local_vector->data, x->local_vector->data, r->local_vector->data, n,
                       d_out, stream());
      x->all_zeros = 0; r->all_zeros = 0; s->all_zeros = 0;
      double sums[2];
      dev_global_sums(r->comm, d_out, 2, sums);          // reads back: the kernel is done with d_diag
      *rr = sums[0]; *rs = sums[1];
      hypre_Free(d_diag, HYPRE_MEMORY_DEVICE);
   }
   else
   {
      launch_pcg_update(alpha, -alpha, p->local_vector->data, s->local_vector->data, x->local_vector->data, r->local_vector->data, n, d_out,
                        stream());
      x->all_zeros = 0; r->all_zeros = 0;
      hypre_ParVectorSetZeros(s);
      hypre_ParCSRDiagScaleVector(A, r, s);
      launch_dot(r->local_vector->data, s->local_vector->data, n, d_out + 1, stream());
      double sums[2];
      dev_global_sums(r->comm, d_out, 2, sums);
      *rr = sums[0]; *rs = sums[1];
   }
   hypre_Free(d_out, HYPRE_MEMORY_DEVICE);
   maybe_sync();
   return hypre_error_flag;
}
// the elements one pass of the grid of launch_dscg_step covers (that of a dot product): a longer vector takes a second trip
HYPRE_BigInt hypre_amd_DotGridPassElements(void) { return (HYPRE_BigInt) dot_grid_pass_elements(); }

}  // extern "C"
