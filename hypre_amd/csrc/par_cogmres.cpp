// hypre_amd — COGMRES: right-preconditioned restarted GMRES whose orthogonalisation is batched, the third Krylov caller
// (`ij -solver 16 | 17`).
//
// Reference: krylov/cogmres.c:274-900 (hypre_COGMRESSolve) with parcsr_ls/HYPRE_parcsr_cogmres.c and
// krylov/HYPRE_cogmres.c for the entry points; defaults of hypre_COGMRESCreate (cogmres.c:85-111): k_dim 5, cgs 1,
// unroll 0, tol 1e-6, a_tol 0, min_iter 0, max_iter 1000, skip_real_r_check 0.
// Step i of a restart cycle orthogonalises the new direction against all i basis vectors at once: classical
// Gram-Schmidt from one MassInnerProd and one MassAxpy (cgs 1), or MassDotpTwo and the correction of cogmres.c:550-566
// that reorthogonalises with the products of the previous direction (cgs 2).  Either way the step reads every basis
// vector twice and ends in two read-backs (the batch and the norm) where modified Gram-Schmidt (par_gmres.cpp) needs
// i + 1.  The Hessenberg matrix is stored column-wise, hh[(i-1)(k_dim+1) + j]; Givens rotations on the host; the true
// residual is recomputed before convergence is accepted; the relative-change and convergence-factor exits of the
// reference (rel_change, cf_tol) are not carried.
#include "amg_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace hamd;

struct hypre_amd_COGMRESData
{
   hypre_Solver base;
   MPI_Comm comm;
   HYPRE_Int k_dim = 5, cgs = 1, unroll = 0, min_iter = 0, max_iter = 1000, skip_real_r_check = 0;
   HYPRE_Real tol = 1e-6, a_tol = 0.0;
   HYPRE_PtrToSolverFcn precond = nullptr, precond_setup = nullptr;
   HYPRE_Solver precond_data = nullptr;
   hypre_ParVector *r = nullptr, *w = nullptr;
   std::vector<hypre_ParVector *> p;
   HYPRE_Int num_iterations = 0, converged = 0;
   HYPRE_Real rel_residual_norm = 0.0;
};

namespace {
void free_vectors(hypre_amd_COGMRESData *d)
{
   hypre_ParVectorDestroy(d->r); hypre_ParVectorDestroy(d->w);
   d->r = d->w = nullptr;
   for (hypre_ParVector *v : d->p) { hypre_ParVectorDestroy(v); }
   d->p.clear();
}
}  // namespace

extern "C" {

HYPRE_Int HYPRE_ParCSRCOGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   hypre_amd_COGMRESData *d = new hypre_amd_COGMRESData();
   memset(&d->base, 0, sizeof(d->base));
   d->comm = comm;
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRCOGMRESDestroy(HYPRE_Solver solver)
{
   hypre_amd_COGMRESData *d = (hypre_amd_COGMRESData *) solver;
   if (!d) { return hypre_error_flag; }
   free_vectors(d);
   delete d;
   return hypre_error_flag;
}

HYPRE_Int HYPRE_COGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v)
{
   if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   ((hypre_amd_COGMRESData *) s)->k_dim = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_COGMRESSetUnroll(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_COGMRESData *) s)->unroll = v; return hypre_error_flag; }   // handed on, ignored by the kernels
HYPRE_Int HYPRE_COGMRESSetCGS(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_COGMRESData *) s)->cgs = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_COGMRESData *) s)->tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { ((hypre_amd_COGMRESData *) s)->a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_COGMRESData *) s)->min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_COGMRESData *) s)->max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetSkipRealResidualCheck(HYPRE_Solver s, HYPRE_Int v) { ((hypre_amd_COGMRESData *) s)->skip_real_r_check = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                  HYPRE_Solver precond_solver)
{
   hypre_amd_COGMRESData *d = (hypre_amd_COGMRESData *) s;
   d->precond = precond; d->precond_setup = precond_setup; d->precond_data = precond_solver;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_COGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }       // accepted, inert
HYPRE_Int HYPRE_COGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_COGMRESData *) s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = ((hypre_amd_COGMRESData *) s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = ((hypre_amd_COGMRESData *) s)->converged; return hypre_error_flag; }

HYPRE_Int HYPRE_ParCSRCOGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_COGMRESData *d = (hypre_amd_COGMRESData *) solver;
   free_vectors(d);
   if (x->local_vector->num_vectors > 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRCOGMRESSetup: multivectors are not served by COGMRES (use HYPRE_ParCSRGMRES)");
      return hypre_error_flag;
   }
   const HYPRE_MemoryLocation loc = x->local_vector->memory_location;
   // work vectors shaped like x (cogmres.c:220-231 CreateVectorArray / CreateVector)
   auto mk = [&]() { hypre_ParVector *v = hypre_ParVectorCreate(A->comm, A->global_num_rows, A->row_starts); hypre_ParVectorInitialize_v2(v, loc); return v; };
   d->r = mk(); d->w = mk();
   for (HYPRE_Int i = 0; i <= d->k_dim; i++) { d->p.push_back(mk()); }
   if (d->precond_setup) { d->precond_setup(d->precond_data, A, b, x); }
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRCOGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_COGMRESData *d = (hypre_amd_COGMRESData *) solver;
   if ((HYPRE_Int) d->p.size() != d->k_dim + 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRCOGMRESSolve: call HYPRE_ParCSRCOGMRESSetup after HYPRE_COGMRESSetKDim");
      return hypre_error_flag;
   }
   const HYPRE_Int k_dim = d->k_dim, unroll = d->unroll, cgs = d->cgs, min_iter = d->min_iter, max_iter = d->max_iter;
   hypre_ParVector *r = d->r, *w = d->w;
   hypre_ParVector **p = d->p.data();
   const HYPRE_Real epsmac = 1.e-16;
   const size_t ld = (size_t) k_dim + 1;           // a column of the Hessenberg matrix
   std::vector<HYPRE_Real> rs_v(ld, 0.0), c_v((size_t) k_dim, 0.0), s_v((size_t) k_dim, 0.0), rv_v(ld, 0.0);
   std::vector<HYPRE_Real> hh_v(ld * (size_t) k_dim, 0.0), uu_v(ld * (size_t) k_dim, 0.0);
   HYPRE_Real *rs = rs_v.data(), *c = c_v.data(), *s = s_v.data(), *rv = rv_v.data(), *hh = hh_v.data(), *uu = uu_v.data();
   HYPRE_Int i = 0, j, k, iter = 0;
   size_t itmp = 0;
   HYPRE_Real t, gamma, r_norm, b_norm, den_norm, epsilon, ieee_check = 0., real_r_norm_old, real_r_norm_new;
   d->converged = 0;
   const int saved_sync = handle().sync_compute;
   handle().sync_compute = 0;
   verify_par_plans(A);                    // a solve never starts from a plan its matrix has moved away from
   auto leave = [&]() { handle().sync_compute = saved_sync; maybe_sync(); return hypre_error_flag; };
   auto precond = [&](hypre_ParVector *rhs, hypre_ParVector *sol)
   {
      hypre_ParVectorSetZeros(sol);       // ClearVector (cogmres.c:541)
      if (d->precond) { d->precond(d->precond_data, A, rhs, sol); }
      else { hypre_ParVectorCopy(rhs, sol); }
   };
   auto norm = [&](hypre_ParVector *v) { return std::sqrt(hypre_ParVectorInnerProd(v, v)); };

   hypre_ParVectorCopy(b, p[0]);
   hypre_ParCSRMatrixMatvec(-1.0, A, x, 1.0, p[0]);
   b_norm = norm(b);
   real_r_norm_old = b_norm;
   if (b_norm != 0.) { ieee_check = b_norm / b_norm; }
   if (ieee_check != ieee_check) { hypre_error(HYPRE_ERROR_GENERIC); return leave(); }
   r_norm = norm(p[0]);
   if (r_norm != 0.) { ieee_check = r_norm / r_norm; }
   if (ieee_check != ieee_check) { hypre_error(HYPRE_ERROR_GENERIC); return leave(); }
   den_norm = (b_norm > 0.0) ? b_norm : r_norm;
   epsilon = std::max(d->a_tol, d->tol * den_norm);

   while (iter < max_iter)
   {
      rs[0] = r_norm;
      if (r_norm == 0.0) { return leave(); }  // cogmres.c:488-500 returns here, counters untouched
      if (r_norm <= epsilon && iter >= min_iter)
      {
         hypre_ParVectorCopy(b, r);
         hypre_ParCSRMatrixMatvec(-1.0, A, x, 1.0, r);
         r_norm = norm(r);
         if (r_norm <= epsilon) { break; }
      }
      t = 1.0 / r_norm;
      hypre_ParVectorScale(t, p[0]);
      i = 0;
      while (i < k_dim && iter < max_iter)
      {
         i++;
         iter++;
         itmp = (size_t) (i - 1) * ld;
         precond(p[i - 1], r);
         hypre_ParCSRMatrixMatvec(1.0, A, r, 0.0, p[i]);
         for (j = 0; j < i; j++) { rv[j] = 0; }
         if (cgs > 1)
         {
            hypre_ParVectorMassDotpTwo(p[i], p[i - 1], p, i, unroll, &hh[itmp], &uu[itmp]);
            for (j = 0; j < i - 1; j++) { uu[(size_t) j * ld + (size_t) i - 1] = uu[itmp + (size_t) j]; }
            for (j = 0; j < i; j++) { rv[j] = hh[itmp + (size_t) j]; }
            for (k = 0; k < i; k++)
            {
               for (j = 0; j < i; j++) { hh[itmp + (size_t) j] -= (uu[(size_t) k * ld + (size_t) j] * rv[j]); }
            }
            for (j = 0; j < i; j++) { hh[itmp + (size_t) j] = -rv[j] - hh[itmp + (size_t) j]; }
         }
         else
         {
            hypre_ParVectorMassInnerProd(p[i], p, i, unroll, &hh[itmp]);
            for (j = 0; j < i; j++) { hh[itmp + (size_t) j] = -hh[itmp + (size_t) j]; }
         }
         hypre_ParVectorMassAxpy(&hh[itmp], p, p[i], i, unroll);
         for (j = 0; j < i; j++) { hh[itmp + (size_t) j] = -hh[itmp + (size_t) j]; }
         t = norm(p[i]);
         hh[itmp + (size_t) i] = t;
         if (hh[itmp + (size_t) i] != 0.0) { t = 1.0 / t; hypre_ParVectorScale(t, p[i]); }
         for (j = 1; j < i; j++)
         {
            t = hh[itmp + (size_t) j - 1];
            hh[itmp + (size_t) j - 1] = s[j - 1] * hh[itmp + (size_t) j] + c[j - 1] * t;
            hh[itmp + (size_t) j] = -s[j - 1] * t + c[j - 1] * hh[itmp + (size_t) j];
         }
         t = hh[itmp + (size_t) i] * hh[itmp + (size_t) i];
         t += hh[itmp + (size_t) i - 1] * hh[itmp + (size_t) i - 1];
         gamma = std::sqrt(t);
         if (gamma == 0.0) { gamma = epsmac; }
         c[i - 1] = hh[itmp + (size_t) i - 1] / gamma;
         s[i - 1] = hh[itmp + (size_t) i] / gamma;
         rs[i] = -hh[itmp + (size_t) i] * rs[i - 1];
         rs[i] /= gamma;
         rs[i - 1] = c[i - 1] * rs[i - 1];
         hh[itmp + (size_t) i - 1] = s[i - 1] * hh[itmp + (size_t) i] + c[i - 1] * hh[itmp + (size_t) i - 1];
         r_norm = std::fabs(rs[i]);
         if (r_norm <= epsilon && iter >= min_iter) { break; }
      }
      // upper triangular solve, then the update through the preconditioner
      rs[i - 1] = rs[i - 1] / hh[itmp + (size_t) i - 1];
      for (k = i - 2; k >= 0; k--)
      {
         t = 0.0;
         for (j = k + 1; j < i; j++) { t -= hh[(size_t) j * ld + (size_t) k] * rs[j]; }
         t += rs[k];
         rs[k] = t / hh[(size_t) k * ld + (size_t) k];
      }
      hypre_ParVectorCopy(p[i - 1], w);
      hypre_ParVectorScale(rs[i - 1], w);
      for (j = i - 2; j >= 0; j--) { hypre_ParVectorAxpy(rs[j], p[j], w); }
      precond(w, r);
      hypre_ParVectorAxpy(1.0, r, x);
      x->all_zeros = 0;
      if (r_norm <= epsilon && iter >= min_iter)
      {
         if (d->skip_real_r_check) { d->converged = 1; break; }
         hypre_ParVectorCopy(b, r);
         hypre_ParCSRMatrixMatvec(-1.0, A, x, 1.0, r);
         real_r_norm_new = r_norm = norm(r);
         if (r_norm <= epsilon) { d->converged = 1; break; }
         if (real_r_norm_new >= real_r_norm_old) { d->converged = 1; break; }     // cogmres.c:843-852
         hypre_ParVectorCopy(r, p[0]);
         i = 0;
         real_r_norm_old = real_r_norm_new;
      }
      // residual vector of the restart (cogmres.c:864-881)
      for (j = i; j > 0; j--)
      {
         rs[j - 1] = -s[j - 1] * rs[j];
         rs[j] = c[j - 1] * rs[j];
      }
      if (i) { hypre_ParVectorAxpy(rs[i] - 1.0, p[i], p[i]); }
      for (j = i - 1; j > 0; j--) { hypre_ParVectorAxpy(rs[j], p[j], p[i]); }
      if (i)
      {
         hypre_ParVectorAxpy(rs[0] - 1.0, p[0], p[0]);
         hypre_ParVectorAxpy(1.0, p[i], p[0]);
      }
   }
   d->num_iterations = iter;
   d->rel_residual_norm = (b_norm > 0.0) ? r_norm / b_norm : r_norm;
   if (iter >= max_iter && r_norm > epsilon && epsilon > 0) { hypre_error(HYPRE_ERROR_CONV); }
   return leave();
}

}  // extern "C"
