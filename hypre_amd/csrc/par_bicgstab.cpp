// hypre_amd — BiCGSTAB on ParVectors on the device: HYPRE_ParCSRBiCGSTAB* / HYPRE_BiCGSTAB* (krylov/bicgstab.c:225-578,
// krylov/HYPRE_bicgstab.c, parcsr_ls/HYPRE_parcsr_bicgstab.c; the reference's `ij -solver 9 | 10`).  An iteration is two
// preconditioner applications and two products with A; between them the reference makes eleven vector calls, five of which
// end in a read-back.  With fused updates (the default) these are two axpys, one pass for <r, s> and <s, s>, one pass for
// the second half step with <r, r> and <r0, r> of the new residual, and one pass for the direction: three read-backs.
// Every fused pass has the bits of the calls it stands for (mass_kernels.hip), so a solve is the same either way.
#include "krylov_common.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

using namespace hamd;

extern "C" {

struct hypre_amd_BiCGSTABData
{
   hypre_Solver base;
   MPI_Comm comm;
   // defaults of hypre_BiCGSTABCreate (bicgstab.c:75-84)
   HYPRE_Real tol = 1e-6, a_tol = 0.0, cf_tol = 0.0;
   HYPRE_Int min_iter = 0, max_iter = 1000, stop_crit = 0, logging = 0, print_level = 0;
   HYPRE_Int fused = 1;
   HYPRE_Int hybrid = 0;                   // -1: the diagonally scaled phase of the hybrid solver (hypre_BiCGSTABSetHybrid)
   KrylovPrecond pc;
   hypre_ParVector *p = nullptr, *q = nullptr, *r = nullptr, *r0 = nullptr, *s = nullptr, *v = nullptr;
   std::vector<HYPRE_Real> norms;          // |r| before the first iteration and after every one, with logging or print_level > 0
   HYPRE_Int num_iterations = 0, converged = 0;
   HYPRE_Real rel_residual_norm = 0.0;
};

}  // extern "C"

namespace {
hypre_amd_BiCGSTABData *D(HYPRE_Solver s) { return (hypre_amd_BiCGSTABData *) s; }

bool on_device(hypre_ParVector *v) { return v->local_vector->memory_location == HYPRE_MEMORY_DEVICE; }
size_t flat_length(hypre_ParVector *v) { return (size_t) v->local_vector->size * (size_t) v->local_vector->num_vectors; }

void free_vectors(hypre_amd_BiCGSTABData *d)
{
   for (hypre_ParVector **v : {&d->p, &d->q, &d->r, &d->r0, &d->s, &d->v}) { hypre_ParVectorDestroy(*v); *v = nullptr; }
}

// <x, y> and <y, y> over all ranks: one pass, one reduction of two values, one read-back
void inner_prod_with_norm2(hypre_ParVector *x, hypre_ParVector *y, HYPRE_Real *xy, HYPRE_Real *yy)
{
   double *d_out = launch_dot_with_norm2(x->local_vector->data, y->local_vector->data, flat_length(y), stream());
   double sums[2];
   dev_global_sums(y->comm, d_out, 2, sums);
   *xy = sums[0]; *yy = sums[1];
}

// x += a v, r += b s, then <r, r> and <r0, r> over all ranks: one pass, one reduction of two values, one read-back
void two_axpys_then_inner_prods(HYPRE_Complex a, hypre_ParVector *v, hypre_ParVector *x, HYPRE_Complex b, hypre_ParVector *s,
                                hypre_ParVector *r, hypre_ParVector *r0, HYPRE_Real *rr, HYPRE_Real *r0r)
{
   double *d_out = launch_bicgstab_update(a, v->local_vector->data, x->local_vector->data, b, s->local_vector->data,
                                          r->local_vector->data, r0->local_vector->data, flat_length(r), stream());
   x->all_zeros = 0; r->all_zeros = 0;
   double sums[2];
   dev_global_sums(r->comm, d_out, 2, sums);
   *rr = sums[0]; *r0r = sums[1];
}

// p = r + c (p + g q)
void direction_update(HYPRE_Complex g, hypre_ParVector *q, HYPRE_Complex c, hypre_ParVector *r, hypre_ParVector *p)
{
   launch_bicgstab_direction(g, q->local_vector->data, c, r->local_vector->data, p->local_vector->data, flat_length(p), stream());
   p->all_zeros = 0;
}

bool same_device_length(const char *who, std::initializer_list<hypre_ParVector *> vs)
{
   const size_t n = flat_length(*vs.begin());
   for (hypre_ParVector *v : vs)
   {
      if (!on_device(v))
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, (std::string(who) + ": operand is not in device memory; host execution is not part of this library").c_str());
         return false;
      }
      if (flat_length(v) != n)
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, (std::string(who) + ": the vectors differ in length").c_str());
         return false;
      }
   }
   return true;
}

// an argument that is written must be none of the others
bool distinct(std::initializer_list<hypre_ParVector *> written, std::initializer_list<hypre_ParVector *> all)
{
   for (hypre_ParVector *w : written)
   {
      int seen = 0;
      for (hypre_ParVector *v : all) { seen += v == w || v->local_vector->data == w->local_vector->data; }
      if (seen != 1) { return false; }
   }
   return true;
}
}  // namespace

extern "C" {

HYPRE_Int HYPRE_ParCSRBiCGSTABCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   hypre_amd_BiCGSTABData *d = new hypre_amd_BiCGSTABData();
   memset(&d->base, 0, sizeof(d->base));
   d->comm = comm;
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRBiCGSTABDestroy(HYPRE_Solver solver)
{
   hypre_amd_BiCGSTABData *d = D(solver);
   if (!d) { return hypre_error_flag; }
   free_vectors(d);
   delete d;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_BiCGSTABDestroy(HYPRE_Solver s) { return HYPRE_ParCSRBiCGSTABDestroy(s); }

HYPRE_Int HYPRE_BiCGSTABSetTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->cf_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetMinIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetStopCrit(HYPRE_Solver s, HYPRE_Int v) { D(s)->stop_crit = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                   HYPRE_Solver precond_solver)
{ return D(s)->pc.set(precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_BiCGSTABGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { *precond_data_ptr = D(s)->pc.data; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetLogging(HYPRE_Solver s, HYPRE_Int v) { D(s)->logging = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { D(s)->print_level = v; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_BiCGSTABGetResidual(HYPRE_Solver s, void *residual) { *((hypre_ParVector **) residual) = D(s)->r; return hypre_error_flag; }

HYPRE_Int hypre_amd_BiCGSTABSetFusedUpdates(HYPRE_Solver s, HYPRE_Int on)
{
   if (on != 0 && on != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->fused = on;
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_BiCGSTABGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->converged; return hypre_error_flag; }
// the same under the name the other Krylov solvers give it (the reference has hypre_BiCGSTABGetConverged only, krylov.h:1227)
HYPRE_Int HYPRE_BiCGSTABGetConverged(HYPRE_Solver s, HYPRE_Int *v) { return hypre_amd_BiCGSTABGetConverged(s, v); }
HYPRE_Int HYPRE_BiCGSTABGetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->cf_tol; return hypre_error_flag; }
HYPRE_Int hypre_BiCGSTABSetHybrid(HYPRE_Solver s, HYPRE_Int level) { D(s)->hybrid = level; return hypre_error_flag; }
HYPRE_Int hypre_amd_BiCGSTABGetLoggedNorms(HYPRE_Solver s, HYPRE_Int *count, const HYPRE_Real **norms)
{
   *count = (HYPRE_Int) D(s)->norms.size();
   *norms = D(s)->norms.data();
   return hypre_error_flag;
}

// the six work vectors shaped like x (bicgstab.c:165-188 CreateVector): the columns of a multivector x
HYPRE_Int HYPRE_ParCSRBiCGSTABSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_BiCGSTABData *d = D(solver);
   free_vectors(d);
   for (hypre_ParVector **v : {&d->p, &d->q, &d->r, &d->r0, &d->s, &d->v}) { *v = par_vector_like(A, x); }
   if (d->pc.setup) { d->pc.setup(d->pc.data, A, b, x); }
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRBiCGSTABSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_BiCGSTABData *d = D(solver);
   hypre_ParVector *p = d->p, *q = d->q, *r = d->r, *r0 = d->r0, *s = d->s, *v = d->v;
   if (!r)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRBiCGSTABSolve: call HYPRE_ParCSRBiCGSTABSetup first");
      return hypre_error_flag;
   }
   if (!on_device(b) || !on_device(x) || !on_device(r))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRBiCGSTABSolve: operand is not in device memory; host execution is not part of this library");
      return hypre_error_flag;
   }
   // multivectors (`ij -nc N`): one iteration over the columns together, inner products over all of them; the fused
   // updates run over the columns' common storage, which has to be one piece
   const HYPRE_Int nvec = x->local_vector->num_vectors;
   for (hypre_ParVector *w : {b, x, p, q, r, r0, s, v})
   {
      const hypre_Vector *l = w->local_vector;
      if (l->num_vectors != nvec || l->size != r->local_vector->size || (nvec > 1 && (l->idxstride != 1 || l->vecstride != l->size)))
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRBiCGSTABSolve: b, x and the work vectors of HYPRE_ParCSRBiCGSTABSetup must have the same rows "
                                                "and number of columns, stored one after the other");
         return hypre_error_flag;
      }
   }
   const HYPRE_Int min_iter = d->min_iter, max_iter = d->max_iter, print_level = d->print_level;
   const HYPRE_Real r_tol = d->tol, a_tol = d->a_tol, cf_tol = d->cf_tol;
   const HYPRE_Real epsmac = DBL_MIN;                            // HYPRE_REAL_MIN
   const bool log = d->logging > 0 || print_level > 0, fused = d->fused != 0;
   HYPRE_Int my_id = 0, iter = 0;
   hypre_MPI_Comm_rank(A->comm, &my_id);
   const bool print = print_level > 0 && my_id == 0;
   HYPRE_Real alpha, beta, gamma, epsilon, temp, res, r_norm, b_norm, ieee_check = 0., cf_ave_0 = 0.0, cf_ave_1 = 0.0, r_norm_0,
              den_norm, gamma_numer, gamma_denom;
   std::vector<HYPRE_Real> &norms = d->norms;
   d->converged = 0;
   norms.clear();
   if (log) { norms.reserve((size_t) std::max<HYPRE_Int>(max_iter, 0) + 1); }

   QuietSolve quiet(A);
   struct Finish                                                 // every way out of the loop below ends the quiet section
   {
      QuietSolve &q;
      ~Finish() { q.restore(); maybe_sync(); }
   } finish{quiet};

   hypre_ParVectorCopy(b, r0);
   hypre_ParCSRMatrixMatvec(-1.0, A, x, 1.0, r0);
   hypre_ParVectorCopy(r0, r);
   hypre_ParVectorCopy(r0, p);
   b_norm = std::sqrt(hypre_ParVectorInnerProd(b, b));
   if (b_norm != 0.) { ieee_check = b_norm / b_norm; }
   if (ieee_check != ieee_check)
   {
      if (log) { printf("\n\nERROR detected by Hypre ...  BEGIN\nERROR -- hypre_BiCGSTABSolve: INFs and/or NaNs detected in input.\n"
                        "User probably placed non-numerics in supplied b.\nReturning error flag += 101.  Program not terminated.\n"
                        "ERROR detected by Hypre ...  END\n\n\n"); }
      hypre_error(HYPRE_ERROR_GENERIC);
      return hypre_error_flag;
   }
   res = hypre_ParVectorInnerProd(r0, r0);
   r_norm = std::sqrt(res);
   r_norm_0 = r_norm;
   if (r_norm != 0.) { ieee_check = r_norm / r_norm; }
   if (ieee_check != ieee_check)
   {
      if (log) { printf("\n\nERROR detected by Hypre ...  BEGIN\nERROR -- hypre_BiCGSTABSolve: INFs and/or NaNs detected in input.\n"
                        "User probably placed non-numerics in supplied A or x_0.\nReturning error flag += 101.  Program not terminated.\n"
                        "ERROR detected by Hypre ...  END\n\n\n"); }
      hypre_error(HYPRE_ERROR_GENERIC);
      return hypre_error_flag;
   }
   if (log)
   {
      norms.push_back(r_norm);
      if (print)
      {
         printf("L2 norm of b: %e\n", b_norm);
         if (b_norm == 0.0) { printf("Rel_resid_norm actually contains the residual norm\n"); }
         printf("Initial L2 norm of residual: %e\n", r_norm);
      }
   }
   // |r_i| <= max(a_tol, r_tol |b|), or r_tol |r_0| when b is zero; stop_crit: the absolute test of the older interface,
   // a_tol if set and else r_tol (bicgstab.c:366-403)
   den_norm = b_norm > 0.0 ? b_norm : r_norm;
   if (d->stop_crit) { epsilon = a_tol == 0.0 ? r_tol : a_tol; }
   else { epsilon = std::max(a_tol, r_tol * den_norm); }
   if (print)
   {
      printf("=============================================\n\n");
      if (b_norm > 0.0) { printf("Iters     resid.norm     conv.rate  rel.res.norm\n-----    ------------    ---------- ------------\n"); }
      else { printf("Iters     resid.norm     conv.rate\n-----    ------------    ----------\n"); }
   }
   d->num_iterations = iter;
   if (b_norm > 0.0) { d->rel_residual_norm = r_norm / b_norm; }
   if (r_norm == 0.0) { return hypre_error_flag; }
   if (r_norm <= epsilon && iter >= min_iter)
   {
      if (print) { printf("\n\nTolerance and min_iter requirements satisfied by initial data.\nFinal L2 norm of residual: %e\n\n", r_norm); }
      d->converged = 1;
      return hypre_error_flag;
   }
   // the three breakdown exits leave num_iterations and rel_residual_norm as they stand, like the reference
   auto broke_down = [&](const char *why) { hypre_error_w_msg(HYPRE_ERROR_GENERIC, why); return hypre_error_flag; };
   while (iter < max_iter)
   {
      iter++;
      d->pc.apply(A, p, v);
      hypre_ParCSRMatrixMatvec(1.0, A, v, 0.0, q);
      temp = hypre_ParVectorInnerProd(r0, q);
      if (std::fabs(temp) >= epsmac) { alpha = res / temp; }
      else { return broke_down("BiCGSTAB broke down!! divide by near zero\n"); }
      // the first half step stays two axpys: one launch for both would move the same 48 bytes per element
      hypre_ParVectorAxpy(alpha, v, x);
      hypre_ParVectorAxpy(-alpha, q, r);
      d->pc.apply(A, r, v);
      hypre_ParCSRMatrixMatvec(1.0, A, v, 0.0, s);
      if (fused) { inner_prod_with_norm2(r, s, &gamma_numer, &gamma_denom); }
      else
      {
         gamma_numer = hypre_ParVectorInnerProd(r, s);
         gamma_denom = hypre_ParVectorInnerProd(s, s);
      }
      gamma = (gamma_numer == 0.0 && gamma_denom == 0.0) ? 0.0 : gamma_numer / gamma_denom;      // 0 / 0 is 0 here, not a NaN
      HYPRE_Real rr, r0r = 0.0;
      if (fused) { two_axpys_then_inner_prods(gamma, v, x, -gamma, s, r, r0, &rr, &r0r); }       // <r0, r> is used if the iteration goes on
      else
      {
         hypre_ParVectorAxpy(gamma, v, x);
         hypre_ParVectorAxpy(-gamma, s, r);
         rr = hypre_ParVectorInnerProd(r, r);
      }
      r_norm = std::sqrt(rr);
      if (log) { norms.push_back(r_norm); }
      if (print)
      {
         if (b_norm > 0.0) { printf("% 5d    %e    %f   %e\n", (int) iter, norms[iter], norms[iter] / norms[iter - 1], norms[iter] / b_norm); }
         else { printf("% 5d    %e    %f\n", (int) iter, norms[iter], norms[iter] / norms[iter - 1]); }
      }
      // converged by the recurrence: the residual is computed from x and tested again
      bool recomputed = false;
      if (r_norm <= epsilon && iter >= min_iter)
      {
         hypre_ParVectorCopy(b, r);
         hypre_ParCSRMatrixMatvec(-1.0, A, x, 1.0, r);
         r_norm = std::sqrt(hypre_ParVectorInnerProd(r, r));
         recomputed = true;
         if (r_norm <= epsilon)
         {
            if (print) { printf("\n\nFinal L2 norm of residual: %e\n\n", r_norm); }
            d->converged = 1;
            break;
         }
      }
      if (cf_tol > 0.0)
      {
         cf_ave_0 = cf_ave_1;
         cf_ave_1 = std::pow(r_norm / r_norm_0, 1.0 / (2.0 * iter));
         if (convergence_factor_exceeds(cf_ave_1, cf_ave_0, cf_tol)) { break; }
      }
      if (std::fabs(res) >= epsmac) { beta = 1.0 / res; }
      else { return broke_down("BiCGSTAB broke down!! res=0 \n"); }
      res = (fused && !recomputed) ? r0r : hypre_ParVectorInnerProd(r0, r);                        // a recomputed r has other bits
      beta *= res;
      if (fused)
      {
         if (std::fabs(gamma) < epsmac)
         {
            hypre_ParVectorAxpy(-gamma, q, p);                                                   // the state the reference leaves
            return broke_down("BiCGSTAB broke down!! gamma=0 \n");
         }
         direction_update(-gamma, q, beta * alpha / gamma, r, p);
      }
      else
      {
         hypre_ParVectorAxpy(-gamma, q, p);
         if (std::fabs(gamma) >= epsmac) { hypre_ParVectorScale(beta * alpha / gamma, p); }
         else { return broke_down("BiCGSTAB broke down!! gamma=0 \n"); }
         hypre_ParVectorAxpy(1.0, r, p);
      }
   }
   d->num_iterations = iter;
   if (b_norm > 0.0) { d->rel_residual_norm = r_norm / b_norm; }
   if (b_norm == 0.0) { d->rel_residual_norm = r_norm; }
   if (iter >= max_iter && r_norm > epsilon && epsilon > 0 && d->hybrid != -1) { hypre_error(HYPRE_ERROR_CONV); }
   return hypre_error_flag;
}

HYPRE_Int HYPRE_BiCGSTABSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return HYPRE_ParCSRBiCGSTABSetup(s, A, b, x); }
HYPRE_Int HYPRE_BiCGSTABSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return HYPRE_ParCSRBiCGSTABSolve(s, A, b, x); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetTol(HYPRE_Solver s, HYPRE_Real v) { return HYPRE_BiCGSTABSetTol(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { return HYPRE_BiCGSTABSetAbsoluteTol(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetMinIter(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_BiCGSTABSetMinIter(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_BiCGSTABSetMaxIter(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetStopCrit(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_BiCGSTABSetStopCrit(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                         HYPRE_Solver precond_solver)
{ return HYPRE_BiCGSTABSetPrecond(s, precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_ParCSRBiCGSTABGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { return HYPRE_BiCGSTABGetPrecond(s, precond_data_ptr); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetLogging(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_BiCGSTABSetLogging(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_BiCGSTABSetPrintLevel(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { return HYPRE_BiCGSTABGetNumIterations(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { return HYPRE_BiCGSTABGetFinalRelativeResidualNorm(s, v); }
HYPRE_Int HYPRE_ParCSRBiCGSTABGetResidual(HYPRE_Solver s, HYPRE_ParVector *residual) { return HYPRE_BiCGSTABGetResidual(s, residual); }

// the three fused vector operations of BiCGSTAB on their own: each has the bits of the library calls it replaces
HYPRE_Int hypre_amd_ParVectorInnerProdWithNorm(hypre_ParVector *x, hypre_ParVector *y, HYPRE_Real *xy, HYPRE_Real *yy)
{
   if (!same_device_length("hypre_amd_ParVectorInnerProdWithNorm", {x, y})) { return hypre_error_flag; }
   inner_prod_with_norm2(x, y, xy, yy);
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_ParVectorTwoAxpysThenInnerProds(HYPRE_Complex a, hypre_ParVector *v, hypre_ParVector *x, HYPRE_Complex b, hypre_ParVector *s,
                                                    hypre_ParVector *r, hypre_ParVector *r0, HYPRE_Real *rr, HYPRE_Real *r0r)
{
   if (!same_device_length("hypre_amd_ParVectorTwoAxpysThenInnerProds", {v, x, s, r, r0})) { return hypre_error_flag; }
   if (!distinct({x, r}, {v, x, s, r, r0}))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ParVectorTwoAxpysThenInnerProds: x and r must each be distinct from every other operand");
      return hypre_error_flag;
   }
   two_axpys_then_inner_prods(a, v, x, b, s, r, r0, rr, r0r);
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_ParVectorAxpyScaleAxpy(HYPRE_Complex g, hypre_ParVector *q, HYPRE_Complex c, hypre_ParVector *r, hypre_ParVector *p)
{
   if (!same_device_length("hypre_amd_ParVectorAxpyScaleAxpy", {q, r, p})) { return hypre_error_flag; }
   if (!distinct({p}, {q, r, p})) { hypre_error_in_arg(5); return hypre_error_flag; }
   direction_update(g, q, c, r, p);
   maybe_sync();
   return hypre_error_flag;
}

}  // extern "C"
