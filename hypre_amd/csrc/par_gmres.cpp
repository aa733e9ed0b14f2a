// hypre_amd — the four right-preconditioned restarted GMRES solvers on ParVectors on the device:
//    GMRES      HYPRE_ParCSRGMRES*  / HYPRE_GMRES*       `ij -solver 3 | 4`     krylov/gmres.c, parcsr_ls/HYPRE_parcsr_gmres.c
//    COGMRES    HYPRE_ParCSRCOGMRES* / HYPRE_COGMRES*    `ij -solver 16 | 17`   krylov/cogmres.c, parcsr_ls/HYPRE_parcsr_cogmres.c
//    FlexGMRES  HYPRE_ParCSRFlexGMRES* / HYPRE_FlexGMRES* `ij -solver 60 | 61`  krylov/flexgmres.c, parcsr_ls/HYPRE_parcsr_flexgmres.c
//    LGMRES     HYPRE_ParCSRLGMRES* / HYPRE_LGMRES*       `ij -solver 50 | 51`  krylov/lgmres.c, parcsr_ls/HYPRE_parcsr_lgmres.c
// The iteration itself (Hessenberg matrix, Givens rotations, every decision) is gmres_core.hpp, for LGMRES its sibling
// lgmres_core.hpp, a loop of its own built from the same step functions; this file gives it the vectors, every inner
// product ending in one scalar read-back, and the entry points (work vectors, preconditioner and the start of a solve
// as PCG has them: krylov_common.hpp).  The first three differ in the GMRESParams their Create fills in (the table is in DESIGN.md) and in two
// refusals: COGMRES Setup takes no multivectors, FlexGMRES Solve no host operands (LGMRES Solve neither).  The
// relative-change exit of the reference (rel_change) is carried by none of the four, the convergence-factor exit (cf_tol)
// by GMRES alone, which the hybrid solver drives with it (par_hybrid.cpp).
//
// Modified Gram-Schmidt, fused (the FlexGMRES default): step i is one hypre_ParVectorInnerProd and i launches of
// launch_axpy_dot, each subtracting the projection on p[j] and leaving <p[j + 1], p[i]> (the last one |p[i]|^2) in the
// same pass: 32 i + 8 bytes per element in i + 1 launches, where the dot / axpy sequence of the reference moves 40 i + 8
// in 2 i + 1.  Same order of operations and same roundings, so a solve has the same bits either way
// (hypre_amd_FlexGMRESSetFusedOrthogonalization).  Classical Gram-Schmidt (COGMRES) reads every basis vector twice per
// step and ends in two read-backs (the batch and the norm) where the modified one needs i + 1.
//
// LGMRES, fused (its default, hypre_amd_LGMRESSetFusedUpdates): the Gram-Schmidt steps as above; the correction of a
// cycle is one scaled copy and one hypre_ParVectorMassAxpy over the Arnoldi and augmentation terms; what ends a cycle that
// restarts (keep the correction, rebuild r0, normalise the new augmentation vector, form A z = (r0 - r_m) / |w|) is
// launch_copy_norm2, two launch_scale_copy and launch_scaled_diff: 4 launches and 72 bytes per element where the
// reference's ten Copy / Scale / InnerProd / Axpy calls move 168.  The same bits either way.
#include "krylov_common.hpp"
#include "lgmres_core.hpp"
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

using namespace hamd;

struct hypre_amd_GMRESData
{
   hypre_Solver base;
   MPI_Comm comm;
   GMRESParams prm;
   KrylovPrecond pc;
   HYPRE_PtrToModifyPCFcn modify_pc = nullptr;          // nullptr: hypre_FlexGMRESModifyPCDefault, which does nothing
   hypre_ParVector *r = nullptr, *w = nullptr;
   std::vector<hypre_ParVector *> p, pre_vecs;          // pre_vecs only if prm.flexible
   HYPRE_Int num_iterations = 0, converged = 0;
   HYPRE_Real rel_residual_norm = 0.0;
   HYPRE_Int fused_steps = 0, plain_dots = 0, plain_axpys = 0;
   // LGMRES only: aug_dim < 0 marks the other three
   HYPRE_Int aug_dim = -1, approx_constant = 1, fused_updates_on = 1;
   std::vector<hypre_ParVector *> aug_vecs, a_aug_vecs;   // aug_dim + 1 (the last a temporary) and aug_dim, as lgmres.c:270-278
   HYPRE_Int fused_updates = 0, plain_updates = 0;
};

namespace {
hypre_amd_GMRESData *D(HYPRE_Solver s) { return (hypre_amd_GMRESData *) s; }

void free_vectors(hypre_amd_GMRESData *d)
{
   hypre_ParVectorDestroy(d->r); hypre_ParVectorDestroy(d->w);
   d->r = d->w = nullptr;
   for (hypre_ParVector *v : d->p) { hypre_ParVectorDestroy(v); }
   for (hypre_ParVector *v : d->pre_vecs) { hypre_ParVectorDestroy(v); }
   for (hypre_ParVector *v : d->aug_vecs) { hypre_ParVectorDestroy(v); }
   for (hypre_ParVector *v : d->a_aug_vecs) { hypre_ParVectorDestroy(v); }
   d->p.clear(); d->pre_vecs.clear(); d->aug_vecs.clear(); d->a_aug_vecs.clear();
}

HYPRE_Int create(MPI_Comm comm, HYPRE_Solver *solver, const GMRESParams &prm)
{
   hypre_amd_GMRESData *d = new hypre_amd_GMRESData();
   memset(&d->base, 0, sizeof(d->base));
   d->comm = comm;
   d->prm = prm;
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}

HYPRE_Int destroy(HYPRE_Solver solver)
{
   if (!solver) { return hypre_error_flag; }
   free_vectors(D(solver));
   delete D(solver);
   return hypre_error_flag;
}

HYPRE_Int set_k_dim(HYPRE_Solver s, HYPRE_Int v)
{
   if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->prm.k_dim = v;
   return hypre_error_flag;
}

bool on_device(hypre_ParVector *v) { return v->local_vector->memory_location == HYPRE_MEMORY_DEVICE; }

// work vectors shaped like x (gmres.c:204-215, cogmres.c:220-231, flexgmres.c:230-250 CreateVector / CreateVectorArray):
// the columns of a multivector x
HYPRE_Int setup(HYPRE_Solver solver, hypre_ParCSRMatrix *A, hypre_ParVector *b, hypre_ParVector *x)
{
   hypre_amd_GMRESData *d = D(solver);
   free_vectors(d);
   auto mk = [&]() { return par_vector_like(A, x); };
   d->r = mk(); d->w = mk();
   for (HYPRE_Int i = 0; i <= d->prm.k_dim; i++)
   {
      d->p.push_back(mk());
      if (d->prm.flexible) { d->pre_vecs.push_back(mk()); }
   }
   for (HYPRE_Int i = 0; i <= d->aug_dim; i++)
   {
      d->aug_vecs.push_back(mk());
      if (i < d->aug_dim) { d->a_aug_vecs.push_back(mk()); }
   }
   if (d->pc.setup) { d->pc.setup(d->pc.data, A, b, x); }
   return hypre_error_flag;
}

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

size_t flat_length(hypre_ParVector *v) { return (size_t) v->local_vector->size * (size_t) v->local_vector->num_vectors; }

// y = a x: the bits of hypre_ParVectorCopy(x, y) followed by hypre_ParVectorScale(a, y), whose shortcut at a == 0 (set
// to zero, whatever x holds) is kept; at a == 1 the product is x itself
void scaled_copy_of(HYPRE_Complex a, hypre_ParVector *x, hypre_ParVector *y)
{
   if (a == 0.0) { launch_set(y->local_vector->data, 0.0, flat_length(y), stream()); }
   else { launch_scale_copy(a, x->local_vector->data, y->local_vector->data, flat_length(y), stream()); }
}

// y = x, then <x, x> over all ranks: the fused launch and the reduction of hypre_ParVectorInnerProd(y, y)
HYPRE_Real copy_then_inner_prod(hypre_ParVector *x, hypre_ParVector *y)
{
   double *d_out = reduce_scratch(2048);
   launch_copy_norm2(x->local_vector->data, y->local_vector->data, flat_length(y), d_out, stream());
   double r = 0.0;
   dev_global_sums(y->comm, d_out, 1, &r);
   return r;
}

// z = a (x - y): the bits of Copy(x, z), Scale(-1, z), Axpy(1, y, z), Scale(-a, z), the last one's shortcut at a == 0 kept
void scaled_difference(HYPRE_Complex a, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z)
{
   if (a == 0.0) { launch_set(z->local_vector->data, 0.0, flat_length(z), stream()); }
   else { launch_scaled_diff(a, x->local_vector->data, y->local_vector->data, z->local_vector->data, flat_length(z), stream()); }
}

// the vector operations gmres_iterate and lgmres_iterate ask for
struct ParOps
{
   hypre_amd_GMRESData *d;
   hypre_ParCSRMatrix *A;
   void matvec(double alpha, hypre_ParVector *x, double beta, hypre_ParVector *y) { hypre_ParCSRMatrixMatvec(alpha, A, x, beta, y); }
   double inner(hypre_ParVector *x, hypre_ParVector *y) { return hypre_ParVectorInnerProd(x, y); }
   void copy(hypre_ParVector *x, hypre_ParVector *y) { hypre_ParVectorCopy(x, y); }
   void scale(double a, hypre_ParVector *y) { hypre_ParVectorScale(a, y); }
   void axpy(double a, hypre_ParVector *x, hypre_ParVector *y) { hypre_ParVectorAxpy(a, x, y); }
   double axpy_dot(double a, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z) { return axpy_then_inner_prod(a, x, y, z); }
   void mass_axpy(double *a, hypre_ParVector **xs, hypre_ParVector *y, int k, int unroll) { hypre_ParVectorMassAxpy(a, xs, y, k, unroll); }
   void mass_inner(hypre_ParVector *x, hypre_ParVector **ys, int k, int unroll, double *out) { hypre_ParVectorMassInnerProd(x, ys, k, unroll, out); }
   void mass_dot_two(hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector **zs, int k, int unroll, double *outx, double *outy)
   { hypre_ParVectorMassDotpTwo(x, y, zs, k, unroll, outx, outy); }
   void precond(int iter, double rel_norm, hypre_ParVector *rhs, hypre_ParVector *sol)
   {
      d->pc.apply(A, rhs, sol, [&] { if (d->modify_pc) { d->modify_pc(d->pc.data, iter, rel_norm); } });
   }
   void solution_changed(hypre_ParVector *x) { x->all_zeros = 0; }
   void scaled_copy(double a, hypre_ParVector *x, hypre_ParVector *y) { scaled_copy_of(a, x, y); }
   double copy_norm2(hypre_ParVector *x, hypre_ParVector *y) { return copy_then_inner_prod(x, y); }
   void scaled_diff(double a, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z) { scaled_difference(a, x, y, z); }
};

// the work vectors are those of another k_dim: msg is the entry point's "...Solve: call ...Setup after ...SetKDim"
bool stale(HYPRE_Solver solver, const char *msg)
{
   if ((HYPRE_Int) D(solver)->p.size() == D(solver)->prm.k_dim + 1) { return false; }
   hypre_error_w_msg(HYPRE_ERROR_GENERIC, msg);
   return true;
}

// one solve: `iterate` runs the loop on the ParOps it is given; the synchronisation after every vector call is off
// meanwhile, and what the loop reports is stored for the getters and turned into the error flags of the reference
template <class Iterate>
HYPRE_Int solve_with(hypre_amd_GMRESData *d, hypre_ParCSRMatrix *A, Iterate iterate)
{
   d->converged = 0;
   d->fused_steps = d->plain_dots = d->plain_axpys = 0;
   QuietSolve quiet(A);
   ParOps ops{d, A};
   const GMRESResult res = iterate(ops);
   if (res.iterations_set) { d->num_iterations = res.iterations; }
   d->converged = res.converged;
   if (res.norm_set) { d->rel_residual_norm = res.rel_residual_norm; }
   d->fused_steps = (HYPRE_Int) res.fused_steps; d->plain_dots = (HYPRE_Int) res.plain_dots; d->plain_axpys = (HYPRE_Int) res.plain_axpys;
   if (res.status == GMRES_NOT_A_NUMBER) { hypre_error(HYPRE_ERROR_GENERIC); }
   if (res.status == GMRES_NOT_CONVERGED) { hypre_error(HYPRE_ERROR_CONV); }
   quiet.restore();
   maybe_sync();
   return hypre_error_flag;
}

HYPRE_Int solve(HYPRE_Solver solver, hypre_ParCSRMatrix *A, hypre_ParVector *b, hypre_ParVector *x)
{
   hypre_amd_GMRESData *d = D(solver);
   return solve_with(d, A, [&](ParOps &ops) { return gmres_iterate<hypre_ParVector *>(d->prm, ops, b, x, d->r, d->w, d->p.data(), d->pre_vecs.data()); });
}
}  // namespace

extern "C" {

// ---- GMRES: defaults of hypre_GMRESCreate (gmres.c:68-110): k_dim 5, tol 1e-6, a_tol 0, min_iter 0, max_iter 1000,
// rel_change 0, skip_real_r_check 0; modified Gram-Schmidt, plain
HYPRE_Int HYPRE_ParCSRGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver) { return create(comm, solver, GMRESParams()); }
HYPRE_Int HYPRE_ParCSRGMRESDestroy(HYPRE_Solver solver) { return destroy(solver); }
HYPRE_Int HYPRE_GMRESSetKDim(HYPRE_Solver s, HYPRE_Int v) { return set_k_dim(s, v); }
HYPRE_Int HYPRE_GMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESSetSkipRealResidualCheck(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.skip_real_r_check = v; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                HYPRE_Solver precond_solver)
{ return D(s)->pc.set(precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_GMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }       // accepted, inert
HYPRE_Int HYPRE_GMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESSetRelChange(HYPRE_Solver s, HYPRE_Int v)
{
   (void) s;
   if (v != 0) { hypre_error_in_arg(2); hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_GMRESSetRelChange: the relative-change stopping test is not built (0 only)"); }
   return hypre_error_flag;
}
HYPRE_Int HYPRE_GMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_GMRESGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->converged; return hypre_error_flag; }
// gmres.c:597-615, 1016-1035: 0.0 (the default) computes nothing and changes no iteration
HYPRE_Int HYPRE_GMRESSetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real v)
{
   D(s)->prm.cf_tol = v;
   D(s)->prm.cf_exit = convergence_factor_exceeds;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_GMRESGetConvergenceFactorTol(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->prm.cf_tol; return hypre_error_flag; }
HYPRE_Int hypre_GMRESSetHybrid(HYPRE_Solver s, HYPRE_Int level) { D(s)->prm.quiet_at_max_iter = level == -1; return hypre_error_flag; }

HYPRE_Int HYPRE_ParCSRGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   return setup(solver, A, b, x);
}
HYPRE_Int HYPRE_ParCSRGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   if (stale(solver, "HYPRE_ParCSRGMRESSolve: call HYPRE_ParCSRGMRESSetup after HYPRE_GMRESSetKDim")) { return hypre_error_flag; }
   return solve(solver, A, b, x);
}

// ---- COGMRES: defaults of hypre_COGMRESCreate (cogmres.c:85-111): k_dim 5, cgs 1, unroll 0, tol 1e-6, a_tol 0,
// min_iter 0, max_iter 1000, skip_real_r_check 0
HYPRE_Int HYPRE_ParCSRCOGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   GMRESParams prm;
   prm.ortho = GMRESOrtho::CGS;
   prm.count_at_zero_residual = false;
   return create(comm, solver, prm);
}
HYPRE_Int HYPRE_ParCSRCOGMRESDestroy(HYPRE_Solver solver) { return destroy(solver); }
HYPRE_Int HYPRE_COGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v) { return set_k_dim(s, v); }
HYPRE_Int HYPRE_COGMRESSetUnroll(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.unroll = v; return hypre_error_flag; }   // handed on, ignored by the kernels
HYPRE_Int HYPRE_COGMRESSetCGS(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.ortho = v > 1 ? GMRESOrtho::CGS2 : GMRESOrtho::CGS; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetSkipRealResidualCheck(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.skip_real_r_check = v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                  HYPRE_Solver precond_solver)
{ return D(s)->pc.set(precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_COGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }       // accepted, inert
HYPRE_Int HYPRE_COGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_COGMRESGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->converged; return hypre_error_flag; }

HYPRE_Int HYPRE_ParCSRCOGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   free_vectors(D(solver));
   if (x->local_vector->num_vectors > 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRCOGMRESSetup: multivectors are not served by COGMRES (use HYPRE_ParCSRGMRES)");
      return hypre_error_flag;
   }
   return setup(solver, A, b, x);
}
HYPRE_Int HYPRE_ParCSRCOGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   if (stale(solver, "HYPRE_ParCSRCOGMRESSolve: call HYPRE_ParCSRCOGMRESSetup after HYPRE_COGMRESSetKDim")) { return hypre_error_flag; }
   return solve(solver, A, b, x);
}

// ---- FlexGMRES: defaults of hypre_FlexGMRESCreate (flexgmres.c:86-91): k_dim 20, tol 1e-6, a_tol 0, min_iter 0,
// max_iter 1000; modified Gram-Schmidt, fused.  Before every preconditioner call the target is cleared and
// modify_pc(precond_data, iter, r_norm / den_norm) is called.
HYPRE_Int HYPRE_ParCSRFlexGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   GMRESParams prm;
   prm.k_dim = 20;
   prm.ortho = GMRESOrtho::MGS_FUSED;
   prm.flexible = true;
   prm.stop_when_residual_grows = false;
   prm.conv_error_at_zero_tol = true;
   return create(comm, solver, prm);
}
HYPRE_Int HYPRE_ParCSRFlexGMRESDestroy(HYPRE_Solver solver) { return destroy(solver); }
HYPRE_Int HYPRE_FlexGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v) { return set_k_dim(s, v); }
HYPRE_Int HYPRE_FlexGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.a_tol = v; return hypre_error_flag; }
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
HYPRE_Int HYPRE_FlexGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                    HYPRE_Solver precond_solver)
{ return D(s)->pc.set(precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_FlexGMRESGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { *precond_data_ptr = D(s)->pc.data; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetModifyPC(HYPRE_Solver s, HYPRE_PtrToModifyPCFcn modify_pc) { D(s)->modify_pc = modify_pc; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }       // accepted, inert
HYPRE_Int HYPRE_FlexGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_FlexGMRESGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->converged; return hypre_error_flag; }

HYPRE_Int hypre_amd_FlexGMRESSetFusedOrthogonalization(HYPRE_Solver s, HYPRE_Int on)
{
   if (on != 0 && on != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->prm.ortho = on ? GMRESOrtho::MGS_FUSED : GMRESOrtho::MGS;
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_FlexGMRESGetLaunchStats(HYPRE_Solver s, HYPRE_Int *fused_steps, HYPRE_Int *plain_dots, HYPRE_Int *plain_axpys)
{
   hypre_amd_GMRESData *d = D(s);
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
   return setup(solver, A, b, x);
}
HYPRE_Int HYPRE_ParCSRFlexGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_GMRESData *d = D(solver);
   if (stale(solver, "HYPRE_ParCSRFlexGMRESSolve: call HYPRE_ParCSRFlexGMRESSetup after HYPRE_FlexGMRESSetKDim")) { return hypre_error_flag; }
   if (!on_device(b) || !on_device(x) || !on_device(d->r))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRFlexGMRESSolve: operand is not in device memory; host execution is not part of this library");
      return hypre_error_flag;
   }
   d->num_iterations = 0;                  // also a solve that ends at the not-a-number check reports 0 iterations here
   return solve(solver, A, b, x);
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

// ---- LGMRES: defaults of hypre_LGMRESCreate (lgmres.c:83-105): k_dim 20, aug_dim 2, approx_constant 1, tol 1e-6,
// a_tol 0, min_iter 0, max_iter 1000; the iteration is lgmres_iterate, fused
HYPRE_Int HYPRE_ParCSRLGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver)
{
   create(comm, solver, LGMRESParams());            // kept as GMRESParams: k_dim 20, the rest of the defaults are the same
   D(*solver)->aug_dim = 2;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRLGMRESDestroy(HYPRE_Solver solver) { return destroy(solver); }
HYPRE_Int HYPRE_LGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v) { return set_k_dim(s, v); }
// at least 0 and at most k_dim - 1, the k_dim in force at this call (lgmres.c:970-986)
HYPRE_Int HYPRE_LGMRESSetAugDim(HYPRE_Solver s, HYPRE_Int v)
{
   D(s)->aug_dim = std::max(0, std::min(v, D(s)->prm.k_dim - 1));
   return hypre_error_flag;
}
HYPRE_Int HYPRE_LGMRESGetAugDim(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->aug_dim; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { D(s)->prm.a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.min_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { D(s)->prm.max_iter = v; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                 HYPRE_Solver precond_solver)
{ return D(s)->pc.set(precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_LGMRESGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { *precond_data_ptr = D(s)->pc.data; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }       // accepted, inert
HYPRE_Int HYPRE_LGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { (void) s; (void) v; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->num_iterations; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { *v = D(s)->rel_residual_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_LGMRESGetConverged(HYPRE_Solver s, HYPRE_Int *v) { *v = D(s)->converged; return hypre_error_flag; }
// the work vector that holds b - A x after a solve that checked it (lgmres.c:207-213); NULL before Setup
HYPRE_Int HYPRE_LGMRESGetResidual(HYPRE_Solver s, void *residual) { *(hypre_ParVector **) residual = D(s)->r; return hypre_error_flag; }

HYPRE_Int hypre_amd_LGMRESSetApproxConstant(HYPRE_Solver s, HYPRE_Int on)
{
   if (on != 0 && on != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->approx_constant = on;
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_LGMRESSetFusedUpdates(HYPRE_Solver s, HYPRE_Int on)
{
   if (on != 0 && on != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->fused_updates_on = on;
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_LGMRESGetLaunchStats(HYPRE_Solver s, HYPRE_Int *fused_steps, HYPRE_Int *plain_dots, HYPRE_Int *plain_axpys,
                                         HYPRE_Int *fused_updates, HYPRE_Int *plain_updates)
{
   hypre_amd_GMRESData *d = D(s);
   if (fused_updates) { *fused_updates = d->fused_updates; }
   if (plain_updates) { *plain_updates = d->plain_updates; }
   return hypre_amd_FlexGMRESGetLaunchStats(s, fused_steps, plain_dots, plain_axpys);
}

HYPRE_Int HYPRE_ParCSRLGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   return setup(solver, A, b, x);
}
HYPRE_Int HYPRE_ParCSRLGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   hypre_amd_GMRESData *d = D(solver);
   if (d->aug_dim > d->prm.k_dim - 1)
   {
      // SetAugDim clamps against the k_dim of its day; a smaller k_dim set afterwards would leave a cycle no Arnoldi step
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRLGMRESSolve: aug_dim exceeds k_dim - 1; call HYPRE_LGMRESSetAugDim after HYPRE_LGMRESSetKDim");
      return hypre_error_flag;
   }
   if (stale(solver, "HYPRE_ParCSRLGMRESSolve: call HYPRE_ParCSRLGMRESSetup after HYPRE_LGMRESSetKDim")) { return hypre_error_flag; }
   if ((HYPRE_Int) d->aug_vecs.size() != d->aug_dim + 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRLGMRESSolve: call HYPRE_ParCSRLGMRESSetup after HYPRE_LGMRESSetAugDim");
      return hypre_error_flag;
   }
   if (!on_device(b) || !on_device(x) || !on_device(d->r))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ParCSRLGMRESSolve: operand is not in device memory; host execution is not part of this library");
      return hypre_error_flag;
   }
   LGMRESParams prm;
   static_cast<GMRESParams &>(prm) = d->prm;
   prm.aug_dim = d->aug_dim; prm.approx_constant = d->approx_constant; prm.fused = d->fused_updates_on != 0;
   d->fused_updates = d->plain_updates = 0;
   return solve_with(d, A, [&](ParOps &ops) {
      const LGMRESResult res = lgmres_iterate<hypre_ParVector *>(prm, ops, b, x, d->r, d->w, d->p.data(), d->aug_vecs.data(), d->a_aug_vecs.data());
      d->fused_updates = (HYPRE_Int) res.fused_updates; d->plain_updates = (HYPRE_Int) res.plain_updates;
      return res;
   });
}

// the spellings of parcsr_ls/HYPRE_parcsr_lgmres.c and the generic Setup / Solve of krylov/HYPRE_lgmres.c
HYPRE_Int HYPRE_LGMRESSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return HYPRE_ParCSRLGMRESSetup(s, A, b, x); }
HYPRE_Int HYPRE_LGMRESSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return HYPRE_ParCSRLGMRESSolve(s, A, b, x); }
HYPRE_Int HYPRE_ParCSRLGMRESSetKDim(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_LGMRESSetKDim(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetAugDim(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_LGMRESSetAugDim(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetTol(HYPRE_Solver s, HYPRE_Real v) { return HYPRE_LGMRESSetTol(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v) { return HYPRE_LGMRESSetAbsoluteTol(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetMinIter(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_LGMRESSetMinIter(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetMaxIter(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_LGMRESSetMaxIter(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                       HYPRE_Solver precond_solver)
{ return HYPRE_LGMRESSetPrecond(s, precond, precond_setup, precond_solver); }
HYPRE_Int HYPRE_ParCSRLGMRESGetPrecond(HYPRE_Solver s, HYPRE_Solver *precond_data_ptr) { return HYPRE_LGMRESGetPrecond(s, precond_data_ptr); }
HYPRE_Int HYPRE_ParCSRLGMRESSetLogging(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_LGMRESSetLogging(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { return HYPRE_LGMRESSetPrintLevel(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { return HYPRE_LGMRESGetNumIterations(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { return HYPRE_LGMRESGetFinalRelativeResidualNorm(s, v); }
HYPRE_Int HYPRE_ParCSRLGMRESGetResidual(HYPRE_Solver s, HYPRE_ParVector *residual) { return HYPRE_LGMRESGetResidual(s, residual); }

// the three fused vector operations of LGMRES on their own: each has the bits of the library calls it replaces
namespace {
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
}  // namespace
HYPRE_Int hypre_amd_ParVectorScaledCopy(HYPRE_Complex a, hypre_ParVector *x, hypre_ParVector *y)
{
   if (!same_device_length("hypre_amd_ParVectorScaledCopy", {x, y})) { return hypre_error_flag; }
   if (x == y) { hypre_error_in_arg(3); return hypre_error_flag; }
   scaled_copy_of(a, x, y);
   maybe_sync();
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_ParVectorCopyThenInnerProd(hypre_ParVector *x, hypre_ParVector *y, HYPRE_Real *result)
{
   if (!same_device_length("hypre_amd_ParVectorCopyThenInnerProd", {x, y})) { return hypre_error_flag; }
   if (x == y) { hypre_error_in_arg(2); return hypre_error_flag; }
   *result = copy_then_inner_prod(x, y);
   return hypre_error_flag;
}
HYPRE_Int hypre_amd_ParVectorScaledDifference(HYPRE_Complex a, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z)
{
   if (!same_device_length("hypre_amd_ParVectorScaledDifference", {x, y, z})) { return hypre_error_flag; }
   if (z == x || z == y) { hypre_error_in_arg(4); return hypre_error_flag; }
   scaled_difference(a, x, y, z);
   maybe_sync();
   return hypre_error_flag;
}

}  // extern "C"
