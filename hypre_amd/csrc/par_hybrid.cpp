// hypre_amd — the hybrid solver on the device: HYPRE_ParCSRHybrid* (parcsr_ls/amg_hybrid.c, parcsr_ls/HYPRE_parcsr_hybrid.c;
// the reference's `ij -solver 20`).  It composes what the library has: a diagonally scaled Krylov solver (1 PCG, 2 GMRES,
// 3 BiCGSTAB) runs with the convergence-factor exit cf_tol and dscg_max_its; if it reports converged, that is the answer.
// Otherwise cf_tol is set to 0, a BoomerAMG preconditioner is created from the stored options and set up (unless one
// exists and setup_type 0 says to keep it), and the same Krylov solver goes on from the current x with pcg_max_its
// (amg_hybrid.c:1770-2310).  The diagonally scaled PCG phase takes the fused step of par_pcg.cpp under the conditions of
// any other PCG.
//
// Options of the reference whose other branches are not built go through the BoomerAMG setters when the preconditioner
// is created, and their gates raise the error; values the Krylov solvers do not carry are refused in the setter here.
#include "krylov_common.hpp"
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

using namespace hamd;

extern "C" {

struct hypre_amd_HybridData
{
   hypre_Solver base;
   // defaults of hypre_AMGHybridCreate (amg_hybrid.c:99-160)
   HYPRE_Real tol = 1.0e-06, a_tol = 0.0, cf_tol = 0.90;
   HYPRE_Int dscg_max_its = 1000, pcg_max_its = 200, two_norm = 0, stop_crit = 0, rel_change = 0, recompute_residual = 0;
   HYPRE_Int solver_type = 1, k_dim = 5, logging = 0, print_level = 0;
   HYPRE_Int setup_type = 1;
   HYPRE_Real strong_threshold = 0.25, max_row_sum = 0.9, trunc_factor = 0.0;
   HYPRE_Int pmax = 4, max_levels = 25, measure_type = 0, coarsen_type = 10, interp_type = 6, cycle_type = 1, relax_order = 0, keepT = 0;
   HYPRE_Int max_coarse_size = 9, min_coarse_size = 1, seq_threshold = 0;
   HYPRE_Int agg_num_levels = 0, agg_interp_type = 4, num_paths = 1, num_functions = 1, nodal = 0;
   std::vector<HYPRE_Int> num_grid_sweeps, grid_relax_type;     // empty: the reference's NULL
   std::vector<HYPRE_Real> relax_weight, omega;                 // per level, empty as above
   std::vector<HYPRE_Real> nongalerkin_tol;
   // the Krylov solver of solver_type `krylov_type` and the preconditioner, both kept between solves
   HYPRE_Solver krylov = nullptr, amg = nullptr;
   HYPRE_Int krylov_type = 0;
   HYPRE_Int dscg_num_its = 0, pcg_num_its = 0;
   HYPRE_Real final_rel_res_norm = 0.0;
   HYPRE_Real times[4] = {0.0, 0.0, 0.0, 0.0};                  // setup 1, solve 1, setup 2, solve 2
};

}  // extern "C"

namespace {
hypre_amd_HybridData *D(HYPRE_Solver s) { return (hypre_amd_HybridData *) s; }

double wall_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define HYBRID_DATA(solver, d)                                           \
   hypre_amd_HybridData *d = D(solver);                                  \
   if (!d) { hypre_error_in_arg(1); return hypre_error_flag; }

HYPRE_Int refuse(const char *what)
{
   hypre_error_in_arg(2);
   hypre_error_w_msg(HYPRE_ERROR_GENERIC, what);
   return hypre_error_flag;
}

// the three Krylov solvers behind one set of calls
struct KrylovCalls
{
   HYPRE_Int (*destroy)(HYPRE_Solver);
   HYPRE_Int (*set_max_iter)(HYPRE_Solver, HYPRE_Int);
   HYPRE_Int (*set_cf_tol)(HYPRE_Solver, HYPRE_Real);
   HYPRE_Int (*set_hybrid)(HYPRE_Solver, HYPRE_Int);
   HYPRE_Int (*set_precond)(HYPRE_Solver, HYPRE_PtrToSolverFcn, HYPRE_PtrToSolverFcn, HYPRE_Solver);
   HYPRE_Int (*setup)(HYPRE_Solver, HYPRE_ParCSRMatrix, HYPRE_ParVector, HYPRE_ParVector);
   HYPRE_Int (*solve)(HYPRE_Solver, HYPRE_ParCSRMatrix, HYPRE_ParVector, HYPRE_ParVector);
   HYPRE_Int (*get_its)(HYPRE_Solver, HYPRE_Int *);
   HYPRE_Int (*get_norm)(HYPRE_Solver, HYPRE_Real *);
   HYPRE_Int (*get_converged)(HYPRE_Solver, HYPRE_Int *);
};
const KrylovCalls &calls_of(HYPRE_Int solver_type)
{
   static const KrylovCalls pcg = {HYPRE_ParCSRPCGDestroy, HYPRE_PCGSetMaxIter, HYPRE_PCGSetConvergenceFactorTol, hypre_PCGSetHybrid, HYPRE_PCGSetPrecond,
                                   HYPRE_ParCSRPCGSetup, HYPRE_ParCSRPCGSolve, HYPRE_PCGGetNumIterations, HYPRE_PCGGetFinalRelativeResidualNorm,
                                   HYPRE_PCGGetConverged};
   static const KrylovCalls gmres = {HYPRE_ParCSRGMRESDestroy, HYPRE_GMRESSetMaxIter, HYPRE_GMRESSetConvergenceFactorTol, hypre_GMRESSetHybrid,
                                     HYPRE_GMRESSetPrecond, HYPRE_ParCSRGMRESSetup, HYPRE_ParCSRGMRESSolve, HYPRE_GMRESGetNumIterations,
                                     HYPRE_GMRESGetFinalRelativeResidualNorm, HYPRE_GMRESGetConverged};
   static const KrylovCalls bicgstab = {HYPRE_ParCSRBiCGSTABDestroy, HYPRE_BiCGSTABSetMaxIter, HYPRE_BiCGSTABSetConvergenceFactorTol,
                                        hypre_BiCGSTABSetHybrid, HYPRE_BiCGSTABSetPrecond, HYPRE_ParCSRBiCGSTABSetup, HYPRE_ParCSRBiCGSTABSolve,
                                        HYPRE_BiCGSTABGetNumIterations, HYPRE_BiCGSTABGetFinalRelativeResidualNorm, HYPRE_BiCGSTABGetConverged};
   return solver_type == 1 ? pcg : solver_type == 2 ? gmres : bicgstab;
}

void destroy_krylov(hypre_amd_HybridData *d)
{
   if (d->krylov) { calls_of(d->krylov_type).destroy(d->krylov); }
   d->krylov = nullptr; d->krylov_type = 0;
}

// the Krylov solver of amg_hybrid.c:1878-1906, 1944-1971, 2009-2032, made once and kept
void create_krylov(hypre_amd_HybridData *d, MPI_Comm comm, HYPRE_Int sol_print_level)
{
   HYPRE_Solver s = nullptr;
   if (d->solver_type == 1)
   {
      HYPRE_ParCSRPCGCreate(comm, &s);
      HYPRE_PCGSetTol(s, d->tol);
      HYPRE_PCGSetAbsoluteTol(s, d->a_tol);
      HYPRE_PCGSetTwoNorm(s, d->two_norm);
      HYPRE_PCGSetRelChange(s, d->rel_change);
      HYPRE_PCGSetRecomputeResidual(s, d->recompute_residual);
      HYPRE_PCGSetLogging(s, d->logging);
      HYPRE_PCGSetPrintLevel(s, sol_print_level);
   }
   else if (d->solver_type == 2)
   {
      HYPRE_ParCSRGMRESCreate(comm, &s);
      HYPRE_GMRESSetTol(s, d->tol);
      HYPRE_GMRESSetAbsoluteTol(s, d->a_tol);
      HYPRE_GMRESSetKDim(s, d->k_dim);
      HYPRE_GMRESSetRelChange(s, d->rel_change);
      HYPRE_GMRESSetLogging(s, d->logging);
      HYPRE_GMRESSetPrintLevel(s, sol_print_level);
   }
   else
   {
      HYPRE_ParCSRBiCGSTABCreate(comm, &s);
      HYPRE_BiCGSTABSetTol(s, d->tol);
      HYPRE_BiCGSTABSetAbsoluteTol(s, d->a_tol);
      HYPRE_BiCGSTABSetStopCrit(s, d->stop_crit);
      HYPRE_BiCGSTABSetLogging(s, d->logging);
      HYPRE_BiCGSTABSetPrintLevel(s, sol_print_level);
   }
   calls_of(d->solver_type).set_hybrid(s, -1);
   d->krylov = s; d->krylov_type = d->solver_type;
}

// the preconditioner of amg_hybrid.c:2108-2213: one cycle per application, every stored option through its setter
HYPRE_Solver create_amg(const hypre_amd_HybridData *d, HYPRE_Int pre_print_level)
{
   HYPRE_Solver s = nullptr;
   HYPRE_BoomerAMGCreate(&s);
   hypre_amd_BoomerAMGSetMemoryLocation(s, HYPRE_MEMORY_DEVICE);
   HYPRE_BoomerAMGSetMaxIter(s, 1);
   HYPRE_BoomerAMGSetTol(s, 0.0);
   HYPRE_BoomerAMGSetCoarsenType(s, d->coarsen_type);
   HYPRE_BoomerAMGSetInterpType(s, d->interp_type);
   HYPRE_BoomerAMGSetMeasureType(s, d->measure_type);
   HYPRE_BoomerAMGSetStrongThreshold(s, d->strong_threshold);
   HYPRE_BoomerAMGSetTruncFactor(s, d->trunc_factor);
   HYPRE_BoomerAMGSetPMaxElmts(s, d->pmax);
   HYPRE_BoomerAMGSetCycleType(s, d->cycle_type);
   HYPRE_BoomerAMGSetPrintLevel(s, pre_print_level);
   HYPRE_BoomerAMGSetMaxLevels(s, d->max_levels);
   HYPRE_BoomerAMGSetMaxRowSum(s, d->max_row_sum);
   HYPRE_BoomerAMGSetMaxCoarseSize(s, d->max_coarse_size);
   HYPRE_BoomerAMGSetMinCoarseSize(s, d->min_coarse_size);
   HYPRE_BoomerAMGSetSeqThreshold(s, d->seq_threshold);
   HYPRE_BoomerAMGSetAggNumLevels(s, d->agg_num_levels);        // agg_interp_type and num_paths are read with it only
   HYPRE_BoomerAMGSetNumPaths(s, d->num_paths);
   HYPRE_BoomerAMGSetNumFunctions(s, d->num_functions);
   HYPRE_BoomerAMGSetNodal(s, d->nodal);
   HYPRE_BoomerAMGSetRelaxOrder(s, d->relax_order);
   HYPRE_BoomerAMGSetKeepTranspose(s, d->keepT);
   for (HYPRE_Real t : d->nongalerkin_tol) { HYPRE_BoomerAMGSetNonGalerkinTol(s, t); }
   // smoothers: the stored four, or 3 / 13 / 14 / 9 (amg_hybrid.c:2135-2155)
   hypre_ParAMGData *amg = (hypre_ParAMGData *) s;
   const HYPRE_Int dflt[4] = {3, 13, 14, 9};
   const HYPRE_Int *grt = d->grid_relax_type.empty() ? dflt : d->grid_relax_type.data();
   for (HYPRE_Int k = 1; k < 4; k++) { HYPRE_BoomerAMGSetCycleRelaxType(s, grt[k], k); }
   amg->grid_relax_type[0] = grt[0];
   amg->user_relax_type = grt[0];
   if (!d->num_grid_sweeps.empty())
   {
      amg->num_grid_sweeps[0] = d->num_grid_sweeps[0];
      for (HYPRE_Int k = 1; k < 4; k++) { HYPRE_BoomerAMGSetCycleNumSweeps(s, d->num_grid_sweeps[(size_t) k], k); }
   }
   const HYPRE_Int levels = std::min<HYPRE_Int>(d->max_levels, (HYPRE_Int) std::max(d->relax_weight.size(), d->omega.size()));
   for (HYPRE_Int l = 0; l < levels; l++)
   {
      if (!d->relax_weight.empty()) { HYPRE_BoomerAMGSetLevelRelaxWt(s, d->relax_weight[(size_t) l], l); }
      if (!d->omega.empty()) { HYPRE_BoomerAMGSetLevelOuterWt(s, d->omega[(size_t) l], l); }
   }
   return s;
}

bool operands_fit(const char *who, hypre_ParCSRMatrix *A, hypre_ParVector *b, hypre_ParVector *x)
{
   if (A->diag->memory_location != HYPRE_MEMORY_DEVICE || b->local_vector->memory_location != HYPRE_MEMORY_DEVICE ||
       x->local_vector->memory_location != HYPRE_MEMORY_DEVICE)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, (std::string(who) + ": operand is not in device memory; host execution is not part of this library").c_str());
      return false;
   }
   if (b->local_vector->num_vectors != 1 || x->local_vector->num_vectors != 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, (std::string(who) + ": multivectors are not served by the hybrid solver (one column)").c_str());
      return false;
   }
   return true;
}
}  // namespace

extern "C" {

HYPRE_Int HYPRE_ParCSRHybridCreate(HYPRE_Solver *solver)
{
   if (!solver) { hypre_error_in_arg(1); return hypre_error_flag; }
   hypre_amd_HybridData *d = new hypre_amd_HybridData();
   memset(&d->base, 0, sizeof(d->base));
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridDestroy(HYPRE_Solver solver)
{
   hypre_amd_HybridData *d = D(solver);
   if (!d) { return hypre_error_flag; }
   if (d->amg) { HYPRE_BoomerAMGDestroy(d->amg); }
   destroy_krylov(d);
   delete d;
   return hypre_error_flag;
}

// ---- the solver's own options (amg_hybrid.c:229-700); ranges as the reference checks them
HYPRE_Int HYPRE_ParCSRHybridSetTol(HYPRE_Solver s, HYPRE_Real v)
{ HYBRID_DATA(s, d); if (v < 0 || v > 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetAbsoluteTol(HYPRE_Solver s, HYPRE_Real v)
{ HYBRID_DATA(s, d); if (v < 0 || v > 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->a_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetConvergenceTol(HYPRE_Solver s, HYPRE_Real v)
{ HYBRID_DATA(s, d); if (v < 0 || v > 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->cf_tol = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetDSCGMaxIter(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->dscg_max_its = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetPCGMaxIter(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->pcg_max_its = v; return hypre_error_flag; }
// 0: a preconditioner that exists is kept, and the solve starts with it; anything else builds a new one in every solve
HYPRE_Int HYPRE_ParCSRHybridSetSetupType(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->setup_type = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetSolverType(HYPRE_Solver s, HYPRE_Int v)
{
   HYBRID_DATA(s, d);
   if (v < 1 || v > 3) { return refuse("HYPRE_ParCSRHybridSetSolverType: 1 PCG, 2 GMRES, 3 BiCGSTAB"); }
   d->solver_type = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetKDim(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->k_dim = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetTwoNorm(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->two_norm = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetStopCrit(HYPRE_Solver s, HYPRE_Int v)
{
   HYBRID_DATA(s, d);
   if (v != 0) { return refuse("HYPRE_ParCSRHybridSetStopCrit: the absolute stopping test of the older interface is not carried by PCG and GMRES here (0 only)"); }
   d->stop_crit = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetRelChange(HYPRE_Solver s, HYPRE_Int v)
{
   HYBRID_DATA(s, d);
   if (v != 0) { return refuse("HYPRE_ParCSRHybridSetRelChange: the relative-change stopping test is not built (0 only)"); }
   d->rel_change = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetRecomputeResidual(HYPRE_Solver s, HYPRE_Int v)
{
   HYBRID_DATA(s, d);
   if (v != 0) { return refuse("HYPRE_ParCSRHybridSetRecomputeResidual: 0 only"); }
   d->recompute_residual = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridGetRecomputeResidual(HYPRE_Solver s, HYPRE_Int *v) { HYBRID_DATA(s, d); *v = d->recompute_residual; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver)
{
   (void) s; (void) precond; (void) precond_setup; (void) precond_solver;
   return refuse("HYPRE_ParCSRHybridSetPrecond: a preconditioner of the application's in place of BoomerAMG is not served");
}
HYPRE_Int HYPRE_ParCSRHybridSetLogging(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->logging = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetPrintLevel(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->print_level = v; return hypre_error_flag; }

// ---- the options of the preconditioner (amg_hybrid.c:700-1650): stored here, handed to BoomerAMG when it is created
HYPRE_Int HYPRE_ParCSRHybridSetStrongThreshold(HYPRE_Solver s, HYPRE_Real v)
{ HYBRID_DATA(s, d); if (v < 0 || v > 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->strong_threshold = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetMaxRowSum(HYPRE_Solver s, HYPRE_Real v)
{ HYBRID_DATA(s, d); if (v < 0 || v > 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->max_row_sum = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetTruncFactor(HYPRE_Solver s, HYPRE_Real v)
{ HYBRID_DATA(s, d); if (v < 0 || v > 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->trunc_factor = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetPMaxElmts(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->pmax = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetMaxLevels(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->max_levels = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetMeasureType(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->measure_type = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetCoarsenType(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->coarsen_type = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetInterpType(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->interp_type = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetCycleType(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 1 || v > 2) { hypre_error_in_arg(2); return hypre_error_flag; } d->cycle_type = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetNumSweeps(HYPRE_Solver s, HYPRE_Int v)
{
   HYBRID_DATA(s, d);
   if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   d->num_grid_sweeps.assign(4, v);
   d->num_grid_sweeps[3] = 1;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetCycleNumSweeps(HYPRE_Solver s, HYPRE_Int v, HYPRE_Int k)
{
   HYBRID_DATA(s, d);
   if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   if (k < 1 || k > 3) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (d->num_grid_sweeps.empty()) { d->num_grid_sweeps.assign(4, 1); }
   d->num_grid_sweeps[(size_t) k] = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetRelaxType(HYPRE_Solver s, HYPRE_Int v)
{
   HYBRID_DATA(s, d);
   d->grid_relax_type.assign(4, v);
   d->grid_relax_type[3] = 9;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetCycleRelaxType(HYPRE_Solver s, HYPRE_Int v, HYPRE_Int k)
{
   HYBRID_DATA(s, d);
   if (k < 1 || k > 3) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (d->grid_relax_type.empty()) { d->grid_relax_type = {3, 13, 14, 9}; }
   d->grid_relax_type[(size_t) k] = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetRelaxOrder(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->relax_order = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetKeepTranspose(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->keepT = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetMaxCoarseSize(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->max_coarse_size = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetMinCoarseSize(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->min_coarse_size = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetSeqThreshold(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->seq_threshold = v; return hypre_error_flag; }
// one weight for every level; the level setters start from 1.0 everywhere if nothing was set (amg_hybrid.c:1290-1440)
HYPRE_Int HYPRE_ParCSRHybridSetRelaxWt(HYPRE_Solver s, HYPRE_Real v) { HYBRID_DATA(s, d); d->relax_weight.assign((size_t) d->max_levels, v); return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetOuterWt(HYPRE_Solver s, HYPRE_Real v) { HYBRID_DATA(s, d); d->omega.assign((size_t) d->max_levels, v); return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetLevelRelaxWt(HYPRE_Solver s, HYPRE_Real v, HYPRE_Int level)
{
   HYBRID_DATA(s, d);
   if (level > d->max_levels - 1 || level < 0) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (d->relax_weight.empty()) { d->relax_weight.assign((size_t) d->max_levels, 1.0); }
   d->relax_weight[(size_t) level] = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetLevelOuterWt(HYPRE_Solver s, HYPRE_Real v, HYPRE_Int level)
{
   HYBRID_DATA(s, d);
   if (level > d->max_levels - 1 || level < 0) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (d->omega.empty()) { d->omega.assign((size_t) d->max_levels, 1.0); }
   d->omega[(size_t) level] = v;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ParCSRHybridSetNumPaths(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->num_paths = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetAggNumLevels(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 0) { hypre_error_in_arg(2); return hypre_error_flag; } d->agg_num_levels = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetAggInterpType(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->agg_interp_type = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetNumFunctions(HYPRE_Solver s, HYPRE_Int v)
{ HYBRID_DATA(s, d); if (v < 1) { hypre_error_in_arg(2); return hypre_error_flag; } d->num_functions = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetNodal(HYPRE_Solver s, HYPRE_Int v) { HYBRID_DATA(s, d); d->nodal = v; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridSetNonGalerkinTol(HYPRE_Solver s, HYPRE_Int num, HYPRE_Real *tols)
{
   HYBRID_DATA(s, d);
   if (num < 0) { hypre_error_in_arg(2); return hypre_error_flag; }
   d->nongalerkin_tol.assign(tols, tols + (tols ? num : 0));
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRHybridGetNumIterations(HYPRE_Solver s, HYPRE_Int *v) { HYBRID_DATA(s, d); *v = d->dscg_num_its + d->pcg_num_its; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridGetDSCGNumIterations(HYPRE_Solver s, HYPRE_Int *v) { HYBRID_DATA(s, d); *v = d->dscg_num_its; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridGetPCGNumIterations(HYPRE_Solver s, HYPRE_Int *v) { HYBRID_DATA(s, d); *v = d->pcg_num_its; return hypre_error_flag; }
// stored with logging on only, as the reference does (amg_hybrid.c:2073-2076, 2243-2247)
HYPRE_Int HYPRE_ParCSRHybridGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *v) { HYBRID_DATA(s, d); *v = d->final_rel_res_norm; return hypre_error_flag; }
HYPRE_Int HYPRE_ParCSRHybridGetSetupSolveTime(HYPRE_Solver s, HYPRE_Real *time)
{
   HYBRID_DATA(s, d);
   for (int k = 0; k < 4; k++) { time[k] = d->times[k]; }
   return hypre_error_flag;
}
// the pieces, for a caller that wants to look at them: the Krylov solver (of solver_type) and the hierarchy, null while
// the solver has not needed one; whether the diagonally scaled PCG phase of the last solve took the fused step
HYPRE_Int hypre_amd_ParCSRHybridGetPrecond(HYPRE_Solver s, HYPRE_Solver *amg) { HYBRID_DATA(s, d); *amg = d->amg; return hypre_error_flag; }
HYPRE_Int hypre_amd_ParCSRHybridGetKrylovSolver(HYPRE_Solver s, HYPRE_Solver *krylov) { HYBRID_DATA(s, d); *krylov = d->krylov; return hypre_error_flag; }

// amg_hybrid.c:1690-1700 does nothing in Setup; the operands are looked at, so that a host operand is refused here already
HYPRE_Int HYPRE_ParCSRHybridSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   HYBRID_DATA(solver, d);
   (void) d;
   if (!A) { hypre_error_in_arg(2); return hypre_error_flag; }
   if (!b) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (!x) { hypre_error_in_arg(4); return hypre_error_flag; }
   operands_fit("HYPRE_ParCSRHybridSetup", A, b, x);
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ParCSRHybridSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   HYBRID_DATA(solver, d);
   if (!b) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (!A) { hypre_error_in_arg(2); return hypre_error_flag; }
   if (!x) { hypre_error_in_arg(4); return hypre_error_flag; }
   if (!operands_fit("HYPRE_ParCSRHybridSolve", A, b, x)) { return hypre_error_flag; }
   for (int k = 0; k < 4; k++) { d->times[k] = 0.0; }
   // an error raised in here, other than "not converged", ends the solve where it stands
   const HYPRE_Int flags_before = hypre_error_flag;
   auto failed = [&] { return ((hypre_error_flag & ~flags_before) & ~HYPRE_ERROR_CONV) != 0; };
   // print_level xy: y for the Krylov solver, x for the preconditioner
   const HYPRE_Int pre_print_level = d->print_level / 10, sol_print_level = d->print_level - pre_print_level * 10;
   if (d->krylov && d->krylov_type != d->solver_type) { destroy_krylov(d); }       // the solver type was changed between solves
   const KrylovCalls &K = calls_of(d->solver_type);
   HYPRE_Int converged = 0;
   HYPRE_Real res_norm = 0.0;
   d->dscg_num_its = 0;
   d->pcg_num_its = 0;

   // the diagonally scaled phase (amg_hybrid.c:1866-2066), skipped when a preconditioner is to be kept
   if (d->setup_type || d->amg == nullptr)
   {
      if (d->amg) { HYPRE_BoomerAMGDestroy(d->amg); d->amg = nullptr; }
      double t1 = wall_seconds();
      if (!d->krylov) { create_krylov(d, A->comm, sol_print_level); }
      K.set_hybrid(d->krylov, -1);
      K.set_max_iter(d->krylov, d->dscg_max_its);
      K.set_cf_tol(d->krylov, d->cf_tol);
      K.set_precond(d->krylov, (HYPRE_PtrToSolverFcn) HYPRE_ParCSRDiagScale, (HYPRE_PtrToSolverFcn) HYPRE_ParCSRDiagScaleSetup, nullptr);
      K.setup(d->krylov, A, b, x);
      double t2 = wall_seconds();
      d->times[0] = t2 - t1;
      K.solve(d->krylov, A, b, x);
      K.get_its(d->krylov, &d->dscg_num_its);
      K.get_norm(d->krylov, &res_norm);
      K.get_converged(d->krylov, &converged);
      d->times[1] = wall_seconds() - t2;
   }
   if (converged)
   {
      if (d->logging) { d->final_rel_res_norm = res_norm; }
      return hypre_error_flag;
   }
   if (failed()) { return hypre_error_flag; }           // a refusal or a breakdown: nothing to go on with

   // ... otherwise the same solver behind BoomerAMG, from the current x (amg_hybrid.c:2081-2310)
   double t1 = wall_seconds();
   if (!d->krylov) { create_krylov(d, A->comm, sol_print_level); }
   K.set_max_iter(d->krylov, d->pcg_max_its);
   K.set_cf_tol(d->krylov, 0.0);
   K.set_hybrid(d->krylov, 0);
   if (d->amg == nullptr)
   {
      d->amg = create_amg(d, pre_print_level);
      if (failed())                                     // an option this library does not build: its gate has spoken
      {
         HYPRE_BoomerAMGDestroy(d->amg); d->amg = nullptr;
         return hypre_error_flag;
      }
      K.set_precond(d->krylov, (HYPRE_PtrToSolverFcn) HYPRE_BoomerAMGSolve, (HYPRE_PtrToSolverFcn) HYPRE_BoomerAMGSetup, d->amg);
   }
   else
   {
      // setup_type 0 with a hierarchy from an earlier solve: BoomerAMGSetup with setup_type 0 returns at once in the
      // reference (par_amg_setup.c:306), so no setup function is handed on
      K.set_precond(d->krylov, (HYPRE_PtrToSolverFcn) HYPRE_BoomerAMGSolve, nullptr, d->amg);
   }
   K.setup(d->krylov, A, b, x);
   double t2 = wall_seconds();
   d->times[2] = t2 - t1;
   if (failed()) { return hypre_error_flag; }
   K.solve(d->krylov, A, b, x);
   K.get_its(d->krylov, &d->pcg_num_its);
   if (d->logging)
   {
      K.get_norm(d->krylov, &res_norm);
      d->final_rel_res_norm = res_norm;
   }
   d->times[3] = wall_seconds() - t2;
   return hypre_error_flag;
}

}  // extern "C"
