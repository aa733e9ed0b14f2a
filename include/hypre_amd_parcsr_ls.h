/*
 * hypre_amd — BoomerAMG: relaxation, V-cycle, solve (the hot path), plus the
 * host-side setup that produces the hierarchy the cycle runs on, and the PCG
 * caller.
 *
 * Functions replace (paths relative to /root/reference/src):
 *   parcsr_ls/par_relax.c:24-173               hypre_BoomerAMGRelax (dispatcher)
 *   parcsr_ls/par_relax.c:1178-1254,180-369    Jacobi / l1-Jacobi (relax 7, 18, 0)
 *   parcsr_ls/par_relax.c:1506-1666, par_relax_device.c:97-155   two-stage GS (11, 12)
 *   parcsr_ls/par_relax.c:691-1377, par_relax_device.c:19-90     hybrid GS family (3,4,6,8,13,14,88,89)
 *   parcsr_ls/par_relax_interface.c:20-117     hypre_BoomerAMGRelaxIF, L1_Jacobi, FCFJacobi
 *   parcsr_ls/par_cycle.c:23-803               hypre_BoomerAMGCycle
 *   parcsr_ls/par_amg_solve.c:22-424           hypre_BoomerAMGSolve
 *   parcsr_ls/HYPRE_parcsr_amg.c:64-91         HYPRE_BoomerAMGSolve
 *   parcsr_ls/par_gauss_elim.c:457-697         hypre_GaussElimSolve (coarsest level)
 *   parcsr_ls/ams.c:527-830                    hypre_ParCSRComputeL1Norms
 *   parcsr_ls/par_amg.c / HYPRE_parcsr_amg.c   Create / Destroy / Set* / Get*
 *   parcsr_ls/par_amg_setup.c:28-4046          hypre_BoomerAMGSetup (host; "next" row of the scope table)
 *   krylov/pcg.c:318-1000 + parcsr_ls/HYPRE_parcsr_pcg.c   PCG with a BoomerAMG preconditioner
 *
 * hypre_ParAMGData below is the solve- and setup-relevant SLICE of the
 * reference struct (parcsr_ls/par_amg.h:19-295): member names and the
 * accessor macros match, the byte layout does not (the reference struct
 * carries ~250 members for solvers outside this path).  Code that touches
 * the solver object only through the HYPRE_BoomerAMG* calls or the
 * hypre_ParAMGData* macros is source compatible; see INTEGRATION.md.
 */
#ifndef HYPRE_AMD_PARCSR_LS_H
#define HYPRE_AMD_PARCSR_LS_H

#include "hypre_amd_parcsr_mv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
   hypre_Solver          base;               /* setup / solve / destroy */
   HYPRE_MemoryLocation  memory_location;    /* where the hierarchy lives after setup */

   /* setup parameters (par_amg.c:162-316 defaults) */
   HYPRE_Int      max_levels;
   HYPRE_Real     strong_threshold;
   HYPRE_Real     max_row_sum;
   HYPRE_Real     trunc_factor;
   HYPRE_Int      measure_type;
   HYPRE_Int      coarsen_type;              /* 8 PMIS, 9 PMIS(seq rand), 10 HMIS */
   HYPRE_Int      P_max_elmts;
   HYPRE_Int      interp_type;               /* 6 ext+i, 3 direct */
   HYPRE_Int      agg_num_levels;
   HYPRE_Int      max_coarse_size;
   HYPRE_Int      min_coarse_size;
   HYPRE_Int      keepTranspose;
   HYPRE_Int      num_functions;

   /* solve parameters */
   HYPRE_Int      max_iter;
   HYPRE_Int      min_iter;
   HYPRE_Int      fcycle;
   HYPRE_Int      cycle_type;
   HYPRE_Int     *num_grid_sweeps;           /* [4] */
   HYPRE_Int     *grid_relax_type;           /* [4] */
   HYPRE_Int    **grid_relax_points;         /* NULL unless set by the user */
   HYPRE_Int      relax_order;
   HYPRE_Int      user_coarse_relax_type;
   HYPRE_Int      user_relax_type;
   HYPRE_Int      user_num_sweeps;
   HYPRE_Real     user_relax_weight;
   HYPRE_Real     outer_wt;
   HYPRE_Real    *relax_weight;              /* [max_levels] */
   HYPRE_Real    *omega;                     /* [max_levels] */
   HYPRE_Int      converge_type;
   HYPRE_Real     tol;

   /* hierarchy */
   hypre_ParCSRMatrix  *A;
   hypre_ParCSRMatrix **A_array;
   hypre_ParVector    **F_array;
   hypre_ParVector    **U_array;
   hypre_ParCSRMatrix **P_array;
   hypre_ParCSRMatrix **R_array;             /* == P_array (restriction is P^T) */
   hypre_IntArray     **CF_marker_array;
   HYPRE_Int            num_levels;
   hypre_Vector       **l1_norms;

   /* work vectors (fine-grid sized, re-sized per level in place) */
   hypre_ParVector   *Vtemp;
   hypre_ParVector   *Rtemp;
   hypre_ParVector   *Ptemp;
   hypre_ParVector   *Ztemp;
   HYPRE_Real         cycle_op_count;

   /* coarsest-level dense solve (par_gauss_elim.c) */
   HYPRE_Int          gs_setup;
   HYPRE_Real        *A_mat;                 /* dense coarse operator, row major, host */
   HYPRE_Real        *b_vec;

   /* log */
   HYPRE_Int        logging;
   HYPRE_Int        num_iterations;
   HYPRE_Real       rel_resid_norm;
   HYPRE_Int        print_level;
   HYPRE_Int        debug_flag;

   /* Chebyshev smoothing, relax 16 (par_amg.h:208-217; defaults par_amg.c:273-277) */
   HYPRE_Int        cheby_order;             /* 1..4, default 2 */
   HYPRE_Int        cheby_eig_est;           /* CG iterations of the estimate, 0 = Gershgorin; default 10 */
   HYPRE_Int        cheby_variant;           /* 0 standard, 1 modified */
   HYPRE_Int        cheby_scale;             /* 1: smooth D^-1/2 A D^-1/2 */
   HYPRE_Real       cheby_fraction;          /* part of the spectrum that is damped, default 0.3 */
   HYPRE_Real      *max_eig_est;             /* [num_levels] */
   HYPRE_Real      *min_eig_est;
   hypre_Vector   **cheby_ds;                /* [num_levels] 1/sqrt(|a_ii|) */
   HYPRE_Real     **cheby_coefs;             /* [num_levels][order + 1], host */

   /* library-private state (device plans, graphs, mixed-precision copies) */
   void            *amd_private;
} hypre_ParAMGData;

#define hypre_ParAMGDataMemoryLocation(d)   ((d)->memory_location)
#define hypre_ParAMGDataMaxLevels(d)        ((d)->max_levels)
#define hypre_ParAMGDataStrongThreshold(d)  ((d)->strong_threshold)
#define hypre_ParAMGDataMaxRowSum(d)        ((d)->max_row_sum)
#define hypre_ParAMGDataTruncFactor(d)      ((d)->trunc_factor)
#define hypre_ParAMGDataCoarsenType(d)      ((d)->coarsen_type)
#define hypre_ParAMGDataPMaxElmts(d)        ((d)->P_max_elmts)
#define hypre_ParAMGDataInterpType(d)       ((d)->interp_type)
#define hypre_ParAMGDataMaxCoarseSize(d)    ((d)->max_coarse_size)
#define hypre_ParAMGDataMinCoarseSize(d)    ((d)->min_coarse_size)
#define hypre_ParAMGDataKeepTranspose(d)    ((d)->keepTranspose)
#define hypre_ParAMGDataMaxIter(d)          ((d)->max_iter)
#define hypre_ParAMGDataMinIter(d)          ((d)->min_iter)
#define hypre_ParAMGDataFCycle(d)           ((d)->fcycle)
#define hypre_ParAMGDataCycleType(d)        ((d)->cycle_type)
#define hypre_ParAMGDataNumGridSweeps(d)    ((d)->num_grid_sweeps)
#define hypre_ParAMGDataGridRelaxType(d)    ((d)->grid_relax_type)
#define hypre_ParAMGDataGridRelaxPoints(d)  ((d)->grid_relax_points)
#define hypre_ParAMGDataRelaxOrder(d)       ((d)->relax_order)
#define hypre_ParAMGDataUserRelaxType(d)    ((d)->user_relax_type)
#define hypre_ParAMGDataRelaxWeight(d)      ((d)->relax_weight)
#define hypre_ParAMGDataOmega(d)            ((d)->omega)
#define hypre_ParAMGDataConvergeType(d)     ((d)->converge_type)
#define hypre_ParAMGDataTol(d)              ((d)->tol)
#define hypre_ParAMGDataAArray(d)           ((d)->A_array)
#define hypre_ParAMGDataFArray(d)           ((d)->F_array)
#define hypre_ParAMGDataUArray(d)           ((d)->U_array)
#define hypre_ParAMGDataPArray(d)           ((d)->P_array)
#define hypre_ParAMGDataRArray(d)           ((d)->R_array)
#define hypre_ParAMGDataCFMarkerArray(d)    ((d)->CF_marker_array)
#define hypre_ParAMGDataNumLevels(d)        ((d)->num_levels)
#define hypre_ParAMGDataL1Norms(d)          ((d)->l1_norms)
#define hypre_ParAMGDataVtemp(d)            ((d)->Vtemp)
#define hypre_ParAMGDataRtemp(d)            ((d)->Rtemp)
#define hypre_ParAMGDataPtemp(d)            ((d)->Ptemp)
#define hypre_ParAMGDataZtemp(d)            ((d)->Ztemp)
#define hypre_ParAMGDataCycleOpCount(d)     ((d)->cycle_op_count)
#define hypre_ParAMGDataNumIterations(d)    ((d)->num_iterations)
#define hypre_ParAMGDataRelativeResidualNorm(d) ((d)->rel_resid_norm)
#define hypre_ParAMGDataPrintLevel(d)       ((d)->print_level)
#define hypre_ParAMGDataLogging(d)          ((d)->logging)
#define hypre_ParAMGDataChebyOrder(d)       ((d)->cheby_order)
#define hypre_ParAMGDataChebyEigEst(d)      ((d)->cheby_eig_est)
#define hypre_ParAMGDataChebyVariant(d)     ((d)->cheby_variant)
#define hypre_ParAMGDataChebyScale(d)       ((d)->cheby_scale)
#define hypre_ParAMGDataChebyFraction(d)    ((d)->cheby_fraction)
#define hypre_ParAMGDataMaxEigEst(d)        ((d)->max_eig_est)
#define hypre_ParAMGDataMinEigEst(d)        ((d)->min_eig_est)
#define hypre_ParAMGDataChebyDS(d)          ((d)->cheby_ds)
#define hypre_ParAMGDataChebyCoefs(d)       ((d)->cheby_coefs)

/* ---- life cycle and parameters (HYPRE_parcsr_amg.c) ---- */
HYPRE_Int HYPRE_BoomerAMGCreate(HYPRE_Solver *solver);
HYPRE_Int HYPRE_BoomerAMGDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_BoomerAMGSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_BoomerAMGSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_BoomerAMGSetMaxLevels(HYPRE_Solver solver, HYPRE_Int max_levels);
HYPRE_Int HYPRE_BoomerAMGSetMaxCoarseSize(HYPRE_Solver solver, HYPRE_Int max_coarse_size);
HYPRE_Int HYPRE_BoomerAMGSetMinCoarseSize(HYPRE_Solver solver, HYPRE_Int min_coarse_size);
HYPRE_Int HYPRE_BoomerAMGSetStrongThreshold(HYPRE_Solver solver, HYPRE_Real strong_threshold);
HYPRE_Int HYPRE_BoomerAMGSetMaxRowSum(HYPRE_Solver solver, HYPRE_Real max_row_sum);
HYPRE_Int HYPRE_BoomerAMGSetCoarsenType(HYPRE_Solver solver, HYPRE_Int coarsen_type);
HYPRE_Int HYPRE_BoomerAMGSetInterpType(HYPRE_Solver solver, HYPRE_Int interp_type);
HYPRE_Int HYPRE_BoomerAMGSetTruncFactor(HYPRE_Solver solver, HYPRE_Real trunc_factor);
HYPRE_Int HYPRE_BoomerAMGSetPMaxElmts(HYPRE_Solver solver, HYPRE_Int P_max_elmts);
HYPRE_Int HYPRE_BoomerAMGSetKeepTranspose(HYPRE_Solver solver, HYPRE_Int keepTranspose);
/* systems of PDEs, "unknown" approach (HYPRE_parcsr_amg.c HYPRE_BoomerAMGSetNumFunctions; par_strength.c:248-403,
 * par_lr_interp.c:1706-1713): row i belongs to function (global row) mod num_functions, couplings between
 * different functions are neither strong nor lumped.  ext+i interpolation only. */
HYPRE_Int HYPRE_BoomerAMGSetNumFunctions(HYPRE_Solver solver, HYPRE_Int num_functions);
/* par_amg.c:3232-3250, par_amg_setup.c:774-780, parcsr_mv/par_csr_filter.c:21-186: with num_functions > 1, build
 * the hierarchy from A without its inter-function couplings (`ij -ff 1`); level 0 is still smoothed with A */
HYPRE_Int HYPRE_BoomerAMGSetFilterFunctions(HYPRE_Solver solver, HYPRE_Int filter_functions);
/* Chebyshev smoother parameters (HYPRE_parcsr_amg.c:1340-1400 -> par_amg.c:4583-4670) */
HYPRE_Int HYPRE_BoomerAMGSetChebyOrder(HYPRE_Solver solver, HYPRE_Int order);
HYPRE_Int HYPRE_BoomerAMGSetChebyFraction(HYPRE_Solver solver, HYPRE_Real ratio);
HYPRE_Int HYPRE_BoomerAMGSetChebyEigEst(HYPRE_Solver solver, HYPRE_Int eig_est);
HYPRE_Int HYPRE_BoomerAMGSetChebyVariant(HYPRE_Solver solver, HYPRE_Int variant);
HYPRE_Int HYPRE_BoomerAMGSetChebyScale(HYPRE_Solver solver, HYPRE_Int scale);
HYPRE_Int HYPRE_BoomerAMGSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_BoomerAMGSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_BoomerAMGSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_BoomerAMGSetConvergeType(HYPRE_Solver solver, HYPRE_Int type);
HYPRE_Int HYPRE_BoomerAMGSetCycleType(HYPRE_Solver solver, HYPRE_Int cycle_type);
HYPRE_Int HYPRE_BoomerAMGSetFCycle(HYPRE_Solver solver, HYPRE_Int fcycle);
HYPRE_Int HYPRE_BoomerAMGSetNumSweeps(HYPRE_Solver solver, HYPRE_Int num_sweeps);
HYPRE_Int HYPRE_BoomerAMGSetCycleNumSweeps(HYPRE_Solver solver, HYPRE_Int num_sweeps, HYPRE_Int k);
HYPRE_Int HYPRE_BoomerAMGSetRelaxType(HYPRE_Solver solver, HYPRE_Int relax_type);
HYPRE_Int HYPRE_BoomerAMGSetCycleRelaxType(HYPRE_Solver solver, HYPRE_Int relax_type, HYPRE_Int k);
HYPRE_Int HYPRE_BoomerAMGSetRelaxOrder(HYPRE_Solver solver, HYPRE_Int relax_order);
HYPRE_Int HYPRE_BoomerAMGSetRelaxWt(HYPRE_Solver solver, HYPRE_Real relax_weight);
HYPRE_Int HYPRE_BoomerAMGSetOuterWt(HYPRE_Solver solver, HYPRE_Real omega);
/* parcsr_ls/HYPRE_parcsr_amg.c:560-600 -> par_amg.c:2466,2590: weight of one level, overriding the uniform value */
HYPRE_Int HYPRE_BoomerAMGSetLevelRelaxWt(HYPRE_Solver solver, HYPRE_Real relax_weight, HYPRE_Int level);
HYPRE_Int HYPRE_BoomerAMGSetLevelOuterWt(HYPRE_Solver solver, HYPRE_Real omega, HYPRE_Int level);
HYPRE_Int HYPRE_BoomerAMGSetPrintLevel(HYPRE_Solver solver, HYPRE_Int print_level);
HYPRE_Int HYPRE_BoomerAMGSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
/* Option gates (HYPRE_parcsr_amg.c): setters an application written against hypre calls routinely, for options whose
 * other branches are outside this library.  The value that selects what is implemented here is accepted (named in each
 * comment); any other value raises HYPRE_ERROR_ARG(2) with a message.  SetDebugFlag / SetNumPaths are accepted and inert. */
HYPRE_Int HYPRE_BoomerAMGSetMeasureType(HYPRE_Solver solver, HYPRE_Int measure_type);          /* 0 local, 1 global */
HYPRE_Int HYPRE_BoomerAMGSetDebugFlag(HYPRE_Solver solver, HYPRE_Int debug_flag);
HYPRE_Int HYPRE_BoomerAMGSetNumPaths(HYPRE_Solver solver, HYPRE_Int num_paths);
HYPRE_Int HYPRE_BoomerAMGSetAggNumLevels(HYPRE_Solver solver, HYPRE_Int agg_num_levels);       /* 0 */
HYPRE_Int HYPRE_BoomerAMGSetNodal(HYPRE_Solver solver, HYPRE_Int nodal);                       /* 0 */
HYPRE_Int HYPRE_BoomerAMGSetSeqThreshold(HYPRE_Solver solver, HYPRE_Int seq_threshold);        /* 0 */
HYPRE_Int HYPRE_BoomerAMGSetRedundant(HYPRE_Solver solver, HYPRE_Int redundant);               /* 0 */
HYPRE_Int HYPRE_BoomerAMGSetRAP2(HYPRE_Solver solver, HYPRE_Int rap2);                         /* 0 */
HYPRE_Int HYPRE_BoomerAMGSetRestriction(HYPRE_Solver solver, HYPRE_Int restr_par);             /* 0 */
/* ILU as a level smoother (par_cycle.c:293-326, 477-483, 614-636; defaults smooth_type 6, smooth_num_levels 0,
 * smooth_num_sweeps 1).  Of the reference's complex smoothers only ILU is built: smooth_type 5 applies HYPRE_ILUSolve
 * smooth_num_sweeps times on every level < smooth_num_levels in place of the relaxation (the coarsest level's direct solve
 * included when the count reaches it); 15 wraps smooth_num_sweeps conjugate-gradient steps around num_grid_sweeps ILU
 * applications from zero.  ORDER: SetSmoothType comes before SetSmoothNumLevels — a positive level count is accepted only
 * while the stored type is 5 or 15, and a type other than these is refused while the count is positive (HYPRE_ERROR_ARG(2)
 * with a message); every type is accepted while the count is 0 and has no effect then.  One rank, one column, fp64
 * hierarchy: anything else is refused by Setup with a message.  Deviation: where the reference's acceleration divides
 * 0 by 0 (gamma = <R, Z> exactly 0: a zero right-hand side) and fills U with NaN, the visit ends and U stays. */
HYPRE_Int HYPRE_BoomerAMGSetSmoothNumLevels(HYPRE_Solver solver, HYPRE_Int smooth_num_levels); /* 0; > 0 with type 5 | 15 */
HYPRE_Int HYPRE_BoomerAMGSetSmoothType(HYPRE_Solver solver, HYPRE_Int smooth_type);
HYPRE_Int HYPRE_BoomerAMGSetSmoothNumSweeps(HYPRE_Solver solver, HYPRE_Int smooth_num_sweeps); /* >= 1 */
/* Parameters of the level smoothers (par_amg.c:223-231: type 0, level 0, max_row_nnz 20, max_iter 1, droptol 0.01,
 * tri_solve 1, 5 and 5 Jacobi iterations, reordering 1), handed on by Setup as par_amg_setup.c:3710-3726 hands them on. */
HYPRE_Int HYPRE_BoomerAMGSetILUType(HYPRE_Solver solver, HYPRE_Int ilu_type);                  /* 0 */
HYPRE_Int HYPRE_BoomerAMGSetILULevel(HYPRE_Solver solver, HYPRE_Int ilu_lfil);                 /* >= 0 */
HYPRE_Int HYPRE_BoomerAMGSetILULocalReordering(HYPRE_Solver solver, HYPRE_Int ilu_reordering_type);   /* 0 none, 1 RCM */
HYPRE_Int HYPRE_BoomerAMGSetILUMaxIter(HYPRE_Solver solver, HYPRE_Int ilu_max_iter);           /* applications per HYPRE_ILUSolve */
/* 1 direct, 0 Jacobi sweeps: the reference's meaning (hypre_amd_ILUSetIterativeTriSolve(.., 1) on the level smoothers;
 * HYPRE_ILUSetTriSolve(.., 0) itself stays refused) */
HYPRE_Int HYPRE_BoomerAMGSetILUTriSolve(HYPRE_Solver solver, HYPRE_Int ilu_tri_solve);
HYPRE_Int HYPRE_BoomerAMGSetILULowerJacobiIters(HYPRE_Solver solver, HYPRE_Int ilu_lower_jacobi_iters);   /* >= 0 */
HYPRE_Int HYPRE_BoomerAMGSetILUUpperJacobiIters(HYPRE_Solver solver, HYPRE_Int ilu_upper_jacobi_iters);   /* >= 0 */
HYPRE_Int HYPRE_BoomerAMGSetILUDroptol(HYPRE_Solver solver, HYPRE_Real ilu_droptol);           /* stored; no effect for type 0 */
HYPRE_Int HYPRE_BoomerAMGSetILUMaxRowNnz(HYPRE_Solver solver, HYPRE_Int ilu_max_row_nnz);      /* stored; no effect for type 0 */
HYPRE_Int HYPRE_BoomerAMGSetILUIterSetupType(HYPRE_Solver solver, HYPRE_Int ilu_iter_setup_type);   /* 0 */
/* the HYPRE_ILU object of a level (NULL where the level has none): parameters and launch statistics through hypre_amd_ILUGet* */
HYPRE_Int hypre_amd_BoomerAMGGetSmoother(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Solver *ilu);
/* the settings as they stand; of the last cycle, the level visits the smoother served and the reductions read back to the
 * host inside them (0 with hypre_amd_SetSmootherFusion on); any pointer may be NULL */
HYPRE_Int hypre_amd_BoomerAMGGetSmootherStats(HYPRE_Solver solver, HYPRE_Int *smooth_type, HYPRE_Int *smooth_num_levels,
                                              HYPRE_Int *smooth_num_sweeps, HYPRE_Int *visits, HYPRE_Int *readbacks);
/* smooth_type 15 with both inner products left on the device (default 1) or as the reference's call sequence with two
 * read-backs per sweep (0); same bits.  on < 0: unchanged; returns the setting. */
HYPRE_Int hypre_amd_SetSmootherFusion(HYPRE_Int on);
/* the vector kernels of the fused acceleration on their own (tests): `scalars` holds gamma, gammaold, <P, V>, stop flag.
 * Direction: P = Z (first) or Z + (gamma / gammaold) P; update: U += alfa P, R -= alfa V with alfa = gamma / <P, V>, and
 * Z = 0 when zero_z; both leave everything as it is when the stop flag is not 0.  Dot: scalars[which ? 2 : 0] = <x, y>
 * (which 0 moves gamma to gammaold first and raises the stop flag at a sum of exactly 0).  Host arrays in and out. */
HYPRE_Int hypre_amd_ILUSmootherKernelTest(HYPRE_Int n, HYPRE_Real *scalars, HYPRE_Int first, HYPRE_Int zero_z, HYPRE_Int with_dots,
                                          HYPRE_Real *U, HYPRE_Real *R, HYPRE_Real *P, HYPRE_Real *Z, const HYPRE_Real *V);
HYPRE_Int HYPRE_BoomerAMGSetAdditive(HYPRE_Solver solver, HYPRE_Int addlvl);                   /* -1 */
HYPRE_Int HYPRE_BoomerAMGSetMultAdditive(HYPRE_Solver solver, HYPRE_Int addlvl);               /* -1 */
HYPRE_Int HYPRE_BoomerAMGSetSimple(HYPRE_Solver solver, HYPRE_Int addlvl);                     /* -1 */
HYPRE_Int HYPRE_BoomerAMGSetNonGalerkinTol(HYPRE_Solver solver, HYPRE_Real nongalerkin_tol);   /* 0.0 */
HYPRE_Int HYPRE_BoomerAMGSetADropTol(HYPRE_Solver solver, HYPRE_Real A_drop_tol);              /* 0.0 */
HYPRE_Int HYPRE_BoomerAMGGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_BoomerAMGGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *rel_resid_norm);

/* library extensions (no reference counterpart) */
/* memory location the hierarchy is placed in by Setup (default: device) */
HYPRE_Int hypre_amd_BoomerAMGSetMemoryLocation(HYPRE_Solver solver, HYPRE_MemoryLocation location);
/* OpenMP thread count the host setup emulates in its thread-partitioned loops
 * (0 = 1; results of the hybrid smoothers' block partition depend on it) */
HYPRE_Int hypre_amd_BoomerAMGSetNumThreads(HYPRE_Solver solver, HYPRE_Int num_threads);
/* Where the Galerkin products of HYPRE_BoomerAMGSetup are formed when the hierarchy's home is device memory and there is
 * one rank: on the device by default (rap_kernels.hip; same columns, order and bits as the host loop), on = 0 keeps the
 * host loop; min_rows: smallest fine level sent to the device (default 20000).  Negative arguments leave a setting
 * unchanged.  Returns the number of products formed on the device since the previous call.  The reference's device setup:
 * parcsr_mv/par_csr_triplemat.c:938-960.  Test switch: on = 2 makes a standalone call of
 * hypre_BoomerAMGBuildCoarseOperatorKT (one rank, RT == P, at least min_rows fine rows) form the product on the device as
 * well; the result's diagonal block (and the stored transpose) then live in device memory. */
HYPRE_Int hypre_amd_SetSetupDeviceRAP(HYPRE_Int on, HYPRE_Int min_rows);
/* Test switches of the device Galerkin product (single-rank and distributed): first_RA / first_O set the table sizes of
 * its first attempt (entries of the intermediate row R*A and of the output row) instead of the pilot's estimate;
 * scratch_limit (bytes) replaces the budget of the strided scratch of the one-walk form — 0 sends the single-rank product
 * to the two-walk form (lengths, then columns and values) and the distributed one, which has no two-walk form, to the
 * host.  -1 restores the default of an argument. */
HYPRE_Int hypre_amd_SetDeviceRapTables(HYPRE_Int first_RA, HYPRE_Int first_O, long long scratch_limit);
/* How the last device Galerkin product was attempted: pilot = 1 if a pilot walk sized the tables, attempts = walks of
 * the first pass, two_walks = 1 for the two-walk form, fell_back = 1 if the product was left to the host loop.  Any
 * pointer may be NULL. */
HYPRE_Int hypre_amd_GetDeviceRapPath(HYPRE_Int *pilot, HYPRE_Int *attempts, HYPRE_Int *two_walks, HYPRE_Int *fell_back);
/* The same for the extended+i interpolation operators (interp_kernels.hip; scalar problems, levels of at least min_rows
 * rows): on = 0 keeps the host loop; on = 1 + k starts the kernel's ladder of table sizes (64, 128, 256, 1024 entries per
 * row; an overflowing row moves everyone up) at rung k — the results do not depend on it, tests walk the rungs; returns
 * the number built on the device since the previous call.  The reference's device routine:
 * parcsr_ls/par_lr_interp_device.c:1001. */
HYPRE_Int hypre_amd_SetSetupDeviceInterp(HYPRE_Int on);
/* How the last call of the device interpolation kernel went, five numbers: out[0] the first rung tried, out[1] the rung
 * that held every row (-1: none), out[2] the attempts made, out[3] the storage mode (0: one pass into rows of fixed
 * stride, P_max_elmts > 0 or a distributed level; 1: lengths first, then columns and values), out[4] why the kernel
 * declined and left the level to the host loop (0: it did not; 1: truncation by threshold alone, P_max_elmts = 0 with
 * trunc_factor > 0; 2: a row fits no rung — more than 1024 points in its interpolatory set, or so many strong
 * neighbours that they and the set could fill the row's map; 3: an allocation failed). */
HYPRE_Int hypre_amd_GetDeviceInterpPath(HYPRE_Int *out);
/* Test switch: the number of waves (one per row in flight) the interpolation kernel is launched with; 0 restores the
 * default, min(rows, 32 per compute unit).  With a few waves over many rows one wave walks many rows, each under a new
 * tag, past the slots its earlier rows left in the map. */
HYPRE_Int hypre_amd_SetDeviceInterpWaves(HYPRE_Int waves);
/* And for strength of connection, PMIS coarsening and the smoother diagonals (setup_kernels.hip; the HOST routines'
 * measures and results, not the reference's device variant with its own random numbers): with all three switches on, a
 * single-rank scalar level of at least min_rows rows is set up without leaving the device — the coarse operator is not
 * fetched, and a matrix handed over in device memory is not copied to the host.  on = 0 keeps the host loops; returns the
 * number of levels coarsened on the device since the previous call.  The reference's device routines:
 * parcsr_ls/par_strength_device.c, parcsr_ls/par_coarsen_device.c:30. */
HYPRE_Int hypre_amd_SetSetupDeviceCoarsen(HYPRE_Int on);
/* Levels of a DISTRIBUTED hierarchy (several ranks, one per GPU) are set up on the device as well when the three switches
 * above are on and a level has at least min_rows rows per rank on average: the single-rank kernels run on the extended
 * numbering [local points | ghost points], fed with the rows the host routines exchange (A_ext, S_ext, P_ext, the product
 * rows computed for the neighbours, the PMIS halo rounds); results equal the host routines' array for array.  on = 0 keeps
 * distributed levels on the host (OpenMP loops); negative: unchanged.  Returns the previous setting.  The reference's device
 * routines: par_coarsen_device.c:30, par_lr_interp_device.c:1001, parcsr_mv/par_csr_triplemat.c:938-960. */
HYPRE_Int hypre_amd_SetSetupDeviceDist(HYPRE_Int on);
/* Test hook of the distributed device setup: rank `rank` pretends, `count` times, that the device kernel of step `what`
 * (1 interpolation, 2 product rows made for the neighbours, 3 Galerkin product) could not fit a row into its tables.  Every
 * rank then repeats that step with the host routine — the agreed fall-back, which real problems reach only through rows of
 * more than a thousand entries. */
HYPRE_Int hypre_amd_SetupDistTestDecline(HYPRE_Int what, HYPRE_Int rank, HYPRE_Int count);
/* The coarse tail of a single-rank V-cycle (levels of at most `rows` rows; 0: off) can be recorded once as a HIP graph and
 * replayed: its kernels are a few microseconds each behind launches that cost as much.  Off by default since the end of
 * round 4 (environment HYPRE_AMD_CYCLE_GRAPH_ROWS=100000 or this call switch it on): with the smallest levels in one kernel
 * (hypre_amd_SetSmallTail) the tail is 13 - 25 launches the host runs ahead of anyway, and eager cycles measured 0.5 - 1.4 %
 * faster than replayed ones on every benchmark configuration.  No reference counterpart (the
 * reference launches and synchronises per operation).  GetGraphInfo: first level of the recorded graph (-1: none) and its
 * node count. */
HYPRE_Int hypre_amd_BoomerAMGSetGraphThreshold(HYPRE_Solver solver, HYPRE_Int rows);
HYPRE_Int hypre_amd_BoomerAMGGetGraphInfo(HYPRE_Solver solver, HYPRE_Int *level, HYPRE_Int *nodes);
/* Mixed precision (BASELINE config C5): inside the cycle the SpMV-class kernels stream an fp32 copy of every level's matrix
 * values, diagonal and ghost blocks alike (4 + 2 instead of 8 + 2 bytes per entry); vectors, accumulation, smoother
 * diagonals, the coarse solve and everything outside the cycle stay fp64, and HYPRE_BoomerAMGSolve applies the cycle to the
 * fp64 residual equation from a non-zero iterate.  The reference has only the whole-library HYPRE_SINGLE
 * (utilities/HYPRE_utilities.h:78-89). */
HYPRE_Int hypre_amd_BoomerAMGSetMixedPrecision(HYPRE_Solver solver, HYPRE_Int on);
/* Fusions across the steps of a cycle (default on; environment HYPRE_AMD_CYCLE_FUSION=0): on one rank the restriction
 * f_c = P^T r also writes the result of the coarse level's first Jacobi-type sweep from zero, u_c = (w f_c) ./ d_c, instead
 * of a kernel of its own reading f_c and d_c again (par_cycle.c:340-420 runs the two as separate steps).  Same bits either
 * way; the switch is for comparisons.  on < 0 leaves the setting; returns it. */
HYPRE_Int hypre_amd_SetCycleFusion(HYPRE_Int on);
/* Solves of several columns (num_vectors > 1) cycle their large levels for all columns at once (default off; environment
 * HYPRE_AMD_MULTIVECTOR_CYCLE=1): on one rank, for a V-cycle with relax 7 / 18 over all points and a direct coarsest solve,
 * every pass over an operator of those levels is one launch for a group of 2 - 4 columns, and from the level where the
 * one-workgroup tail or the recorded graph begins each column runs the single-column cycle.  Every column keeps the bits of
 * its single-vector solve; every other configuration cycles column by column.  hypre_amd_SpmvSetFusedMultivectors(0) sends
 * every pass down the column path as well.  on < 0 leaves the setting; returns it. */
HYPRE_Int hypre_amd_SetMultivectorCycle(HYPRE_Int on);
/* The smallest levels of a V(1,1) cycle with Jacobi / l1-Jacobi or two-stage Gauss-Seidel smoothing (relax 7 / 18 / 11 / 12,
 * no C/F ordering) and a direct
 * coarse solve in ONE kernel of one workgroup (default on; environment HYPRE_AMD_SMALL_TAIL=0): from the first level whose
 * operator — and every coarser one — holds at most 20 000 entries (HYPRE_AMD_SMALL_TAIL_NNZ) down and back up, every step
 * of par_cycle.c:23-803 is a launch of ~5 us for a fraction of a microsecond of work; one workgroup walks them with a
 * barrier in between.  One rank only.  Same arithmetic, the products of a row added in a fixed order of its own (rounding
 * differences against the per-level kernels).  on < 0 leaves the setting; returns it. */
HYPRE_Int hypre_amd_SetSmallTail(HYPRE_Int on);
/* Test hook: how the tail's kernel holds the first level's operator — 0 with everything else in LDS, 1 in the lanes'
 * registers (its rows times their lanes fill the workgroup once), 2 streamed from global memory; -1 (default) the first of
 * these that fits. */
HYPRE_Int hypre_amd_SetSmallTailForm(HYPRE_Int form);
/* first level of the one-workgroup tail in the last cycle of this solver (-1: none, -2: no cycle has run) */
HYPRE_Int hypre_amd_BoomerAMGGetSmallTailLevel(HYPRE_Solver solver);
/* Test hook: the dense solve of the coarsest level on its own.  a (n x n, row-major) and b are host arrays and stay as they
 * are; a is factored by the routine the cycle's coarse solve factors its operator with (the reference's pivot-free
 * elimination, utilities/gselim.h), b goes to the device, one kernel substitutes, x (host, n entries) receives the
 * result.  form 0: the kernel the cycle launches for n unknowns (one wave up to 32, one lane above); 1: the one-lane
 * kernel whatever n is. */
HYPRE_Int hypre_amd_CoarseSolveTest(const HYPRE_Real *a, HYPRE_Int n, const HYPRE_Real *b, HYPRE_Int form, HYPRE_Real *x);
/* grid / operator complexity of the last setup */
HYPRE_Int hypre_amd_BoomerAMGGetComplexities(HYPRE_Solver solver, HYPRE_Real *grid, HYPRE_Real *op);
/* Multi-rank device hierarchies: levels with at most `rows` global rows are gathered onto every rank at
 * setup and the V-cycle below the first such level runs locally from one all-reduced right-hand side
 * (latency of four halo exchanges per level removed).  Applies to V-cycles with smoothers whose result
 * does not depend on the row distribution (relax 0/7/18 with or without CF ordering, Chebyshev 16); default 16384,
 * 0 disables.  hypre's own relative is the seq_threshold /
 * hypre_seqAMGSetup path (par_amg_setup.c), which re-coarsens the gathered operator instead. */
HYPRE_Int hypre_amd_BoomerAMGSetReplicateThreshold(HYPRE_Solver solver, HYPRE_Int rows);
HYPRE_Int hypre_amd_BoomerAMGGetReplicatedLevel(HYPRE_Solver solver);      /* -1: none */
/* par_amg_solve.c:391-401: operation count of the last cycle (the reference's cycle complexity = this / nnz(A_0)) */
HYPRE_Int hypre_amd_BoomerAMGGetCycleOpCount(HYPRE_Solver solver, HYPRE_Real *count);
/* algorithmic HBM bytes of one cycle on the current hierarchy (SURVEY §8d formula) */
HYPRE_Real hypre_amd_BoomerAMGCycleBytes(HYPRE_Solver solver);
/* level accessors for tests / the oracle harness */
HYPRE_Int hypre_amd_BoomerAMGGetNumLevels(HYPRE_Solver solver);
hypre_ParCSRMatrix *hypre_amd_BoomerAMGGetA(HYPRE_Solver solver, HYPRE_Int level);
hypre_ParCSRMatrix *hypre_amd_BoomerAMGGetP(HYPRE_Solver solver, HYPRE_Int level);
hypre_IntArray     *hypre_amd_BoomerAMGGetCFMarker(HYPRE_Solver solver, HYPRE_Int level);
hypre_Vector       *hypre_amd_BoomerAMGGetL1Norms(HYPRE_Solver solver, HYPRE_Int level);
HYPRE_Int hypre_amd_BoomerAMGGetGridRelaxType(HYPRE_Solver solver, HYPRE_Int k);
HYPRE_Int hypre_amd_BoomerAMGGetNumGridSweeps(HYPRE_Solver solver, HYPRE_Int k);

/* ---- setup building blocks (host) ---- */
HYPRE_Int hypre_BoomerAMGSetup(void *amg_vdata, hypre_ParCSRMatrix *A, hypre_ParVector *f, hypre_ParVector *u);
HYPRE_Int hypre_BoomerAMGCreateS(hypre_ParCSRMatrix *A, HYPRE_Real strength_threshold, HYPRE_Real max_row_sum,
                                 HYPRE_Int num_functions, HYPRE_Int *dof_func, hypre_ParCSRMatrix **S_ptr);
HYPRE_Int hypre_BoomerAMGCoarsenPMIS(hypre_ParCSRMatrix *S, hypre_ParCSRMatrix *A, HYPRE_Int CF_init,
                                     HYPRE_Int debug_flag, hypre_IntArray **CF_marker_ptr);
HYPRE_Int hypre_BoomerAMGCoarsenHMIS(hypre_ParCSRMatrix *S, hypre_ParCSRMatrix *A, HYPRE_Int measure_type,
                                     HYPRE_Int cut_factor, HYPRE_Int debug_flag, hypre_IntArray **CF_marker_ptr);
HYPRE_Int hypre_BoomerAMGBuildExtPIInterp(hypre_ParCSRMatrix *A, HYPRE_Int *CF_marker, hypre_ParCSRMatrix *S,
                                          HYPRE_BigInt *num_cpts_global, HYPRE_Int num_functions,
                                          HYPRE_Int *dof_func, HYPRE_Int debug_flag, HYPRE_Real trunc_factor,
                                          HYPRE_Int max_elmts, hypre_ParCSRMatrix **P_ptr);
HYPRE_Int hypre_BoomerAMGBuildExtInterp(hypre_ParCSRMatrix *A, HYPRE_Int *CF_marker, hypre_ParCSRMatrix *S,
                                        HYPRE_BigInt *num_cpts_global, HYPRE_Int num_functions,
                                        HYPRE_Int *dof_func, HYPRE_Int debug_flag, HYPRE_Real trunc_factor,
                                        HYPRE_Int max_elmts, hypre_ParCSRMatrix **P_ptr);
HYPRE_Int hypre_BoomerAMGBuildExtPICCInterp(hypre_ParCSRMatrix *A, HYPRE_Int *CF_marker, hypre_ParCSRMatrix *S,
                                            HYPRE_BigInt *num_cpts_global, HYPRE_Int num_functions,
                                            HYPRE_Int *dof_func, HYPRE_Int debug_flag, HYPRE_Real trunc_factor,
                                            HYPRE_Int max_elmts, hypre_ParCSRMatrix **P_ptr);
HYPRE_Int hypre_BoomerAMGBuildDirInterp(hypre_ParCSRMatrix *A, HYPRE_Int *CF_marker, hypre_ParCSRMatrix *S,
                                        HYPRE_BigInt *num_cpts_global, HYPRE_Int num_functions,
                                        HYPRE_Int *dof_func, HYPRE_Int debug_flag, HYPRE_Real trunc_factor,
                                        HYPRE_Int max_elmts, HYPRE_Int interp_type, hypre_ParCSRMatrix **P_ptr);
HYPRE_Int hypre_BoomerAMGInterpTruncation(hypre_ParCSRMatrix *P, HYPRE_Real trunc_factor, HYPRE_Int max_elmts);
HYPRE_Int hypre_BoomerAMGBuildCoarseOperatorKT(hypre_ParCSRMatrix *RT, hypre_ParCSRMatrix *A,
                                               hypre_ParCSRMatrix *P, HYPRE_Int keepTranspose,
                                               hypre_ParCSRMatrix **RAP_ptr);
HYPRE_Int hypre_ParCSRComputeL1Norms(hypre_ParCSRMatrix *A, HYPRE_Int option, HYPRE_Int *cf_marker,
                                     HYPRE_Real **l1_norm_ptr);
/* parcsr_ls/ams.c:4535-4915: the variant the host routine switches to under OpenMP (options 1, 4, 5, 6) */
HYPRE_Int hypre_ParCSRComputeL1NormsThreads(hypre_ParCSRMatrix *A, HYPRE_Int option, HYPRE_Int num_threads,
                                            HYPRE_Int *cf_marker, HYPRE_Real **l1_norm_ptr);

/* ---- the hot path ---- */
HYPRE_Int hypre_BoomerAMGRelax(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                               HYPRE_Int relax_type, HYPRE_Int relax_points, HYPRE_Real relax_weight,
                               HYPRE_Real omega, HYPRE_Real *l1_norms, hypre_ParVector *u,
                               hypre_ParVector *Vtemp, hypre_ParVector *Ztemp);
HYPRE_Int hypre_BoomerAMGRelaxIF(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                                 HYPRE_Int relax_type, HYPRE_Int relax_order, HYPRE_Int cycle_param,
                                 HYPRE_Real relax_weight, HYPRE_Real omega, HYPRE_Real *l1_norms,
                                 hypre_ParVector *u, hypre_ParVector *Vtemp, hypre_ParVector *Ztemp);
HYPRE_Int hypre_ParCSRRelax_L1_Jacobi(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                                      HYPRE_Int relax_points, HYPRE_Real relax_weight, HYPRE_Real *l1_norms,
                                      hypre_ParVector *u, hypre_ParVector *Vtemp);
HYPRE_Int hypre_BoomerAMGRelax_FCFJacobi(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                                         HYPRE_Real relax_weight, hypre_ParVector *u, hypre_ParVector *Vtemp);
/* Chebyshev polynomial smoothing.
 *   parcsr_ls/par_relax_more.c:34-198   spectrum estimates: Gershgorin discs / Lanczos on k CG steps (host, setup time)
 *   parcsr_ls/par_cheby.c:57-222        coefficients of the degree-(order-1) polynomial and the scaling vector (host)
 *   parcsr_ls/par_cheby.c:405-446, par_cheby_device.c:119-294   u += p(A)(f - A u) (device operands only) */
HYPRE_Int hypre_ParCSRMaxEigEstimate(hypre_ParCSRMatrix *A, HYPRE_Int scale, HYPRE_Real *max_eig, HYPRE_Real *min_eig);
HYPRE_Int hypre_ParCSRMaxEigEstimateCG(hypre_ParCSRMatrix *A, HYPRE_Int scale, HYPRE_Int max_iter,
                                       HYPRE_Real *max_eig, HYPRE_Real *min_eig);
HYPRE_Int hypre_ParCSRRelax_Cheby_Setup(hypre_ParCSRMatrix *A, HYPRE_Real max_eig, HYPRE_Real min_eig,
                                        HYPRE_Real fraction, HYPRE_Int order, HYPRE_Int scale, HYPRE_Int variant,
                                        HYPRE_Real **coefs_ptr, HYPRE_Real **ds_ptr);
HYPRE_Int hypre_ParCSRRelax_Cheby_Solve(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Real *ds_data,
                                        HYPRE_Real *coefs, HYPRE_Int order, HYPRE_Int scale, HYPRE_Int variant,
                                        hypre_ParVector *u, hypre_ParVector *v, hypre_ParVector *r,
                                        hypre_ParVector *orig_u_vec, hypre_ParVector *tmp_vec);
/* level data of the Chebyshev smoother for inspection (NULL when relax 16 is not in use) */
HYPRE_Int     hypre_amd_BoomerAMGGetChebyOrderScale(HYPRE_Solver solver, HYPRE_Int *order, HYPRE_Int *scale);
HYPRE_Real   *hypre_amd_BoomerAMGGetChebyCoefs(HYPRE_Solver solver, HYPRE_Int level);
hypre_Vector *hypre_amd_BoomerAMGGetChebyDS(HYPRE_Solver solver, HYPRE_Int level);

HYPRE_Int hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(hypre_ParCSRMatrix *A, hypre_ParVector *f,
                                                        HYPRE_Real relax_weight, HYPRE_Real omega,
                                                        HYPRE_Real *A_diag_diag, hypre_ParVector *u,
                                                        hypre_ParVector *r, hypre_ParVector *z,
                                                        HYPRE_Int num_inner_iters);
HYPRE_Int hypre_BoomerAMGRelaxHybridGaussSeidelDevice(hypre_ParCSRMatrix *A, hypre_ParVector *f,
                                                      HYPRE_Int *cf_marker, HYPRE_Int relax_points,
                                                      HYPRE_Real relax_weight, HYPRE_Real omega,
                                                      HYPRE_Real *l1_norms, hypre_ParVector *u,
                                                      hypre_ParVector *Vtemp, hypre_ParVector *Ztemp,
                                                      HYPRE_Int GS_order, HYPRE_Int Symm);
/* Emulated OpenMP threads (blocks of hypre_partition1D) of the hybrid sweeps for DIRECT relaxation calls; values below 1
 * become 1.  A solve sets its own count (hypre_amd_BoomerAMGSetNumThreads) for its duration and puts this one back. */
HYPRE_Int hypre_amd_RelaxSetNumThreads(HYPRE_Int n);
/* What the last hypre_BoomerAMGRelaxHybridGaussSeidelDevice call used and did: lanes per row (4, 8, 16, 32), blocks of the
 * schedule (the thread count clamped to the row count), and the launches of the one-workgroup run kernel and of the
 * one-grid-per-level kernel, summed over both directions of a symmetric sweep.  Host counters; any pointer may be NULL. */
HYPRE_Int hypre_amd_GsSweepStats(HYPRE_Int *lanes, HYPRE_Int *threads, HYPRE_Int *run_launches, HYPRE_Int *level_launches);
/* Multicolour Gauss-Seidel, relax types 21 (colours ascending) and 22 (descending) of hypre_BoomerAMGRelax.  No
 * counterpart in the reference (parcsr_ls/par_relax*.c knows no colouring): it is the hybrid Gauss-Seidel sweep of
 * par_relax.c:691-945 (Jacobi across ranks, Gauss-Seidel inside a rank) on the colour-permuted local ordering, which
 * the GPU can run one colour at a time.  `diag`: smoother diagonal (the l1_norms option-5 vector of relax 7 / 11 / 12)
 * or NULL for the stored diagonal; Vtemp: local work vector (may be NULL on one rank); direction: +1 / -1. */
HYPRE_Int hypre_BoomerAMGRelaxMultiColorGaussSeidelDevice(hypre_ParCSRMatrix *A, hypre_ParVector *f,
                                                          HYPRE_Int *cf_marker, HYPRE_Int relax_points,
                                                          HYPRE_Real relax_weight, HYPRE_Real *diag,
                                                          hypre_ParVector *u, hypre_ParVector *Vtemp,
                                                          HYPRE_Int direction);
/* number of colours of A's diagonal block (greedy first-fit over the symmetrised pattern, built on demand);
 * colors_out: host array of one colour per local row, or NULL */
HYPRE_Int hypre_amd_ParCSRMatrixMultiColoring(hypre_ParCSRMatrix *A, HYPRE_Int *colors_out);
/* The one-workgroup multicolour sweeps (small levels, the tails of small colours of larger ones) request what does not depend
 * on the iterate — a row's place, right-hand side, diagonal, own value and first entries — one pass ahead (default 1), or
 * walk the plain chain of dependent loads (0); < 0 leaves the setting; returns it.  Same results. */
HYPRE_Int hypre_amd_SetMcLookAhead(HYPRE_Int on);
HYPRE_Int hypre_GaussElimSetup(hypre_ParAMGData *amg_data, HYPRE_Int level, HYPRE_Int relax_type);
HYPRE_Int hypre_GaussElimSolve(hypre_ParAMGData *amg_data, HYPRE_Int level, HYPRE_Int relax_type);
HYPRE_Int hypre_BoomerAMGCycle(void *amg_vdata, hypre_ParVector **F_array, hypre_ParVector **U_array);
HYPRE_Int hypre_BoomerAMGSolve(void *amg_vdata, hypre_ParCSRMatrix *A, hypre_ParVector *f, hypre_ParVector *u);

/* ---- PCG with BoomerAMG as preconditioner (the caller in the benchmark configs) ---- */
HYPRE_Int HYPRE_ParCSRPCGCreate(MPI_Comm comm, HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRPCGDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_PCGSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_PCGSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_PCGSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_PCGSetTwoNorm(HYPRE_Solver solver, HYPRE_Int two_norm);
HYPRE_Int HYPRE_PCGSetLogging(HYPRE_Solver solver, HYPRE_Int logging);             /* accepted, inert */
HYPRE_Int HYPRE_PCGSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);            /* accepted, inert */
HYPRE_Int HYPRE_PCGSetRelChange(HYPRE_Solver solver, HYPRE_Int rel_change);        /* 0 only */
HYPRE_Int HYPRE_PCGSetRecomputeResidual(HYPRE_Solver solver, HYPRE_Int recompute); /* 0 only */
HYPRE_Int HYPRE_PCGSetFlex(HYPRE_Solver solver, HYPRE_Int flex);     /* pcg.c:339-345, 636-639, 720-723, 957-965; before Setup */
HYPRE_Int HYPRE_PCGSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                              HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
/* the diagonal-scaling preconditioner of the reference driver's DS-PCG (`ij -solver 2`; parcsr_ls/HYPRE_parcsr_pcg.c):
 * x = y ./ diag(A); vectors may be multivectors (`-nc N`: test/TEST_ij/vector.jobs) */
HYPRE_Int HYPRE_ParCSRDiagScaleSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector y, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRDiagScale(HYPRE_Solver solver, HYPRE_ParCSRMatrix HA, HYPRE_ParVector Hy, HYPRE_ParVector Hx);
HYPRE_Int HYPRE_ParCSRPCGSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRPCGSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_PCGGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_PCGGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
/* pcg.c:893-950: with cf_tol > 0 the solve gives up, without an error, when the average convergence factor
 * cf = (i_prod / i_prod_0)^(1 / (2 i)), weighted by 1 - |cf - cf_before| / max(cf, cf_before), exceeds cf_tol; 0 (the
 * default) computes nothing.  Converged is 1 when the last solve ended by meeting its tolerance: not at the
 * convergence-factor exit, a breakdown or max_iter (pcg.c:841). */
HYPRE_Int HYPRE_PCGSetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real cf_tol);
HYPRE_Int HYPRE_PCGGetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real *cf_tol);
HYPRE_Int HYPRE_PCGGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);
/* Behind HYPRE_ParCSRDiagScale on vectors of one column in device memory, the update of x and r, the diagonal scaling
 * and the inner product of an iteration are one launch over a copy of the diagonal that Setup packs (64 bytes per
 * element instead of 92, 2 launches instead of 5); x, r, the iteration count and the norms have the same bits.  Set
 * before Setup; 1 is the default (measured in DESIGN.md 6b).  The packed diagonal is that of the matrix Setup saw: after changing the values, call Setup again.
 * GetFusedDiagScaleUsed, valid after Setup: 1 when the solves of this Setup take it; 0 for another preconditioner, a
 * multivector, host operands or a matrix with a row that has no entry. */
HYPRE_Int hypre_amd_PCGSetFusedDiagScale(HYPRE_Solver solver, HYPRE_Int on);
HYPRE_Int hypre_amd_PCGGetFusedDiagScaleUsed(HYPRE_Solver solver, HYPRE_Int *used);
/* That step on its own, s holding A p on entry: x += alpha p, r -= alpha s, s = r ./ diag(A), rr = <r, r>, rs = <r, s>
 * over all ranks; fused 1 the one launch, 0 the three it stands for.  The same bits.  hypre_amd_DotGridPassElements: the
 * elements one trip of its grid covers. */
HYPRE_Int hypre_amd_ParVectorDiagScaledCGStep(HYPRE_Int fused, HYPRE_Complex alpha, hypre_ParCSRMatrix *A, hypre_ParVector *p,
                                              hypre_ParVector *s, hypre_ParVector *x, hypre_ParVector *r, HYPRE_Real *rr, HYPRE_Real *rs);
HYPRE_BigInt hypre_amd_DotGridPassElements(void);

/* ---- GMRES with BoomerAMG as right preconditioner (`ij -solver 3`) ----
 * krylov/gmres.c:274-1000, krylov/HYPRE_gmres.c, parcsr_ls/HYPRE_parcsr_gmres.c; defaults of
 * hypre_GMRESCreate (gmres.c:68-110): k_dim 5, tol 1e-6, max_iter 1000.  SetKDim must precede Setup
 * (Setup allocates the k_dim + 1 basis vectors, gmres.c:204-215).  HYPRE_ERROR_CONV when max_iter is
 * reached above the tolerance (gmres.c:982-985). */
HYPRE_Int HYPRE_ParCSRGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRGMRESDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_GMRESSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_GMRESSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_GMRESSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_GMRESSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_GMRESSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_GMRESSetSkipRealResidualCheck(HYPRE_Solver solver, HYPRE_Int skip_real_r_check);
HYPRE_Int HYPRE_GMRESSetLogging(HYPRE_Solver solver, HYPRE_Int logging);           /* accepted, inert */
HYPRE_Int HYPRE_GMRESSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);          /* accepted, inert */
HYPRE_Int HYPRE_GMRESSetRelChange(HYPRE_Solver solver, HYPRE_Int rel_change);      /* 0 only */
HYPRE_Int HYPRE_GMRESSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_ParCSRGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_GMRESGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_GMRESGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_GMRESGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);
/* gmres.c:597-615: the convergence-factor exit as for PCG above, on the norm of the recurrence, looked at after every
 * step; the correction of the restart cycle under way is not added to x.  GMRES only: COGMRES and LGMRES have no such
 * setter, FlexGMRES takes 0.0 only. */
HYPRE_Int HYPRE_GMRESSetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real cf_tol);
HYPRE_Int HYPRE_GMRESGetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real *cf_tol);

/* ---- COGMRES: restarted GMRES whose Gram-Schmidt step is batched (`ij -solver 16 | 17`) ----
 * krylov/cogmres.c:274-900, krylov/HYPRE_cogmres.c, parcsr_ls/HYPRE_parcsr_cogmres.c; defaults of hypre_COGMRESCreate
 * (cogmres.c:85-111): k_dim 5, cgs 1, unroll 0, tol 1e-6, max_iter 1000.  Step i of a restart cycle orthogonalises with
 * one hypre_ParVectorMassInnerProd and one hypre_ParVectorMassAxpy over the i basis vectors (classical Gram-Schmidt,
 * cgs 1), or with hypre_ParVectorMassDotpTwo and the reorthogonalising correction of cogmres.c:550-566 (cgs 2): two
 * read-backs a step instead of i + 1.  SetUnroll is kept for the reference's callers and changes nothing (see
 * hypre_SeqVectorMassInnerProd).  SetKDim must precede Setup; the relative-change and convergence-factor exits are not
 * carried, as for GMRES. */
HYPRE_Int HYPRE_ParCSRCOGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRCOGMRESDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_COGMRESSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_COGMRESSetUnroll(HYPRE_Solver solver, HYPRE_Int unroll);
HYPRE_Int HYPRE_COGMRESSetCGS(HYPRE_Solver solver, HYPRE_Int cgs);
HYPRE_Int HYPRE_COGMRESSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_COGMRESSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_COGMRESSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_COGMRESSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_COGMRESSetSkipRealResidualCheck(HYPRE_Solver solver, HYPRE_Int skip_real_r_check);
HYPRE_Int HYPRE_COGMRESSetLogging(HYPRE_Solver solver, HYPRE_Int logging);         /* accepted, inert */
HYPRE_Int HYPRE_COGMRESSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);        /* accepted, inert */
HYPRE_Int HYPRE_COGMRESSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                  HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_ParCSRCOGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRCOGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_COGMRESGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_COGMRESGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_COGMRESGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);

/* ---- FlexGMRES: restarted GMRES that keeps the preconditioned vectors (the reference's `ij -solver 60 | 61`) ----
 * krylov/flexgmres.c:330-760, krylov/HYPRE_flexgmres.c, parcsr_ls/HYPRE_parcsr_flexgmres.c; defaults of
 * hypre_FlexGMRESCreate (flexgmres.c:86-91): k_dim 20, tol 1e-6, a_tol 0, min_iter 0, max_iter 1000.  The correction of
 * a restart cycle is a combination of the stored vectors Z_j = M_j^{-1} v_j, so the preconditioner may differ from one
 * application to the next and is applied once per iteration, never once more per restart.  Before every application the
 * target is cleared and modify_pc(precond_solver, iteration, |r| / |b|) is called (default: does nothing).  SetKDim must
 * precede Setup (2 (k_dim + 1) + 2 work vectors).  The convergence-factor exit is not carried: SetConvergenceFactorTol
 * takes 0.0 only.  HYPRE_ERROR_CONV when max_iter is reached above the tolerance — unlike flexgmres.c:743 also when both
 * tolerances are zero.  Vectors may be multivectors; the inner product is the flat one over all columns. */
typedef HYPRE_Int (*HYPRE_PtrToModifyPCFcn)(HYPRE_Solver, HYPRE_Int, HYPRE_Real);
HYPRE_Int HYPRE_ParCSRFlexGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRFlexGMRESDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRFlexGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_FlexGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_FlexGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_FlexGMRESSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_FlexGMRESSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_FlexGMRESSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_FlexGMRESSetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real cf_tol);   /* 0.0 only */
HYPRE_Int HYPRE_FlexGMRESSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_FlexGMRESSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_FlexGMRESSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                    HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_FlexGMRESGetPrecond(HYPRE_Solver solver, HYPRE_Solver *precond_data_ptr);
HYPRE_Int HYPRE_FlexGMRESSetModifyPC(HYPRE_Solver solver, HYPRE_PtrToModifyPCFcn modify_pc);   /* NULL: the default */
HYPRE_Int HYPRE_FlexGMRESSetLogging(HYPRE_Solver solver, HYPRE_Int logging);       /* accepted, inert */
HYPRE_Int HYPRE_FlexGMRESSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);      /* accepted, inert */
HYPRE_Int HYPRE_FlexGMRESGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_FlexGMRESGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_FlexGMRESGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                          HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_ParCSRFlexGMRESGetPrecond(HYPRE_Solver solver, HYPRE_Solver *precond_data_ptr);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetModifyPC(HYPRE_Solver solver, HYPRE_PtrToModifyPCFcn modify_pc);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
HYPRE_Int HYPRE_ParCSRFlexGMRESSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);
HYPRE_Int HYPRE_ParCSRFlexGMRESGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_ParCSRFlexGMRESGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
/* Modified Gram-Schmidt of FlexGMRES, fused (1, the default): Arnoldi step i is one inner product and i launches that
 * each subtract the projection on one basis vector and leave the inner product with the next one (the last: the squared
 * norm) in the same pass; the correction of a restart is one batched update.  0: the reference's sequence of
 * InnerProd / Axpy calls.  Either way a solve gives the same bits in x, the same iteration count and the same norm. */
HYPRE_Int hypre_amd_FlexGMRESSetFusedOrthogonalization(HYPRE_Solver solver, HYPRE_Int on);
/* Launches of the Gram-Schmidt steps of the last solve: fused steps, separate inner products (the norms included) and
 * separate updates.  Fused, step i counts (i, 1, 0); not fused (0, i + 1, i).  Host counters; any pointer may be NULL. */
HYPRE_Int hypre_amd_FlexGMRESGetLaunchStats(HYPRE_Solver solver, HYPRE_Int *fused_steps, HYPRE_Int *plain_dots, HYPRE_Int *plain_axpys);
/* y += alpha x, then *result = <z, y> over all ranks, in one pass over the vectors (z may be y): the fused launch of a
 * Gram-Schmidt step and the reduction of hypre_ParVectorInnerProd.  The bits of hypre_ParVectorAxpy followed by
 * hypre_ParVectorInnerProd(z, y). */
HYPRE_Int hypre_amd_ParVectorAxpyThenInnerProd(HYPRE_Complex alpha, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z,
                                               HYPRE_Real *result);

/* ---- LGMRES: restarted GMRES that carries corrections across restarts (the reference's `ij -solver 50 | 51`) ----
 * krylov/lgmres.c:326-934, krylov/HYPRE_lgmres.c, parcsr_ls/HYPRE_parcsr_lgmres.c; defaults of hypre_LGMRESCreate
 * (lgmres.c:83-105): k_dim 20, aug_dim 2, tol 1e-6, a_tol 0, min_iter 0, max_iter 1000.  A restart cycle has k_dim
 * steps; the last ones (as many as there are augmentation vectors, aug_dim at most) are not Arnoldi steps but reuse the
 * normalised corrections z of the cycles before, kept with A z = (r0 - r_m) / |w|, so they cost neither a matrix nor a
 * preconditioner application.  SetAugDim clamps to 0 .. k_dim - 1 with the k_dim in force at the call; SetKDim and
 * SetAugDim must precede Setup (k_dim + 2 aug_dim + 4 work vectors shaped like x; Solve refuses otherwise).  Operands
 * are in device memory and may be multivectors (the flat inner product over all columns).  The relative-change and
 * convergence-factor exits are not carried.  HYPRE_ERROR_CONV when max_iter is reached above a non-zero tolerance
 * (lgmres.c:918).  A residual of exactly zero returns at once and leaves count and norm as they were (lgmres.c:545). */
HYPRE_Int HYPRE_ParCSRLGMRESCreate(MPI_Comm comm, HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRLGMRESDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_ParCSRLGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRLGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_LGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_LGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_LGMRESSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_LGMRESSetAugDim(HYPRE_Solver solver, HYPRE_Int aug_dim);
HYPRE_Int HYPRE_LGMRESGetAugDim(HYPRE_Solver solver, HYPRE_Int *aug_dim);
HYPRE_Int HYPRE_LGMRESSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_LGMRESSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_LGMRESSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_LGMRESSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_LGMRESSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                 HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_LGMRESGetPrecond(HYPRE_Solver solver, HYPRE_Solver *precond_data_ptr);
HYPRE_Int HYPRE_LGMRESSetLogging(HYPRE_Solver solver, HYPRE_Int logging);          /* accepted, inert */
HYPRE_Int HYPRE_LGMRESSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);         /* accepted, inert */
HYPRE_Int HYPRE_LGMRESGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_LGMRESGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_LGMRESGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);
HYPRE_Int HYPRE_LGMRESGetResidual(HYPRE_Solver solver, void *residual);             /* a HYPRE_ParVector * */
HYPRE_Int HYPRE_ParCSRLGMRESSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_ParCSRLGMRESSetAugDim(HYPRE_Solver solver, HYPRE_Int aug_dim);
HYPRE_Int HYPRE_ParCSRLGMRESSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_ParCSRLGMRESSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_ParCSRLGMRESSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_ParCSRLGMRESSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_ParCSRLGMRESSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                       HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_ParCSRLGMRESGetPrecond(HYPRE_Solver solver, HYPRE_Solver *precond_data_ptr);
HYPRE_Int HYPRE_ParCSRLGMRESSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
HYPRE_Int HYPRE_ParCSRLGMRESSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);
HYPRE_Int HYPRE_ParCSRLGMRESGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_ParCSRLGMRESGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_ParCSRLGMRESGetResidual(HYPRE_Solver solver, HYPRE_ParVector *residual);
/* lgmres.c:593-600, a field the reference sets only in Create: 1 (the default) keeps a cycle at k_dim steps while fewer
 * than aug_dim augmentation vectors exist; 0 takes k_dim - aug_dim Arnoldi steps from the first cycle on. */
HYPRE_Int hypre_amd_LGMRESSetApproxConstant(HYPRE_Solver solver, HYPRE_Int on);
/* 1 (the default): Gram-Schmidt steps fused as for FlexGMRES; the correction of a cycle one scaled copy and one batched
 * update over Arnoldi and augmentation terms; the end of a cycle that restarts 4 launches (copy with squared norm, two
 * scaled copies, scaled difference), 72 bytes per vector element.  0: the reference's Copy / Scale / InnerProd / Axpy
 * sequence, 10 calls and 168 bytes for that end.  Either way a solve gives the same bits in x, the same iteration count
 * and the same norm. */
HYPRE_Int hypre_amd_LGMRESSetFusedUpdates(HYPRE_Solver solver, HYPRE_Int on);
/* Launches of the last solve.  The first three as hypre_amd_FlexGMRESGetLaunchStats.  fused_updates: launches of the
 * three operations below, for the correction and the end of every cycle; plain_updates: library calls made in their
 * place.  With aug_dim > 0 a cycle that restarts counts 5 fused or 12 plain, the cycle a solve converges in 2 or 3.
 * Host counters; any pointer may be NULL. */
HYPRE_Int hypre_amd_LGMRESGetLaunchStats(HYPRE_Solver solver, HYPRE_Int *fused_steps, HYPRE_Int *plain_dots, HYPRE_Int *plain_axpys,
                                         HYPRE_Int *fused_updates, HYPRE_Int *plain_updates);
/* The vector operations LGMRES adds, each one pass with the bits of the library calls it stands for; device memory,
 * equal lengths, the target distinct from the sources.
 *   ScaledCopy          y = a x           hypre_ParVectorCopy(x, y); hypre_ParVectorScale(a, y)
 *   CopyThenInnerProd   y = x, <x, x>     hypre_ParVectorCopy(x, y); hypre_ParVectorInnerProd(y, y)   (over all ranks)
 *   ScaledDifference    z = a (x - y)     hypre_ParVectorCopy(x, z); Scale(-1, z); Axpy(1, y, z); Scale(-a, z) */
HYPRE_Int hypre_amd_ParVectorScaledCopy(HYPRE_Complex a, hypre_ParVector *x, hypre_ParVector *y);
HYPRE_Int hypre_amd_ParVectorCopyThenInnerProd(hypre_ParVector *x, hypre_ParVector *y, HYPRE_Real *result);
HYPRE_Int hypre_amd_ParVectorScaledDifference(HYPRE_Complex a, hypre_ParVector *x, hypre_ParVector *y, hypre_ParVector *z);

/* ---- BiCGSTAB: the short-recurrence solver for non-symmetric operators (the reference's `ij -solver 9 | 10`) ----
 * krylov/bicgstab.c:225-578, krylov/HYPRE_bicgstab.c, parcsr_ls/HYPRE_parcsr_bicgstab.c; defaults of hypre_BiCGSTABCreate
 * (bicgstab.c:75-84): tol 1e-6, a_tol 0, cf_tol 0, min_iter 0, max_iter 1000, stop_crit 0.  An iteration applies the
 * preconditioner twice and A twice and keeps six work vectors shaped like x, whatever the iteration count.  Operands are
 * in device memory and may be multivectors (the flat inner product over all columns).  It stops at
 * |r| <= max(a_tol, tol |b|) (|r_0| for |b| when b is zero; with stop_crit the absolute a_tol, or tol if a_tol is 0) once
 * min_iter iterations are done, and then only if b - A x computed from x passes the same test; with cf_tol > 0 also when
 * the average convergence factor (|r| / |r_0|)^(1 / (2 iter)) stays above cf_tol.  HYPRE_ERROR_CONV when max_iter is
 * reached above the tolerance.  The three breakdowns (<r0, A M^-1 p>, <r0, r> or the step length gamma below the smallest
 * normal number) raise HYPRE_ERROR_GENERIC with a message and, as in the reference, return without storing the iteration
 * count or the norm.  Logging or PrintLevel > 0 keeps |r| of every iteration; PrintLevel > 0 prints the reference's table
 * on rank 0. */
HYPRE_Int HYPRE_ParCSRBiCGSTABCreate(MPI_Comm comm, HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRBiCGSTABDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRBiCGSTABSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetStopCrit(HYPRE_Solver solver, HYPRE_Int stop_crit);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                         HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_ParCSRBiCGSTABGetPrecond(HYPRE_Solver solver, HYPRE_Solver *precond_data_ptr);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
HYPRE_Int HYPRE_ParCSRBiCGSTABSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);
HYPRE_Int HYPRE_ParCSRBiCGSTABGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_ParCSRBiCGSTABGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_ParCSRBiCGSTABGetResidual(HYPRE_Solver solver, HYPRE_ParVector *residual);
HYPRE_Int HYPRE_BiCGSTABDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_BiCGSTABSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_BiCGSTABSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_BiCGSTABSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_BiCGSTABSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_BiCGSTABSetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real cf_tol);
HYPRE_Int HYPRE_BiCGSTABSetMinIter(HYPRE_Solver solver, HYPRE_Int min_iter);
HYPRE_Int HYPRE_BiCGSTABSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_BiCGSTABSetStopCrit(HYPRE_Solver solver, HYPRE_Int stop_crit);
HYPRE_Int HYPRE_BiCGSTABSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond,
                                   HYPRE_PtrToSolverFcn precond_setup, HYPRE_Solver precond_solver);
HYPRE_Int HYPRE_BiCGSTABGetPrecond(HYPRE_Solver solver, HYPRE_Solver *precond_data_ptr);
HYPRE_Int HYPRE_BiCGSTABSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
HYPRE_Int HYPRE_BiCGSTABSetPrintLevel(HYPRE_Solver solver, HYPRE_Int level);
HYPRE_Int HYPRE_BiCGSTABGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_BiCGSTABGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_BiCGSTABGetResidual(HYPRE_Solver solver, void *residual);           /* a HYPRE_ParVector * */
/* 1 (the default): of the eleven vector calls the reference makes between the two products with A, the two inner
 * products of the step length are one pass, the second half step with the squared norm and <r0, r> of the new residual
 * one pass, the direction update one pass; three read-backs instead of five.  The first half step stays two axpys (one
 * launch would move the same bytes).  0: the reference's sequence of InnerProd / Axpy / Scale calls.  Either way a solve
 * gives the same bits in x, the same iteration count and the same norms. */
HYPRE_Int hypre_amd_BiCGSTABSetFusedUpdates(HYPRE_Solver solver, HYPRE_Int on);
/* 1 when the last solve ended by meeting its tolerance (the reference keeps this flag without a getter). */
HYPRE_Int hypre_amd_BiCGSTABGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);
/* The norms the last solve logged (Logging or PrintLevel > 0): |r_0|, then |r| of the recurrence after every iteration.
 * The array belongs to the solver and holds until its next Solve or Destroy. */
HYPRE_Int hypre_amd_BiCGSTABGetLoggedNorms(HYPRE_Solver solver, HYPRE_Int *count, const HYPRE_Real **norms);
/* The vector operations BiCGSTAB adds, each one pass with the bits of the library calls it stands for (sums over all
 * ranks, reduced together); device memory, equal lengths, a vector that is written distinct from every other operand.
 *   InnerProdWithNorm         <x, y>, <y, y>                   InnerProd(x, y); InnerProd(y, y)
 *   TwoAxpysThenInnerProds    x += a v, r += b s,              Axpy(a, v, x); Axpy(b, s, r);
 *                             <r, r>, <r0, r>                  InnerProd(r, r); InnerProd(r0, r)
 *   AxpyScaleAxpy             p = r + c (p + g q)              Axpy(g, q, p); Scale(c, p); Axpy(1, r, p) */
HYPRE_Int hypre_amd_ParVectorInnerProdWithNorm(hypre_ParVector *x, hypre_ParVector *y, HYPRE_Real *xy, HYPRE_Real *yy);
HYPRE_Int hypre_amd_ParVectorTwoAxpysThenInnerProds(HYPRE_Complex a, hypre_ParVector *v, hypre_ParVector *x, HYPRE_Complex b,
                                                    hypre_ParVector *s, hypre_ParVector *r, hypre_ParVector *r0, HYPRE_Real *rr,
                                                    HYPRE_Real *r0r);
HYPRE_Int hypre_amd_ParVectorAxpyScaleAxpy(HYPRE_Complex g, hypre_ParVector *q, HYPRE_Complex c, hypre_ParVector *r, hypre_ParVector *p);
/* hypre_amd_BiCGSTABGetConverged under the name the other Krylov solvers use, and the getter of cf_tol */
HYPRE_Int HYPRE_BiCGSTABGetConverged(HYPRE_Solver solver, HYPRE_Int *converged);
HYPRE_Int HYPRE_BiCGSTABGetConvergenceFactorTol(HYPRE_Solver solver, HYPRE_Real *cf_tol);

/* ---- Hybrid: diagonal scaling first, BoomerAMG only if convergence is slow (the reference's `ij -solver 20`) ----
 * parcsr_ls/amg_hybrid.c, parcsr_ls/HYPRE_parcsr_hybrid.c; defaults of hypre_AMGHybridCreate (amg_hybrid.c:99-160): tol 1e-6,
 * a_tol 0, cf_tol 0.9, dscg_max_its 1000, pcg_max_its 200, solver_type 1, k_dim 5, setup_type 1, logging 0; for the
 * preconditioner strong_threshold 0.25, max_row_sum 0.9, trunc_factor 0, P_max_elmts 4, max_levels 25, coarsen_type 10,
 * interp_type 6, cycle_type 1, relax_order 0, keep_transpose 0, max_coarse_size 9, min_coarse_size 1, smoothers 13 / 14 / 9.
 * Solve (amg_hybrid.c:1770-2310) runs the Krylov solver of solver_type (1 PCG, 2 GMRES, 3 BiCGSTAB) behind
 * HYPRE_ParCSRDiagScale with the convergence-factor exit cf_tol and dscg_max_its; if it reports converged that is the
 * answer and no hierarchy is built.  Otherwise cf_tol becomes 0, BoomerAMG is created from the stored options and set
 * up, and the same solver goes on from the current x with pcg_max_its.  A second Solve builds a new hierarchy unless
 * SetSetupType(0) was called: then an existing one is kept and the solve starts behind it at once.  The diagonally
 * scaled PCG phase takes the fused step of hypre_amd_PCGSetFusedDiagScale when that is the default.
 * Operands are in device memory, one column.  Options the library does not build (AggNumLevels, Nodal, SeqThreshold,
 * NonGalerkinTol other than 0, ...) are stored and raise the error of the BoomerAMG setter when the preconditioner is
 * created; RelChange, RecomputeResidual and StopCrit other than 0, and SetPrecond, are refused at once.  Setup does
 * nothing but look at the operands, as in the reference.  The final norm is stored with Logging > 0 only
 * (amg_hybrid.c:2073, 2243).  PrintLevel xy: y goes to the Krylov solver, x to BoomerAMG. */
HYPRE_Int HYPRE_ParCSRHybridCreate(HYPRE_Solver *solver);
HYPRE_Int HYPRE_ParCSRHybridDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_ParCSRHybridSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRHybridSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ParCSRHybridSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_ParCSRHybridSetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real a_tol);
HYPRE_Int HYPRE_ParCSRHybridSetConvergenceTol(HYPRE_Solver solver, HYPRE_Real cf_tol);
HYPRE_Int HYPRE_ParCSRHybridSetDSCGMaxIter(HYPRE_Solver solver, HYPRE_Int dscg_max_its);
HYPRE_Int HYPRE_ParCSRHybridSetPCGMaxIter(HYPRE_Solver solver, HYPRE_Int pcg_max_its);
HYPRE_Int HYPRE_ParCSRHybridSetSetupType(HYPRE_Solver solver, HYPRE_Int setup_type);
HYPRE_Int HYPRE_ParCSRHybridSetSolverType(HYPRE_Solver solver, HYPRE_Int solver_type);
HYPRE_Int HYPRE_ParCSRHybridSetKDim(HYPRE_Solver solver, HYPRE_Int k_dim);
HYPRE_Int HYPRE_ParCSRHybridSetTwoNorm(HYPRE_Solver solver, HYPRE_Int two_norm);
HYPRE_Int HYPRE_ParCSRHybridSetStopCrit(HYPRE_Solver solver, HYPRE_Int stop_crit);                  /* 0 only */
HYPRE_Int HYPRE_ParCSRHybridSetRelChange(HYPRE_Solver solver, HYPRE_Int rel_change);                /* 0 only */
HYPRE_Int HYPRE_ParCSRHybridSetRecomputeResidual(HYPRE_Solver solver, HYPRE_Int recompute_residual); /* 0 only */
HYPRE_Int HYPRE_ParCSRHybridGetRecomputeResidual(HYPRE_Solver solver, HYPRE_Int *recompute_residual);
HYPRE_Int HYPRE_ParCSRHybridSetPrecond(HYPRE_Solver solver, HYPRE_PtrToSolverFcn precond, HYPRE_PtrToSolverFcn precond_setup,
                                       HYPRE_Solver precond_solver);                                /* refused */
HYPRE_Int HYPRE_ParCSRHybridSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
HYPRE_Int HYPRE_ParCSRHybridSetPrintLevel(HYPRE_Solver solver, HYPRE_Int print_level);
HYPRE_Int HYPRE_ParCSRHybridSetStrongThreshold(HYPRE_Solver solver, HYPRE_Real strong_threshold);
HYPRE_Int HYPRE_ParCSRHybridSetMaxRowSum(HYPRE_Solver solver, HYPRE_Real max_row_sum);
HYPRE_Int HYPRE_ParCSRHybridSetTruncFactor(HYPRE_Solver solver, HYPRE_Real trunc_factor);
HYPRE_Int HYPRE_ParCSRHybridSetPMaxElmts(HYPRE_Solver solver, HYPRE_Int P_max_elmts);
HYPRE_Int HYPRE_ParCSRHybridSetMaxLevels(HYPRE_Solver solver, HYPRE_Int max_levels);
HYPRE_Int HYPRE_ParCSRHybridSetMeasureType(HYPRE_Solver solver, HYPRE_Int measure_type);
HYPRE_Int HYPRE_ParCSRHybridSetCoarsenType(HYPRE_Solver solver, HYPRE_Int coarsen_type);
HYPRE_Int HYPRE_ParCSRHybridSetInterpType(HYPRE_Solver solver, HYPRE_Int interp_type);
HYPRE_Int HYPRE_ParCSRHybridSetCycleType(HYPRE_Solver solver, HYPRE_Int cycle_type);
HYPRE_Int HYPRE_ParCSRHybridSetNumSweeps(HYPRE_Solver solver, HYPRE_Int num_sweeps);
HYPRE_Int HYPRE_ParCSRHybridSetCycleNumSweeps(HYPRE_Solver solver, HYPRE_Int num_sweeps, HYPRE_Int k);
HYPRE_Int HYPRE_ParCSRHybridSetRelaxType(HYPRE_Solver solver, HYPRE_Int relax_type);
HYPRE_Int HYPRE_ParCSRHybridSetCycleRelaxType(HYPRE_Solver solver, HYPRE_Int relax_type, HYPRE_Int k);
HYPRE_Int HYPRE_ParCSRHybridSetRelaxOrder(HYPRE_Solver solver, HYPRE_Int relax_order);
HYPRE_Int HYPRE_ParCSRHybridSetKeepTranspose(HYPRE_Solver solver, HYPRE_Int keepT);
HYPRE_Int HYPRE_ParCSRHybridSetMaxCoarseSize(HYPRE_Solver solver, HYPRE_Int max_coarse_size);
HYPRE_Int HYPRE_ParCSRHybridSetMinCoarseSize(HYPRE_Solver solver, HYPRE_Int min_coarse_size);
HYPRE_Int HYPRE_ParCSRHybridSetSeqThreshold(HYPRE_Solver solver, HYPRE_Int seq_threshold);
HYPRE_Int HYPRE_ParCSRHybridSetRelaxWt(HYPRE_Solver solver, HYPRE_Real relax_wt);
HYPRE_Int HYPRE_ParCSRHybridSetOuterWt(HYPRE_Solver solver, HYPRE_Real outer_wt);
HYPRE_Int HYPRE_ParCSRHybridSetLevelRelaxWt(HYPRE_Solver solver, HYPRE_Real relax_wt, HYPRE_Int level);
HYPRE_Int HYPRE_ParCSRHybridSetLevelOuterWt(HYPRE_Solver solver, HYPRE_Real outer_wt, HYPRE_Int level);
HYPRE_Int HYPRE_ParCSRHybridSetNumPaths(HYPRE_Solver solver, HYPRE_Int num_paths);
HYPRE_Int HYPRE_ParCSRHybridSetAggNumLevels(HYPRE_Solver solver, HYPRE_Int agg_num_levels);
HYPRE_Int HYPRE_ParCSRHybridSetAggInterpType(HYPRE_Solver solver, HYPRE_Int agg_interp_type);
HYPRE_Int HYPRE_ParCSRHybridSetNumFunctions(HYPRE_Solver solver, HYPRE_Int num_functions);
HYPRE_Int HYPRE_ParCSRHybridSetNodal(HYPRE_Solver solver, HYPRE_Int nodal);
HYPRE_Int HYPRE_ParCSRHybridSetNonGalerkinTol(HYPRE_Solver solver, HYPRE_Int num_levels, HYPRE_Real *nongalerkin_tol);
HYPRE_Int HYPRE_ParCSRHybridGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_its);             /* both phases */
HYPRE_Int HYPRE_ParCSRHybridGetDSCGNumIterations(HYPRE_Solver solver, HYPRE_Int *dscg_num_its);
HYPRE_Int HYPRE_ParCSRHybridGetPCGNumIterations(HYPRE_Solver solver, HYPRE_Int *pcg_num_its);
HYPRE_Int HYPRE_ParCSRHybridGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *norm);
HYPRE_Int HYPRE_ParCSRHybridGetSetupSolveTime(HYPRE_Solver solver, HYPRE_Real *time);              /* 4 values: setup 1, solve 1, setup 2, solve 2 */
/* the hierarchy (null while no solve has needed one) and the Krylov solver the hybrid solver keeps; they stay its own */
HYPRE_Int hypre_amd_ParCSRHybridGetPrecond(HYPRE_Solver solver, HYPRE_Solver *amg);
HYPRE_Int hypre_amd_ParCSRHybridGetKrylovSolver(HYPRE_Solver solver, HYPRE_Solver *krylov);

/* ---- ILU: block-Jacobi ILU(k), a solver and a preconditioner (the reference's `ij -solver 80 | 81 | 82`, -ilu_type 0) ----
 * parcsr_ls/HYPRE_parcsr_ilu.c, par_ilu.c, par_ilu_setup.c, par_ilu_solve.c; defaults of hypre_ILUCreate (par_ilu.c:61-106):
 * ilu_type 0, level of fill 0, local reordering 1 (reverse Cuthill-McKee), tri_solve 1 (direct), max_iter 20, tol 1e-7,
 * print level 0, logging 0.  Every rank factors its diagonal block; couplings to other ranks are dropped in the factors
 * and appear only in the residual product with A.  Setup orders, factors (unit L, inverse D, U in the permuted order;
 * a pivot below 1e-14 in magnitude becomes 1e-6) and computes the dependency levels of L and U on the host, whatever
 * memory A is in; the factors travel to the device in level order when A is there, or with the first Solve on device
 * vectors.  Solve (hypre_ILUSolve) iterates  u += (L D^-1 U)^-1 (f - A u)  until the relative residual norm is below tol,
 * at least once and at most max_iter times (HYPRE_ERROR_CONV at max_iter with tol > 0); a zero right-hand side gives
 * u = 0; with tol 0 and print level and logging at most 1 (a preconditioner) no norm is computed.  Setup and Solve have
 * the HYPRE_PtrToSolverFcn signature: hand them to any *SetPrecond.  A, f and u lie all in device memory (level-scheduled
 * kernels) or all in host memory (the host solve, which the kernels reproduce bit for bit); one column.
 * Iterative triangular solves (the reference's tri_solve 0, hypre_ILUSolveLUIter): with hypre_amd_ILUSetIterativeTriSolve on,
 * each triangular solve is a fixed number of Jacobi sweeps from a zero iterate (HYPRE_ILUSetLowerJacobiIters /
 * HYPRE_ILUSetUpperJacobiIters, 5 and 5); without a lower or without an upper sweep an application leaves u as it is.  On
 * the device the factors then lie in row slices of 64 rows as well and an application is at most lower + upper launches
 * beside the product with A, whatever the number of dependency levels; the host path is reproduced bit for bit.
 * Outside the scope, refused by the setter: ilu_type other than 0 (ILUT, Schur-GMRES, NSH, RAS, ddPQ, RAP).  Iterative
 * setup has no entry point.  As a BoomerAMG level smoother: HYPRE_BoomerAMGSetSmoothType 5 | 15 above.  HYPRE_ILUSolve skips
 * the residual product when u->all_zeros is set (hypre_ParVectorSetZeros) and takes f as it is: f - A 0 is f. */
HYPRE_Int HYPRE_ILUCreate(HYPRE_Solver *solver);
HYPRE_Int HYPRE_ILUDestroy(HYPRE_Solver solver);
HYPRE_Int HYPRE_ILUSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ILUSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ILUSetType(HYPRE_Solver solver, HYPRE_Int ilu_type);                    /* 0 only */
HYPRE_Int HYPRE_ILUSetLevelOfFill(HYPRE_Solver solver, HYPRE_Int lfil);
HYPRE_Int HYPRE_ILUSetLocalReordering(HYPRE_Solver solver, HYPRE_Int reordering_type);   /* 0 none, 1 RCM */
/* 1 only.  The iterative solves the reference selects with 0 are served by hypre_amd_ILUSetIterativeTriSolve below; this
 * setter goes on refusing 0, as the tests that came with it pin. */
HYPRE_Int HYPRE_ILUSetTriSolve(HYPRE_Solver solver, HYPRE_Int tri_solve);
HYPRE_Int HYPRE_ILUSetLowerJacobiIters(HYPRE_Solver solver, HYPRE_Int lower_jacobi_iters);   /* >= 0, default 5 */
HYPRE_Int HYPRE_ILUSetUpperJacobiIters(HYPRE_Solver solver, HYPRE_Int upper_jacobi_iters);   /* >= 0, default 5 */
/* 0 (default): direct triangular solves; 1: Jacobi sweeps.  hypre_amd_ILUGetParameters then reports tri_solve 0.  May be
 * changed between two solves of one Setup. */
HYPRE_Int hypre_amd_ILUSetIterativeTriSolve(HYPRE_Solver solver, HYPRE_Int iterative);
/* The switch, the sweeps per factor, the launches of the last application on the device (0 after a host one) and the
 * entries of L and U in the slice form with its padding (0 before Setup).  Any pointer may be NULL. */
HYPRE_Int hypre_amd_ILUGetIterativeStats(HYPRE_Solver solver, HYPRE_Int *iterative, HYPRE_Int *lower_jacobi_iters, HYPRE_Int *upper_jacobi_iters,
                                         HYPRE_Int *launches_per_application, HYPRE_BigInt *padded_nnz_L, HYPRE_BigInt *padded_nnz_U);
HYPRE_Int HYPRE_ILUSetMaxIter(HYPRE_Solver solver, HYPRE_Int max_iter);
HYPRE_Int HYPRE_ILUSetTol(HYPRE_Solver solver, HYPRE_Real tol);
HYPRE_Int HYPRE_ILUSetPrintLevel(HYPRE_Solver solver, HYPRE_Int print_level);
HYPRE_Int HYPRE_ILUSetLogging(HYPRE_Solver solver, HYPRE_Int logging);
HYPRE_Int HYPRE_ILUGetNumIterations(HYPRE_Solver solver, HYPRE_Int *num_iterations);
HYPRE_Int HYPRE_ILUGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *res_norm);
/* the parameters as they stand (a new object: the defaults above); any pointer may be NULL */
HYPRE_Int hypre_amd_ILUGetParameters(HYPRE_Solver solver, HYPRE_Int *ilu_type, HYPRE_Int *lfil, HYPRE_Int *reordering, HYPRE_Int *tri_solve,
                                     HYPRE_Int *max_iter, HYPRE_Real *tol, HYPRE_Int *print_level, HYPRE_Int *logging);
/* Levels of L and of U, the launches of the last application by kernel form (run: one workgroup sweeps consecutive levels
 * of at most 1024 rows; level: a grid for one wider level; both factors together; 0 after a host solve) and the entries
 * of L and U.  Host counters; any pointer may be NULL. */
HYPRE_Int hypre_amd_ILUGetSolveStats(HYPRE_Solver solver, HYPRE_Int *levels_L, HYPRE_Int *levels_U, HYPRE_Int *run_launches,
                                     HYPRE_Int *level_launches, HYPRE_Int *nnz_L, HYPRE_Int *nnz_U);
/* The two triangular solves alone, u += (L D^-1 U)^-1 f without the product with A, in the memory f and u lie in (device
 * vectors: after a Setup with A in device memory or a Solve on device vectors).  The kernels reproduce the host solve bit
 * for bit; the residual product of a Solve is summed in another order on the device than on the host. */
HYPRE_Int hypre_amd_ILUApplyFactors(HYPRE_Solver solver, HYPRE_ParVector f, HYPRE_ParVector u);
/* The residual f - A u that the last application on the device started from: the solver's own device vector (NULL before
 * the factors are on the device).  With hypre_amd_ILUApplyFactors on host vectors a test can repeat every application of a
 * device Solve on the host from the device's own residual. */
HYPRE_Int hypre_amd_ILUGetResidual(HYPRE_Solver solver, HYPRE_ParVector *residual);
/* The factors of the last Setup on the host, in the permuted numbering (row ii is row perm[ii] of A): unit L strictly
 * lower with ascending columns, U strictly upper, D the inverse pivots.  The arrays stay the solver's. */
HYPRE_Int hypre_amd_ILUGetFactors(HYPRE_Solver solver, HYPRE_Int *n, const HYPRE_Int **perm, const HYPRE_Int **L_i, const HYPRE_Int **L_j,
                                  const HYPRE_Real **L_data, const HYPRE_Real **D_inv, const HYPRE_Int **U_i, const HYPRE_Int **U_j,
                                  const HYPRE_Real **U_data);
/* hypre_ILUGetLocalPerm on its own: perm[new] = old for an n x n pattern in host memory */
HYPRE_Int hypre_amd_ILULocalRCM(HYPRE_Int n, const HYPRE_Int *A_i, const HYPRE_Int *A_j, HYPRE_Int *perm);

#ifdef __cplusplus
}
#endif
#endif
