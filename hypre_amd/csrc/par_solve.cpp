// hypre_amd — the BoomerAMG solve phase on the device: relaxation sweeps, the
// V/W/F cycle and the outer solve loop.
//
// Reference counterparts (behaviour; the structure is MI355X-first):
//   parcsr_ls/par_relax.c:24-173,1178-1254,1506-1666   relaxation dispatcher, Jacobi, two-stage GS
//   parcsr_ls/par_relax_device.c:19-155                device smoothers
//   parcsr_ls/par_relax_interface.c:20-117             CF-ordered passes
//   parcsr_ls/par_gauss_elim.c:457-697                 coarsest-level solve
//   parcsr_ls/par_cycle.c:23-803                       cycle state machine
//   parcsr_ls/par_amg_solve.c:22-424                   outer loop, convergence test
//
// What is different from the reference's device path:
//   * a Jacobi / l1-Jacobi sweep is ONE pass over the matrix (SpMV with the
//     update fused into the row epilogue) instead of copy + SpMV + elementwise;
//   * sweeps are out-of-place and every level ping-pongs between two solution
//     buffers, so no copy-back pass exists inside a cycle;
//   * nothing inside a cycle synchronises with the host (the reference syncs
//     after every vector op and SpMV); one stream sync ends the cycle;
//   * the coarsest-level elimination runs on the device from precomputed
//     factors instead of a device->host->device round trip per cycle.
#include "amg_internal.hpp"
#include <algorithm>
#include <cmath>
#include <string>

using namespace hamd;

namespace hamd {

void AmgPrivate::drop_graph()
{
   if (graph_exec) { (void) hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
   if (graph) { (void) hipGraphDestroy(graph); graph = nullptr; }
   graph_state = 0; graph_sig = 0; graph_launches = 0;
   graph_cur.clear();
}

void AmgPrivate::release_mv_levels()
{
   for (MvLevel &m : mv_lev) { plan_free(m.f); plan_free(m.home); plan_free(m.alt); }
   mv_lev.clear();
   plan_free(mv_vtemp); mv_vtemp = nullptr;
   mv_cols = 0; mv_first = -1;
}

void AmgPrivate::release_device()
{
   drop_graph();
   release_mv_levels();
   graph_level = -1;
   for (double *p : u_alt) { if (p) { hypre_Free(p, HYPRE_MEMORY_DEVICE); } }
   u_alt.clear(); u_alt_len.clear();
   for (double *p : diag_buf) { if (p) { hypre_Free(p, HYPRE_MEMORY_DEVICE); } }
   diag_buf.clear(); diag_len.clear();
   if (d_coarse_lu) { hypre_Free(d_coarse_lu, HYPRE_MEMORY_DEVICE); d_coarse_lu = nullptr; }
   if (d_coarse_rhs) { hypre_Free(d_coarse_rhs, HYPRE_MEMORY_DEVICE); d_coarse_rhs = nullptr; }
   coarse_n = 0;
   if (tail_image) { (void) hipFree(tail_image); tail_image = nullptr; }
   tail_image_sig = 0; small_tail_level = -2; small_tail_used = -2; tail_outside = -1;
   if (mp_r) { hypre_ParVectorDestroy(mp_r); mp_r = nullptr; }
   if (mp_e) { hypre_ParVectorDestroy(mp_e); mp_e = nullptr; }
   if (mv_resid) { hypre_ParVectorDestroy(mv_resid); mv_resid = nullptr; }
   if (d_cg_scalars) { hypre_Free(d_cg_scalars, HYPRE_MEMORY_DEVICE); d_cg_scalars = nullptr; }
}

double *AmgPrivate::level_diag(int level, int n)
{
   if ((int) diag_buf.size() <= level) { diag_buf.resize((size_t) level + 1, nullptr); diag_len.resize((size_t) level + 1, 0); }
   if (diag_len[(size_t) level] < n || !diag_buf[(size_t) level])
   {
      if (diag_buf[(size_t) level]) { hypre_Free(diag_buf[(size_t) level], HYPRE_MEMORY_DEVICE); drop_graph(); graph_state = 0; }
      diag_buf[(size_t) level] = hypre_TAlloc(double, (size_t) std::max(n, 1), HYPRE_MEMORY_DEVICE);
      diag_len[(size_t) level] = n;
   }
   return diag_buf[(size_t) level];
}

// ---------------------------------------------------------------------------
// raw-pointer cores
// ---------------------------------------------------------------------------
static inline void wrap(hypre_Vector *v, const double *data, int size)
{
   memset(v, 0, sizeof(*v));
   v->data = const_cast<double *>(data);
   v->size = size; v->num_vectors = 1; v->vecstride = size; v->idxstride = 1;
   v->memory_location = HYPRE_MEMORY_DEVICE;
}
static inline void wrap_par(hypre_ParVector *pv, hypre_Vector *lv, MPI_Comm comm, HYPRE_BigInt gsize)
{
   memset(pv, 0, sizeof(*pv));
   pv->comm = comm; pv->global_size = gsize; pv->local_vector = lv;
}

void dev_par_matvec(HYPRE_Complex alpha, hypre_ParCSRMatrix *A, const double *x, HYPRE_Complex beta,
                    const double *b, double *y)
{
   hypre_Vector xv, bv, yv;
   hypre_ParVector xp, bp, yp;
   wrap(&xv, x, A->diag->num_cols); wrap(&bv, b, A->diag->num_rows); wrap(&yv, y, A->diag->num_rows);
   wrap_par(&xp, &xv, A->comm, A->global_num_cols);
   wrap_par(&bp, &bv, A->comm, A->global_num_rows);
   wrap_par(&yp, &yv, A->comm, A->global_num_rows);
   hypre_ParCSRMatrixMatvecOutOfPlaceDevice(alpha, A, &xp, beta, &bp, &yp);
}

void dev_par_matvecT(HYPRE_Complex alpha, hypre_ParCSRMatrix *A, const double *x, HYPRE_Complex beta, double *y)
{
   hypre_Vector xv, yv;
   hypre_ParVector xp, yp;
   wrap(&xv, x, A->diag->num_rows); wrap(&yv, y, A->diag->num_cols);
   wrap_par(&xp, &xv, A->comm, A->global_num_rows);
   wrap_par(&yp, &yv, A->comm, A->global_num_cols);
   hypre_ParCSRMatrixMatvecTDevice(alpha, A, &xp, beta, &yp);
}

// u_out = u_in + (w f - w A u_in)./d  on rows with cf_marker == relax_points
// (all rows when relax_points == 0); other rows are copied.  Single rank: one
// fused pass.  Distributed: the interior pass is fused as well and the ghost
// couplings are folded in by a second, halo-sized pass.
void dev_jacobi_sweep(hypre_ParCSRMatrix *A, const double *f, const int *cf_marker, int relax_points,
                      double w, const double *d, const double *u_in, double *u_out)
{
   hipStream_t s = stream();
   hypre_CSRMatrix *diag = A->diag;
   const int n = diag->num_rows;
   if (n <= 0) { return; }
   HYPRE_Int nprocs;
   hypre_MPI_Comm_size(A->comm, &nprocs);
   // distributed: start the halo of u_in, run the fused interior sweep while it
   // travels, then fold the ghost couplings into the boundary rows
   //    u_out[row] -= w * (A_offd u_ghost)[row] / d[row]        (halo-sized pass)
   hypre_ParCSRCommHandle *ch = nprocs > 1 ? dev_halo_begin(A, u_in) : nullptr;
   SpmvPlan *plan = get_plan(diag);
   SpmvArgs a{};
   a.Ai = diag->i; a.Aj = diag->j; a.Aa = diag->data; a.Aa32 = nullptr;
   a.x = u_in; a.b = f; a.y = u_out; a.aux = nullptr; a.d = d;
   a.marker = cf_marker; a.marker_val = relax_points;
   a.alpha = w; a.beta = 0.0; a.fill = HYPRE_SPMV_FILL_WHOLE; a.row_offset = 0;
   spmv_default_flags(a);
   launch_spmv(plan, a, (relax_points != 0 && cf_marker) ? OP_JACOBI_CF : OP_JACOBI, s);
   dev_halo_end(ch);
   hypre_CSRMatrix *offd = A->offd;
   if (nprocs > 1 && offd->num_cols > 0 && offd->num_nonzeros > 0)
   {
      SpmvArgs o{};
      o.Ai = offd->i; o.Aj = offd->j; o.Aa = offd->data;
      o.Aa32 = handle().fp32_values ? fp32_values_of(offd) : nullptr;     // mixed precision covers the ghost block too
      o.x = A->comm_pkg->tmp_data; o.y = u_out; o.d = d;
      o.marker = (relax_points != 0) ? cf_marker : nullptr; o.marker_val = relax_points;
      o.alpha = -w;
      if (offd->rownnz) { launch_spmv_rownnz(offd->rownnz, offd->num_rownnz, o, s); }
      else { launch_spmv_allrows_update(offd->num_rows, o, s); }
   }
}

}  // namespace hamd

// per-matrix scratch for the in-place public relax entry (result lands in the
// caller's u, so one extra vector is needed for the out-of-place sweep)
static double *relax_scratch(size_t n)
{
   static double *buf = nullptr;
   static size_t len = 0;
   if (len < n)
   {
      if (buf) { hypre_Free(buf, HYPRE_MEMORY_DEVICE); }
      buf = hypre_TAlloc(double, n, HYPRE_MEMORY_DEVICE);
      len = n;
   }
   return buf;
}
static double *diag_scratch(size_t n)
{
   static double *buf = nullptr;
   static size_t len = 0;
   if (len < n)
   {
      if (buf) { hypre_Free(buf, HYPRE_MEMORY_DEVICE); }
      buf = hypre_TAlloc(double, n, HYPRE_MEMORY_DEVICE);
      len = n;
   }
   return buf;
}

namespace { int &cycle_fusion(); int &smoother_fusion(); int &small_tail_on(); int &small_tail_forced_form(); }    // (defined with the cycle below)

extern "C" {

// ===========================================================================
// relaxation (public, in-place on u as the reference)
// ===========================================================================
HYPRE_Int hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(hypre_ParCSRMatrix *A, hypre_ParVector *f,
                                                        HYPRE_Real relax_weight, HYPRE_Real omega,
                                                        HYPRE_Real *A_diag_diag, hypre_ParVector *u,
                                                        hypre_ParVector *r, hypre_ParVector *z,
                                                        HYPRE_Int num_inner_iters)
{
   (void) omega;
   hipStream_t s = stream();
   hypre_CSRMatrix *diag = A->diag;
   const int n = diag->num_rows;
   double *ud = u->local_vector->data, *rd = r->local_vector->data, *zd = z->local_vector->data;
   QuietSync quiet;
   // 0) r = w (f - A u)     1) z = r./D ; u += z
   // u known to be zero (par_vector.h all_zeros; set by SetZeros and by the cycle on the way down):
   // A u = 0 exactly, so r = w f without touching the matrix.  The reference uses the flag this way
   // only in its Jacobi sweep (par_relax.c:1221-1228); the result here is the same bits either way.
   HYPRE_Int nprocs = 1;
   hypre_MPI_Comm_size(A->comm, &nprocs);
   hypre_CSRMatrix *Lm = (n > 0 && diag->num_nonzeros > 0) ? strict_lower_of(diag) : nullptr;
   // At least one inner step over a non-empty triangle (hypre_amd_SetCycleFusion): on one rank the sweep in two or three
   // passes instead of four or five — stage 0 and the scaling of stage 1 in one kernel (z = (w f - w A u) .* (1 ./ D): an
   // epilogue of the residual's pass; from a zero iterate one vector kernel), and the "u += z" of stage 1 folded into the
   // first inner step's epilogue (u = (u + z) + mult z'): every rounding where it was, 24 - 32 bytes per row less.
   // Several ranks: the residual needs the ghost block's part before it can be scaled, so it stays a pass of its own, the
   // scaling a vector kernel (z = r .* (1 ./ D), without the "u += z"), and the first inner step — local by construction: the
   // triangle of this rank's own diagonal block — folds the "u += z" in all the same.
   const bool fused = cycle_fusion() && Lm && Lm->num_nonzeros > 0 && num_inner_iters >= 1;
   const bool one_rank = nprocs == 1 && A->offd->num_nonzeros == 0;
   const bool from_zero = u->all_zeros != 0;
   if (fused)
   {
      if (from_zero) { launch_scaled_recip(relax_weight, f->local_vector->data, A_diag_diag, zd, (size_t) n, s); }
      else if (!one_rank)
      {
         dev_par_matvec(-relax_weight, A, ud, relax_weight, f->local_vector->data, rd);
         launch_scaled_recip(1.0, rd, A_diag_diag, zd, (size_t) n, s);           // (1.0 * r is r: the product with the reciprocal as before)
      }
      else
      {
         SpmvArgs a{};
         a.Ai = diag->i; a.Aj = diag->j; a.Aa = diag->data; a.Aa32 = nullptr;
         a.x = ud; a.b = f->local_vector->data; a.y = zd; a.aux = nullptr; a.d = A_diag_diag; a.marker = nullptr;
         a.alpha = -relax_weight; a.beta = relax_weight; a.fill = HYPRE_SPMV_FILL_WHOLE;
         spmv_default_flags(a);
         launch_spmv(get_plan(diag), a, OP_RESID_RD, s);
      }
   }
   else
   {
      if (from_zero) { launch_scale_copy(relax_weight, f->local_vector->data, rd, (size_t) n, s); }
      else { dev_par_matvec(-relax_weight, A, ud, relax_weight, f->local_vector->data, rd); }
      launch_diagscale2(A_diag_diag, rd, 1.0, zd, ud, 1, (size_t) n, s);
   }
   double mult = -1.0;
   double *zin = zd, *zout = rd;
   if (Lm)
   {
      // the inner steps run on a cached copy of the strictly lower triangle (half the bytes of
      // masking the full matrix, which is what the reference's fill-mode SpMV does)
      SpmvPlan *plan = get_plan(Lm);
      for (int k = 0; k < num_inner_iters && Lm->num_nonzeros > 0; k++)
      {
         if (fused && k == 0)
         {
            // z' = (L z)./D ; u = (u + z) + mult z'   (u is not read when it is known to be zero)
            SpmvArgs a{};
            a.Ai = Lm->i; a.Aj = Lm->j; a.Aa = Lm->data; a.Aa32 = nullptr;
            a.x = zin; a.b = nullptr; a.y = zout; a.aux = ud; a.d = A_diag_diag; a.marker = nullptr;
            a.alpha = mult; a.beta = from_zero ? 0.0 : 1.0; a.fill = HYPRE_SPMV_FILL_WHOLE;
            spmv_default_flags(a);
            launch_spmv(plan, a, OP_TSGS_FIRST, s);
            std::swap(zin, zout);
            mult *= -1.0;
            continue;
         }
         // 2+3) z_out = (L_strict z_in)./D ; u += mult * z_out   — one fused pass
         SpmvArgs a{};
         a.Ai = Lm->i; a.Aj = Lm->j; a.Aa = Lm->data; a.Aa32 = nullptr;
         a.x = zin; a.b = nullptr; a.y = zout; a.aux = ud; a.d = A_diag_diag; a.marker = nullptr;
         a.alpha = mult; a.beta = 0.0; a.fill = HYPRE_SPMV_FILL_WHOLE;
         spmv_default_flags(a);
         launch_spmv(plan, a, OP_TSGS, s);
         std::swap(zin, zout);
         mult *= -1.0;
      }
   }
   u->all_zeros = 0;
   quiet.restore();
   maybe_sync();
   return hypre_error_flag;
}

HYPRE_Int hypre_BoomerAMGRelax(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                               HYPRE_Int relax_type, HYPRE_Int relax_points, HYPRE_Real relax_weight,
                               HYPRE_Real omega, HYPRE_Real *l1_norms, hypre_ParVector *u,
                               hypre_ParVector *Vtemp, hypre_ParVector *Ztemp)
{
   HYPRE_AMD_REQUIRE_DEVICE(A->diag->memory_location, "hypre_BoomerAMGRelax(A)");
   HYPRE_AMD_REQUIRE_DEVICE(u->local_vector->memory_location, "hypre_BoomerAMGRelax(u)");
   HYPRE_AMD_REQUIRE_DEVICE(f->local_vector->memory_location, "hypre_BoomerAMGRelax(f)");
   hipStream_t s = stream();
   const int n = A->diag->num_rows;
   QuietSync quiet;
   double *ud = u->local_vector->data;
   const double *fd = f->local_vector->data;
   switch (relax_type)
   {
      case 0: case 7: case 18:
      {
         // smoother diagonal: l1 norms (18), stored diagonal vector (7), first row entry (0)
         const double *d = l1_norms;
         if (relax_type == 0 || !d)
         {
            double *dd = diag_scratch((size_t) std::max(n, 1));
            launch_diag_first(A->diag->i, A->diag->data, dd, n, s);
            d = dd;
         }
         if (u->all_zeros && relax_type != 0)
         {
            // par_relax.c:1221-1228: u == 0 => u = (w f)./d, no SpMV
            launch_scaled_div(relax_weight, fd, d, ud, relax_points ? cf_marker : nullptr, relax_points, (size_t) n, s);
         }
         else
         {
            double *tmp = relax_scratch((size_t) std::max(n, 1));
            dev_jacobi_sweep(A, fd, cf_marker, relax_points, relax_weight, d, ud, tmp);
            launch_copy(ud, tmp, (size_t) n, s);
         }
         break;
      }
      case 11:
         hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(A, f, relax_weight, omega, l1_norms, u, Vtemp, Ztemp, 1);
         break;
      case 12:
         hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(A, f, relax_weight, omega, l1_norms, u, Vtemp, Ztemp, 2);
         break;
      // hybrid Gauss-Seidel / SOR family (par_relax.c:1256-1377): plain 3 forward, 4 backward,
      // 6 symmetric; l1-scaled 13 forward, 14 backward, 8/88 symmetric, 89 = 13 then 14
      case 3:
         hypre_BoomerAMGRelaxHybridGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, omega, nullptr, u, Vtemp, Ztemp, 1, 0);
         break;
      case 4:
         hypre_BoomerAMGRelaxHybridGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, omega, nullptr, u, Vtemp, Ztemp, -1, 0);
         break;
      case 6:
         hypre_BoomerAMGRelaxHybridGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, omega, nullptr, u, Vtemp, Ztemp, 1, 1);
         break;
      case 8: case 88: case 13: case 14: case 89:
         if (!l1_norms)
         {
            hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGRelax: the l1 Gauss-Seidel variants need l1_norms");
            break;
         }
         if (relax_type == 8 || relax_type == 88) { hypre_BoomerAMGRelaxHybridGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, omega, l1_norms, u, Vtemp, Ztemp, 1, 1); }
         if (relax_type == 13 || relax_type == 89) { hypre_BoomerAMGRelaxHybridGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, omega, l1_norms, u, Vtemp, Ztemp, 1, 0); }
         if (relax_type == 14 || relax_type == 89) { hypre_BoomerAMGRelaxHybridGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, omega, l1_norms, u, Vtemp, Ztemp, -1, 0); }
         break;
      // multicolour Gauss-Seidel (no reference counterpart; par_relax_mc.cpp): 21 colours ascending, 22 descending
      case 21:
         hypre_BoomerAMGRelaxMultiColorGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, l1_norms, u, Vtemp, 1);
         break;
      case 22:
         hypre_BoomerAMGRelaxMultiColorGaussSeidelDevice(A, f, cf_marker, relax_points, relax_weight, l1_norms, u, Vtemp, -1);
         break;
      default:
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGRelax: relax_type is outside the scope of this library");
         break;
   }
   u->all_zeros = 0;
   quiet.restore();
   maybe_sync();
   return 0;     // relax_error (par_relax.c:36,172)
}

HYPRE_Int hypre_BoomerAMGRelaxIF(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                                 HYPRE_Int relax_type, HYPRE_Int relax_order, HYPRE_Int cycle_param,
                                 HYPRE_Real relax_weight, HYPRE_Real omega, HYPRE_Real *l1_norms,
                                 hypre_ParVector *u, hypre_ParVector *Vtemp, hypre_ParVector *Ztemp)
{
   HYPRE_Int err = 0;
   if (relax_order == 1 && cycle_param < 3)
   {
      const HYPRE_Int pts[2] = {cycle_param < 2 ? 1 : -1, cycle_param < 2 ? -1 : 1};
      for (int i = 0; i < 2; i++)
      {
         err = hypre_BoomerAMGRelax(A, f, cf_marker, relax_type, pts[i], relax_weight, omega, l1_norms, u, Vtemp, Ztemp);
      }
   }
   else
   {
      err = hypre_BoomerAMGRelax(A, f, cf_marker, relax_type, 0, relax_weight, omega, l1_norms, u, Vtemp, Ztemp);
   }
   return err;
}

HYPRE_Int hypre_ParCSRRelax_L1_Jacobi(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                                      HYPRE_Int relax_points, HYPRE_Real relax_weight, HYPRE_Real *l1_norms,
                                      hypre_ParVector *u, hypre_ParVector *Vtemp)
{
   return hypre_BoomerAMGRelax(A, f, cf_marker, 18, relax_points, relax_weight, 0.0, l1_norms, u, Vtemp, nullptr);
}

HYPRE_Int hypre_BoomerAMGRelax_FCFJacobi(hypre_ParCSRMatrix *A, hypre_ParVector *f, HYPRE_Int *cf_marker,
                                         HYPRE_Real relax_weight, hypre_ParVector *u, hypre_ParVector *Vtemp)
{
   const HYPRE_Int pts[3] = {-1, 1, -1};
   for (int i = 0; i < 3; i++) { hypre_BoomerAMGRelax(A, f, cf_marker, 0, pts[i], relax_weight, 0.0, nullptr, u, Vtemp, nullptr); }
   return hypre_error_flag;
}

// ===========================================================================
// coarsest level
// ===========================================================================
// Factor the dense operator once with the reference's elimination order; the
// device kernel then replays the right-hand-side operations of hypre_gselim.
// M (n x n, row-major) -> its factors in place: the multipliers below the diagonal (zeros below a zero pivot, whose step
// the elimination skips: the kernels then test the pivot alone), the eliminated rows on and above it
static void coarse_factors_in_place(std::vector<double> &M, int n)
{
   for (int k = 0; k < n - 1; k++)
   {
      if (M[(size_t) k * n + k] != 0.0)
      {
         const double divA = 1.0 / M[(size_t) k * n + k];
         for (int j = k + 1; j < n; j++)
         {
            if (M[(size_t) j * n + k] != 0.0)
            {
               const double factor = M[(size_t) j * n + k] * divA;
               for (int m = k + 1; m < n; m++) { M[(size_t) j * n + m] -= factor * M[(size_t) k * n + m]; }
               M[(size_t) j * n + k] = factor;      // keep the multiplier in the eliminated slot
            }
         }
      }
      else
      {
         for (int j = k + 1; j < n; j++) { M[(size_t) j * n + k] = 0.0; }
      }
   }
}

static void ensure_coarse_factors(hypre_ParAMGData *d)
{
   AmgPrivate *pv = (AmgPrivate *) d->amd_private;
   if (pv->d_coarse_lu || !d->A_mat) { return; }
   hypre_ParCSRMatrix *A = d->A_array[d->num_levels - 1];
   const int n = (int) A->global_num_rows;
   std::vector<double> M(d->A_mat, d->A_mat + (size_t) n * n);
   coarse_factors_in_place(M, n);
   pv->coarse_n = n;
   pv->coarse_first_row = (int) A->first_row_index;
   pv->d_coarse_lu = hypre_TAlloc(double, (size_t) std::max(n * n, 1), HYPRE_MEMORY_DEVICE);
   pv->d_coarse_rhs = hypre_TAlloc(double, (size_t) std::max(n, 1), HYPRE_MEMORY_DEVICE);
   hypre_TMemcpy(pv->d_coarse_lu, M.data(), double, (size_t) n * n, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
}

HYPRE_Int hypre_GaussElimSolve(hypre_ParAMGData *d, HYPRE_Int level, HYPRE_Int relax_type)
{
   (void) relax_type;
   AmgPrivate *pv = (AmgPrivate *) d->amd_private;
   hypre_ParCSRMatrix *A = d->A_array[level];
   if (!d->gs_setup) { hypre_GaussElimSetup(d, level, relax_type); }
   ensure_coarse_factors(d);
   hipStream_t s = stream();
   const int n = pv->coarse_n, nloc = A->diag->num_rows;
   double *fd = d->F_array[level]->local_vector->data;
   double *ud = d->U_array[level]->local_vector->data;
   HYPRE_Int nprocs;
   hypre_MPI_Comm_size(A->comm, &nprocs);
   if (nprocs == 1)
   {
      HIP_CHECK(hipMemcpyAsync(pv->d_coarse_rhs, fd, sizeof(double) * (size_t) n, hipMemcpyDeviceToDevice, s));
      launch_coarse_solve(pv->d_coarse_lu, pv->d_coarse_rhs, n, s);
      HIP_CHECK(hipMemcpyAsync(ud, pv->d_coarse_rhs, sizeof(double) * (size_t) n, hipMemcpyDeviceToDevice, s));
   }
   else
   {
      // gather the (<= max_coarse_size) right-hand side on every rank: zero-fill,
      // drop the own slice in, sum over ranks (one tiny all-reduce instead of an
      // Allgatherv through the host, par_gauss_elim.c:575)
      HIP_CHECK(hipMemsetAsync(pv->d_coarse_rhs, 0, sizeof(double) * (size_t) n, s));
      if (nloc) { HIP_CHECK(hipMemcpyAsync(pv->d_coarse_rhs + pv->coarse_first_row, fd, sizeof(double) * (size_t) nloc, hipMemcpyDeviceToDevice, s)); }
      dev_allreduce_sum(A->comm, pv->d_coarse_rhs, n);
      launch_coarse_solve(pv->d_coarse_lu, pv->d_coarse_rhs, n, s);
      if (nloc) { HIP_CHECK(hipMemcpyAsync(ud, pv->d_coarse_rhs + pv->coarse_first_row, sizeof(double) * (size_t) nloc, hipMemcpyDeviceToDevice, s)); }
   }
   return hypre_error_flag;
}

// Test hook: the coarsest level's solve on its own.  a (n x n, row-major) and b are host arrays; the factors are the ones
// ensure_coarse_factors makes, the kernel the one launch_coarse_solve picks (form 0) or the one-lane kernel (form 1).
HYPRE_Int hypre_amd_CoarseSolveTest(const HYPRE_Real *a, HYPRE_Int n, const HYPRE_Real *b, HYPRE_Int form, HYPRE_Real *x)
{
   if (n < 1 || !a || !b || !x || form < 0 || form > 1) { hypre_error_in_arg(n < 1 ? 2 : 4); return hypre_error_flag; }
   std::vector<double> M(a, a + (size_t) n * n);
   coarse_factors_in_place(M, n);
   hipStream_t s = stream();
   double *d_lu = hypre_TAlloc(double, (size_t) n * n, HYPRE_MEMORY_DEVICE);
   double *d_x = hypre_TAlloc(double, (size_t) n, HYPRE_MEMORY_DEVICE);
   hypre_TMemcpy(d_lu, M.data(), double, (size_t) n * n, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
   hypre_TMemcpy(d_x, b, double, (size_t) n, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
   launch_coarse_solve(d_lu, d_x, n, s, form);
   HIP_CHECK(hipStreamSynchronize(s));
   hypre_TMemcpy(x, d_x, double, (size_t) n, HYPRE_MEMORY_HOST, HYPRE_MEMORY_DEVICE);
   hypre_TFree(d_lu, HYPRE_MEMORY_DEVICE);
   hypre_TFree(d_x, HYPRE_MEMORY_DEVICE);
   return hypre_error_flag;
}

// ===========================================================================
// the cycle
// ===========================================================================
namespace {

// where a level's current iterate lives: its home vector or the alternate
struct LevelVec
{
   double *home = nullptr, *alt = nullptr, *cur = nullptr;
   double *other() const { return cur == home ? alt : home; }
   void flip() { cur = other(); }
};

// Levels pv->tail_level and below on this rank's replica (par_amg_replicate.cpp): gather f, cycle, keep own slice.
int run_replicated_tail(hypre_ParAMGData *d, AmgPrivate *pv, const double *f_local, double *u_local, double *op_count)
{
   hypre_ParAMGData *t = pv->tail;
   hypre_ParCSRMatrix *Al = d->A_array[pv->tail_level];
   const int nloc = Al->diag->num_rows;
   const size_t first = (size_t) Al->row_starts[0];
   const int ng = (int) t->A_array[0]->global_num_rows;
   hipStream_t s = stream();
   double *g = pv->d_tail_f;
   HIP_CHECK(hipMemsetAsync(g, 0, sizeof(double) * (size_t) ng, s));
   if (nloc) { HIP_CHECK(hipMemcpyAsync(g + first, f_local, sizeof(double) * (size_t) nloc, hipMemcpyDeviceToDevice, s)); }
   dev_allreduce_sum(Al->comm, g, ng);
   HIP_CHECK(hipMemcpyAsync(t->F_array[0]->local_vector->data, g, sizeof(double) * (size_t) ng, hipMemcpyDeviceToDevice, s));
   hypre_ParVectorSetZeros(t->U_array[0]);
   ((AmgPrivate *) t->amd_private)->mixed_precision = pv->mixed_precision;     // may have been switched after setup
   t->cycle_op_count = 0;
   const int err = hypre_BoomerAMGCycle(t, t->F_array, t->U_array);
   if (nloc)
   {
      HIP_CHECK(hipMemcpyAsync(u_local, t->U_array[0]->local_vector->data + first, sizeof(double) * (size_t) nloc,
                               hipMemcpyDeviceToDevice, s));
   }
   if (op_count) { *op_count += t->cycle_op_count; }
   return err;
}

// fusions across the cycle's steps (hypre_amd_SetCycleFusion; HYPRE_AMD_CYCLE_FUSION=0): same results, fewer passes
int &cycle_fusion()
{
   static int on = [] { const char *e = getenv("HYPRE_AMD_CYCLE_FUSION"); return e ? atoi(e) : 1; }();
   return on;
}
// the smallest levels of a Jacobi V(1,1) cycle in one kernel of one workgroup (tail_kernels.hip; hypre_amd_SetSmallTail)
int &smoother_fusion()
{
   static int on = [] { const char *e = getenv("HYPRE_AMD_SMOOTHER_FUSION"); return e ? atoi(e) : 1; }();
   return on;
}

int &small_tail_on()
{
   static int on = [] { const char *e = getenv("HYPRE_AMD_SMALL_TAIL"); return e ? atoi(e) : 1; }();
   return on;
}
// The image of levels st .. L-1 the one-workgroup tail copies into LDS (tail_kernels.hip): every array the walk reads, at the
// offset the kernel addresses it, and behind it the room of the work vectors.  Built when the hierarchy (its arrays'
// addresses) is new; false: the levels do not fit the LDS of one workgroup.
// form: 0 every array in LDS; 1 the first level's operator in the lanes' registers (its rows times their lanes fit the
// workgroup's 768 lanes, a lane's share is at most 32 entries); 2 the first level's operator streamed from where it lies
bool build_small_tail_image(hypre_ParAMGData *d, AmgPrivate *pv, int st, hipStream_t s, int form = 0)
{
   const bool first_operator_outside = form != 0;
   const int L = d->num_levels;
   hypre_ParCSRMatrix **A = d->A_array, **P = d->P_array;
   unsigned long long h = 1469598103934665603ull;
   auto mix = [&](unsigned long long v) { h ^= v; h *= 1099511628211ull; };
   mix((unsigned long long) st); mix((unsigned long long) L); mix((unsigned long long) (uintptr_t) pv->d_coarse_lu); mix((unsigned long long) pv->coarse_n);
   mix((unsigned long long) form);
   for (int l = st; l < L; l++)
   {
      mix((unsigned long long) (uintptr_t) A[l]->diag->i); mix((unsigned long long) (uintptr_t) A[l]->diag->data); mix((unsigned long long) A[l]->diag->num_nonzeros);
      if (l < L - 1)
      {
         mix((unsigned long long) (uintptr_t) P[l]->diag->data); mix((unsigned long long) (uintptr_t) P[l]->diagT->data);
         mix((unsigned long long) (uintptr_t) d->l1_norms[l]->data);
      }
   }
   if (pv->tail_image && pv->tail_image_sig == h) { return true; }
   if (pv->tail_image) { (void) hipFree(pv->tail_image); pv->tail_image = nullptr; pv->tail_image_sig = 0; }
   int reg_lanes = 0;
   if (form == 1)
   {
      // lanes per row of the register form: enough that a lane holds at most 16 entries of the longest row, few enough that
      // all rows fit the workgroup at once
      hypre_CSRMatrix *Ad = A[st]->diag;
      std::vector<HYPRE_Int> ri((size_t) Ad->num_rows + 1);
      HIP_CHECK(hipStreamSynchronize(s));
      hypre_TMemcpy(ri.data(), Ad->i, HYPRE_Int, Ad->num_rows + 1, HYPRE_MEMORY_HOST, HYPRE_MEMORY_DEVICE);
      int longest = 0;
      for (HYPRE_Int r = 0; r < Ad->num_rows; r++) { longest = std::max(longest, (int) (ri[(size_t) r + 1] - ri[(size_t) r])); }
      // (the lanes per row the other forms take, where a lane's share then fits its registers: the same order of the sums)
      // (the register form runs 768 lanes, a lane holding at most 32 entries: tail_kernels.hip)
      int wmax = 1, wlen = 1;
      while (2 * wmax <= 64 && 2LL * wmax * std::max((int) Ad->num_rows, 1) <= 768) { wmax *= 2; }
      const int avg = Ad->num_rows > 0 ? (int) ((Ad->num_nonzeros + Ad->num_rows - 1) / Ad->num_rows) : 1;
      while (wlen < avg && wlen < 64) { wlen *= 2; }
      int W = std::min(wmax, wlen);
      while (32 * W < longest && W < 64) { W *= 2; }
      if (32 * W < longest || (long long) W * Ad->num_rows > 768 || Ad->num_nonzeros < 1) { return false; }
      reg_lanes = W;
   }
   SmallTailArgs &ta = pv->tail_args;
   ta = SmallTailArgs{};
   int off = 0;
   auto take = [&](size_t bytes) { const int o = off; off += (int) ((bytes + 15) & ~(size_t) 15); return o; };
   auto lanes = [](int rows, int entries)
   {
      int wmax = 1, wlen = 1;
      while (2 * wmax <= 64 && 2 * wmax * std::max(rows, 1) <= 1024) { wmax *= 2; }
      const int avg = rows > 0 ? (entries + rows - 1) / rows : 1;
      while (wlen < avg && wlen < 64) { wlen *= 2; }
      return std::min(wmax, wlen);
   };
   struct Piece { const void *src; int off; size_t bytes; };
   std::vector<Piece> pieces;
   auto put = [&](const void *src, size_t bytes) { const int o = take(bytes); pieces.push_back({src, o, bytes}); return o; };
   ta.nl = L - st;
   for (int l = st; l < L - 1; l++)
   {
      SmallTailLevel &q = ta.lv[l - st];
      hypre_CSRMatrix *Ad = A[l]->diag, *Pd = P[l]->diag, *Rd = P[l]->diagT;
      q.n = Ad->num_rows;
      q.Ai = put(Ad->i, sizeof(int) * ((size_t) Ad->num_rows + 1));
      if (l == st && first_operator_outside) { q.gAj = Ad->j; q.gAa = Ad->data; ta.gAi = Ad->i; ta.nnz0 = Ad->num_nonzeros; }
      else
      {
         q.Aj = put(Ad->j, sizeof(int) * (size_t) Ad->num_nonzeros);
         q.Aa = put(Ad->data, sizeof(double) * (size_t) Ad->num_nonzeros);
      }
      q.Pi = put(Pd->i, sizeof(int) * ((size_t) Pd->num_rows + 1)); q.Pj = put(Pd->j, sizeof(int) * (size_t) Pd->num_nonzeros);
      q.Pa = put(Pd->data, sizeof(double) * (size_t) Pd->num_nonzeros);
      q.Ri = put(Rd->i, sizeof(int) * ((size_t) Rd->num_rows + 1)); q.Rj = put(Rd->j, sizeof(int) * (size_t) Rd->num_nonzeros);
      q.Ra = put(Rd->data, sizeof(double) * (size_t) Rd->num_nonzeros);
      q.d = put(d->l1_norms[l]->data, sizeof(double) * (size_t) Ad->num_rows);
      q.wA = lanes(Ad->num_rows, Ad->num_nonzeros); q.wP = lanes(Pd->num_rows, Pd->num_nonzeros); q.wR = lanes(Rd->num_rows, Rd->num_nonzeros);
      if (l == st && form == 1) { q.wA = reg_lanes; ta.reg_first = 1; }
   }
   ta.lv[L - 1 - st].n = A[L - 1]->diag->num_rows;
   ta.ncoarse = pv->coarse_n;
   ta.lu_off = put(pv->d_coarse_lu, sizeof(double) * (size_t) pv->coarse_n * (size_t) pv->coarse_n);
   ta.image_bytes = off;
   for (int l = st; l < L; l++)
   {
      SmallTailLevel &q = ta.lv[l - st];
      q.f = take(sizeof(double) * (size_t) q.n); q.u = take(sizeof(double) * (size_t) q.n); q.alt = take(sizeof(double) * (size_t) q.n);
   }
   ta.vt_off = take(sizeof(double) * (size_t) ta.lv[0].n);
   ta.lds_bytes = off;
   if (off > 158 * 1024) { ta = SmallTailArgs{}; return false; }
   if (hipMalloc(&pv->tail_image, (size_t) std::max(ta.image_bytes, 16)) != hipSuccess) { (void) hipGetLastError(); pv->tail_image = nullptr; return false; }
   for (const Piece &pc : pieces)
   {
      if (pc.bytes) { HIP_CHECK(hipMemcpyAsync((char *) pv->tail_image + pc.off, pc.src, pc.bytes, hipMemcpyDeviceToDevice, s)); }
   }
   ta.image = pv->tail_image;
   pv->tail_image_sig = h;
   return true;
}

// tests: the form of the tail's image (-1: the first that fits)
int &small_tail_forced_form() { static int f = -1; return f; }
// everything the launches of the sub-cycle below level gl depend on
unsigned long long tail_signature(hypre_ParAMGData *d, AmgPrivate *pv, int gl, hypre_ParVector **F, hypre_ParVector **U)
{
   unsigned long long h = 1469598103934665603ull;
   auto mix = [&](unsigned long long v) { h ^= v; h *= 1099511628211ull; };
   auto mixd = [&](double v) { unsigned long long b; memcpy(&b, &v, sizeof b); mix(b); };
   mix((unsigned long long) d->num_levels); mix((unsigned long long) gl);
   for (int k = 0; k < 4; k++) { mix((unsigned long long) d->grid_relax_type[k]); mix((unsigned long long) d->num_grid_sweeps[k]); }
   mix((unsigned long long) d->relax_order); mix((unsigned long long) d->cycle_type); mix((unsigned long long) d->fcycle);
   mix((unsigned long long) d->user_relax_type); mix((unsigned long long) (d->grid_relax_points != nullptr));
   mix((unsigned long long) pv->mixed_precision); mix((unsigned long long) pv->emulated_threads);
   mix((unsigned long long) (uintptr_t) d->Vtemp->local_vector->data);
   for (int l = gl; l < d->num_levels; l++)
   {
      mixd(d->relax_weight[l]); mixd(d->omega[l]);
      mix((unsigned long long) (uintptr_t) d->A_array[l]->diag->data); mix((unsigned long long) (uintptr_t) d->A_array[l]->diag->j);
      mix((unsigned long long) d->A_array[l]->diag->num_nonzeros);
      if (l < d->num_levels - 1 && d->P_array[l])
      {
         mix((unsigned long long) (uintptr_t) d->P_array[l]->diag->data);
         mix((unsigned long long) (uintptr_t) (d->P_array[l]->diagT ? d->P_array[l]->diagT->data : nullptr));
      }
      mix((unsigned long long) (uintptr_t) F[l]->local_vector->data); mix((unsigned long long) (uintptr_t) U[l]->local_vector->data);
      mix((unsigned long long) (uintptr_t) (d->l1_norms[l] ? d->l1_norms[l]->data : nullptr));
      mix((unsigned long long) (uintptr_t) (l < (int) pv->u_alt.size() ? pv->u_alt[(size_t) l] : nullptr));
      mix((unsigned long long) (uintptr_t) (l < (int) pv->diag_buf.size() ? pv->diag_buf[(size_t) l] : nullptr));
   }
   mix(plan_generation());            // a plan dropped or rebuilt anywhere (the recorded kernels point into plans' tables)
   mix((unsigned long long) cycle_fusion());     // (the recorded tail leaves out what a fused restriction into it did)
   mix((unsigned long long) (small_tail_on() ? pv->small_tail_nnz : 0)); mix((unsigned long long) (small_tail_forced_form() + 1));
   mix((unsigned long long) hypre_amd_SetMcLookAhead(-1));     // (one kernel instead of a dozen launches in the recorded tail)
   SpmvArgs a{};
   spmv_default_flags(a);
   mix((unsigned long long) a.variant); mix((unsigned long long) a.gather_t); mix((unsigned long long) a.xcd_map);
   return h;
}

bool is_jacobi_type(int t) { return t == 0 || t == 7 || t == 18; }
bool is_ge_type(int t) { return t == 9 || t == 19 || t == 98 || t == 99 || t == 198 || t == 199; }

}  // namespace

// Fusions across the steps of a cycle from now on (default 1): the restriction also writes the coarse level's first sweep
// from zero.  Same bits either way; a switch for comparisons.  on < 0: unchanged; returns the setting.
HYPRE_Int hypre_amd_SetCycleFusion(HYPRE_Int on)
{
   if (on >= 0) { cycle_fusion() = on != 0; }
   return cycle_fusion();
}

// The smallest levels of a V(1,1) cycle with Jacobi-type smoothing in one kernel of one workgroup from now on (default 1):
// the levels whose operators hold at most `max_entries` entries each (default 20 000; < 0: unchanged).  The order of a
// row's sum differs from the per-level kernels' (rounding only).  on < 0: unchanged; returns the setting.
HYPRE_Int hypre_amd_SetSmallTail(HYPRE_Int on)
{
   if (on >= 0) { small_tail_on() = on != 0; }
   return small_tail_on();
}
// Test hook: the form the tail's image takes from now on — 0 every array in LDS, 1 the first level's operator in the lanes'
// registers, 2 streamed from where it lies; -1 the first of these that fits (default).  A form that does not fit a
// hierarchy moves the tail a level down.
HYPRE_Int hypre_amd_SetSmallTailForm(HYPRE_Int form)
{
   small_tail_forced_form() = (form >= 0 && form <= 2) ? form : -1;
   return hypre_error_flag;
}

// The conjugate-gradient acceleration around the ILU level smoother (smooth_type 15) with its two inner products left on the
// device from now on (default 1; ilu_smoother_kernels.hip): no read-back inside a level visit.  0: the reference's call
// sequence on the library's vector routines, two read-backs per sweep.  Same bits either way.  on < 0: unchanged; returns
// the setting.
HYPRE_Int hypre_amd_SetSmootherFusion(HYPRE_Int on)
{
   if (on >= 0) { smoother_fusion() = on != 0; }
   return smoother_fusion();
}

// Test hook: one pass of the fused acceleration's vector kernels through their launchers, on host arrays of n entries
// (V is only read) and the four scalars: [the sum <R, Z>,] the direction, [the sum <P, V>,] the update.
HYPRE_Int hypre_amd_ILUSmootherKernelTest(HYPRE_Int n, HYPRE_Real *scalars, HYPRE_Int first, HYPRE_Int zero_z, HYPRE_Int with_dots,
                                          HYPRE_Real *U, HYPRE_Real *R, HYPRE_Real *P, HYPRE_Real *Z, const HYPRE_Real *V)
{
   if (n < 1) { hypre_error_in_arg(1); return hypre_error_flag; }
   if (!scalars || !U || !R || !P || !Z || !V) { hypre_error_in_arg(2); return hypre_error_flag; }
   if (!ensure_device())
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ILUSmootherKernelTest: no HIP device is available");
      return hypre_error_flag;
   }
   hipStream_t s = stream();
   const size_t m = (size_t) n;
   const size_t ld = (m + 1) & ~(size_t) 1;          // every vector starts on 16 bytes, as the library's own do
   double *buf = hypre_TAlloc(double, 5 * ld + ILU_CG_SCALARS, HYPRE_MEMORY_DEVICE);
   double *dU = buf, *dR = buf + ld, *dP = buf + 2 * ld, *dZ = buf + 3 * ld, *dV = buf + 4 * ld, *sc = buf + 5 * ld;
   HYPRE_Real *host[4] = {U, R, P, Z};
   for (int k = 0; k < 4; k++) { hypre_TMemcpy(buf + (size_t) k * ld, host[k], double, m, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST); }
   hypre_TMemcpy(dV, V, double, m, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
   hypre_TMemcpy(sc, scalars, double, (size_t) ILU_CG_SCALARS, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
   if (with_dots) { launch_ilu_cg_dot(dR, dZ, m, sc, 0, s); }
   launch_ilu_cg_direction(sc, first != 0, dZ, dP, m, s);
   if (with_dots) { launch_ilu_cg_dot(dP, dV, m, sc, 1, s); }
   launch_ilu_cg_update(sc, dP, dV, dU, dR, zero_z ? dZ : nullptr, m, s);
   HIP_CHECK(hipStreamSynchronize(s));
   for (int k = 0; k < 4; k++) { hypre_TMemcpy(host[k], buf + (size_t) k * ld, double, m, HYPRE_MEMORY_HOST, HYPRE_MEMORY_DEVICE); }
   hypre_TMemcpy(scalars, sc, double, (size_t) ILU_CG_SCALARS, HYPRE_MEMORY_HOST, HYPRE_MEMORY_DEVICE);
   hypre_TFree(buf, HYPRE_MEMORY_DEVICE);
   return hypre_error_flag;
}

// The cycle from level `first` down and back up to it (0: the whole cycle).  first > 0 is the entry of the multi-column driver
// below: the levels above were cycled for all columns at once, F_array[first] holds the restricted residual of one column
// and, with first_presmoothed, U_array[first] the sweep from zero the restriction's epilogue wrote; the result is left in
// U_array[first].  The one-workgroup tail and the recorded graph start where they always do.
static HYPRE_Int amg_cycle_from(void *amg_vdata, hypre_ParVector **F_array, hypre_ParVector **U_array, int first, int first_presmoothed);
HYPRE_Int hypre_BoomerAMGCycle(void *amg_vdata, hypre_ParVector **F_array, hypre_ParVector **U_array)
{
   return amg_cycle_from(amg_vdata, F_array, U_array, 0, 0);
}
static HYPRE_Int amg_cycle_from(void *amg_vdata, hypre_ParVector **F_array, hypre_ParVector **U_array, int first, int first_presmoothed)
{
   hypre_ParAMGData *d = (hypre_ParAMGData *) amg_vdata;
   AmgPrivate *pv = (AmgPrivate *) d->amd_private;
   const int L = d->num_levels;
   hypre_ParCSRMatrix **A = d->A_array, **P = d->P_array;
   HYPRE_AMD_REQUIRE_DEVICE(A[0]->diag->memory_location, "hypre_BoomerAMGCycle(A)");
   HYPRE_AMD_REQUIRE_DEVICE(U_array[0]->local_vector->memory_location, "hypre_BoomerAMGCycle(u)");
   HYPRE_AMD_REQUIRE_DEVICE(F_array[0]->local_vector->memory_location, "hypre_BoomerAMGCycle(f)");
   hipStream_t s = stream();
   QuietSync quiet;
   const int saved_gs_threads = handle().gs_threads;
   handle().gs_threads = pv->emulated_threads;
   const bool saved_fp32 = handle().fp32_values;
   handle().fp32_values = pv->mixed_precision;

   // alternate solution buffers (allocated on the first cycle, reused afterwards)
   if ((int) pv->u_alt.size() != L) { pv->u_alt.assign((size_t) L, nullptr); pv->u_alt_len.assign((size_t) L, 0); }
   std::vector<LevelVec> lv((size_t) L);
   for (int l = 0; l < L; l++)
   {
      const int n = A[l]->diag->num_rows;
      if (pv->u_alt_len[(size_t) l] < n)
      {
         if (pv->u_alt[(size_t) l]) { hypre_Free(pv->u_alt[(size_t) l], HYPRE_MEMORY_DEVICE); }
         pv->u_alt[(size_t) l] = hypre_TAlloc(double, (size_t) std::max(n, 1), HYPRE_MEMORY_DEVICE);
         pv->u_alt_len[(size_t) l] = n;
      }
      lv[(size_t) l].home = U_array[l]->local_vector->data;
      lv[(size_t) l].alt = pv->u_alt[(size_t) l];
      lv[(size_t) l].cur = lv[(size_t) l].home;
   }
   std::vector<int> lev_counter((size_t) L, 0), zeros((size_t) L, 0);
   // presmoothed[l]: the restriction into level l also wrote the result of the level's first sweep from zero, u = (w f) ./ d
   std::vector<int> presmoothed((size_t) L, 0);
   zeros[(size_t) first] = U_array[first]->all_zeros;
   for (int k = 1; k < L; k++) { lev_counter[(size_t) k] = d->fcycle ? 1 : d->cycle_type; }
   lev_counter[(size_t) first] = 1;
   presmoothed[(size_t) first] = first_presmoothed;
   int fcycle_lev = L - 2, level = first, cycle_param = (first > 0 && first == L - 1) ? 3 : 1, err = 0;
   bool not_finished = true;
   double *vtemp = d->Vtemp->local_vector->data;
   double *ztemp = d->Ztemp->local_vector->data;
   const bool old_version = d->grid_relax_points != nullptr;
   double cycle_op_count = d->cycle_op_count;

   HYPRE_Int cycle_nprocs = 1;
   hypre_MPI_Comm_size(A[0]->comm, &cycle_nprocs);
   // ILU as a level smoother: on the levels below snl it replaces the relaxation, the coarsest level's direct solve included
   // (par_cycle.c:477 stands before :491); the one-workgroup tail, the recorded graph and the restriction's fused first
   // sweep start at a level >= snl or not at all
   const int snl = pv->ilu_smoothing() ? std::min<int>(pv->smooth_num_levels, (int) pv->ilu_smoothers.size()) : 0;
   pv->smoother_visits = pv->smoother_readbacks = 0;
   if (snl > 0 && (pv->mixed_precision || cycle_nprocs > 1))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGCycle: ILU smoothing (smooth_type 5 | 15) serves neither the mixed-precision hierarchy nor several ranks");
      handle().fp32_values = saved_fp32;
      handle().gs_threads = saved_gs_threads;
      return 1;
   }
   // ---- the smallest levels in one kernel of one workgroup (tail_kernels.hip): one rank, a plain V(1,1) cycle, Jacobi or
   // l1-Jacobi over all points with the smoother diagonals at hand, a direct solve on the coarsest level ----
   int st = -1;
   {
      const int t1 = d->grid_relax_type[1], t2 = d->grid_relax_type[2], t3 = d->grid_relax_type[3];
      const bool ok = small_tail_on() && pv->small_tail_nnz > 0 && cycle_nprocs == 1 && d->cycle_type == 1 && !d->fcycle && !old_version &&
                      L >= 3 && (t1 == 7 || t1 == 18 || t1 == 11 || t1 == 12) && (t2 == 7 || t2 == 18 || t2 == 11 || t2 == 12) &&
                      !(pv->replica && (t1 == 11 || t1 == 12 || t2 == 11 || t2 == 12)) && is_ge_type(t3) && d->relax_order == 0 &&
                      d->num_grid_sweeps[1] == 1 && d->num_grid_sweeps[2] == 1 && d->num_grid_sweeps[3] == 1 && !pv->tail;
      if (ok)
      {
         if (pv->small_tail_level == -2)
         {
            int first = L - 1;
            while (first - 1 >= 1 && A[first - 1]->diag->num_nonzeros <= pv->small_tail_nnz && L - (first - 1) <= SMALL_TAIL_MAX_LEVELS) { first--; }
            pv->small_tail_level = (first <= L - 2) ? first : -1;
         }
         st = pv->small_tail_level;
         if (st >= 0 && st < snl) { st = snl <= L - 2 ? snl : -1; }
         for (int l = st; st >= 0 && l < L; l++)
         {
            const bool last = l == L - 1;
            const bool here = A[l]->diag->memory_location == HYPRE_MEMORY_DEVICE && A[l]->offd->num_nonzeros == 0 &&
                              (last || (d->l1_norms[l] && d->l1_norms[l]->data && P[l] && P[l]->diagT &&
                                        P[l]->diagT->memory_location == HYPRE_MEMORY_DEVICE && P[l]->offd->num_nonzeros == 0));
            if (!here) { st = -1; }
         }
         if (st >= 0)
         {
            if (!d->gs_setup) { hypre_GaussElimSetup(d, L - 1, t3); }
            ensure_coarse_factors(d);
            if (pv->coarse_n != A[L - 1]->diag->num_rows || pv->coarse_n > SMALL_TAIL_MAX_COARSE || pv->coarse_n < 1) { st = -1; }
         }
         // the levels' arrays as the kernel holds them in LDS; a tail that does not fit starts a level further down
         auto image_of = [&](int lvl)
         {
            // (the form that worked last time first: with an unchanged hierarchy that is a comparison of two numbers)
            const int forced = small_tail_forced_form();
            if (forced >= 0) { pv->tail_outside = forced; return build_small_tail_image(d, pv, lvl, s, forced); }
            if (pv->tail_outside >= 0 && build_small_tail_image(d, pv, lvl, s, pv->tail_outside)) { return true; }
            for (int form = 0; form < 3; form++)
            {
               if (build_small_tail_image(d, pv, lvl, s, form)) { pv->tail_outside = form; return true; }
            }
            pv->tail_outside = -1;
            return false;
         };
         while (st >= 0 && !image_of(st))
         {
            st = (st + 1 <= L - 2) ? st + 1 : -1;
            pv->small_tail_level = st;
         }
      }
   }
   pv->small_tail_used = st;
   // ---- coarse tail as a HIP graph (single rank, plain V-cycle, smoothers whose launches do not depend on host state
   // that changes from cycle to cycle) ----
   int gl = -1;
   {
      auto graphable = [&](int t) { return is_jacobi_type(t) || is_ge_type(t) || t == 11 || t == 12 || t == 16 || t == 21 || t == 22; };
      static const int graph_env = [] { const char *e = getenv("HYPRE_AMD_CYCLE_GRAPH"); return e ? atoi(e) : 1; }();
      const bool ok = graph_env && pv->graph_rows > 0 && cycle_nprocs == 1 && d->cycle_type == 1 && !d->fcycle && !old_version &&
                      L >= 3 && graphable(d->grid_relax_type[1]) && graphable(d->grid_relax_type[2]) && graphable(d->grid_relax_type[3]);
      if (ok)
      {
         if (pv->graph_level < 0)
         {
            for (int l = std::max(1, snl); l < L - 1; l++) { if (A[l]->global_num_rows <= (HYPRE_BigInt) pv->graph_rows) { pv->graph_level = l; break; } }
         }
         gl = pv->graph_level;
         if (gl >= 0 && gl < snl) { gl = pv->graph_level = snl; }
         if (gl >= L - 1) { gl = -1; }
      }
      if (gl < 0 && pv->graph_state) { pv->drop_graph(); }
      if (gl >= 0)
      {
         const unsigned long long sig = tail_signature(d, pv, gl, F_array, U_array);
         if (pv->graph_state && sig != pv->graph_sig) { pv->drop_graph(); }
         pv->graph_sig = sig;
      }
   }
   bool arrived_down = first > 0, capturing = false;
   double op_count_at_capture = 0.0, csr_at_capture = 0.0, stream_at_capture = 0.0;

   while (not_finished)
   {
      const int n = A[level]->diag->num_rows;
      hypre_amd_CommSetTag(level);             // (diagnosis: exchanges from here on belong to this level)
      // the tail: replay, or record on the second visit
      bool replayed = false;
      if (gl >= 0 && level == gl && arrived_down)
      {
         if (pv->graph_state == 2)
         {
            HIP_CHECK(hipGraphLaunch(pv->graph_exec, s));
            for (int l = gl; l < L; l++) { lv[(size_t) l].cur = pv->graph_cur[(size_t) (l - gl)]; zeros[(size_t) l] = 0; lev_counter[(size_t) l] = -1; }
            cycle_op_count += pv->graph_op_count;
            account_bytes(pv->graph_bytes_csr, pv->graph_bytes_stream);      // what the recorded launches accounted for
            replayed = true;
         }
         else if (pv->graph_state == 1)
         {
            if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) { capturing = true; op_count_at_capture = cycle_op_count; csr_at_capture = handle().bytes_csr; stream_at_capture = handle().bytes_stream; }
            else { (void) hipGetLastError(); pv->graph_state = 0; gl = -1; }
         }
      }
      if (st >= 0 && level == st && arrived_down && !replayed)
      {
         // everything from here down and back up to this level's post-smoothing sweep: one launch
         SmallTailArgs ta = pv->tail_args;
         double csr_bytes = 0.0;
         for (int l = st; l < L; l++)
         {
            ta.lv[l - st].w = d->relax_weight[l];
            if (l < L - 1)
            {
               cycle_op_count += 2.0 * A[l]->d_num_nonzeros;
               csr_bytes += 2.0 * (12.0 * A[l]->diag->num_nonzeros + 36.0 * A[l]->diag->num_rows) +
                            2.0 * (12.0 * P[l]->diag->num_nonzeros + 20.0 * P[l]->diag->num_rows);
            }
            else { cycle_op_count += A[l]->d_num_nonzeros; }
         }
         ta.f_in = F_array[st]->local_vector->data;
         ta.u_io = lv[(size_t) st].home;
         {
            const int t1 = d->grid_relax_type[1], t2 = d->grid_relax_type[2];
            ta.kind_down = (t1 == 11 || t1 == 12) ? 1 : 0; ta.inner_down = t1 == 12 ? 2 : 1;
            ta.kind_up = (t2 == 11 || t2 == 12) ? 1 : 0; ta.inner_up = t2 == 12 ? 2 : 1;
         }
         ta.first_presmoothed = presmoothed[(size_t) st];
         presmoothed[(size_t) st] = 0;
         ta.round32 = handle().fp32_values ? 1 : 0;
         account_bytes(csr_bytes);
         launch_small_tail(ta, s);
         for (int l = st; l < L; l++) { lv[(size_t) l].cur = lv[(size_t) l].home; zeros[(size_t) l] = 0; lev_counter[(size_t) l] = -1; }
         replayed = true;
      }
      arrived_down = false;
      int num_sweep, relax_type;
      if (L > 1) { num_sweep = d->num_grid_sweeps[cycle_param]; relax_type = d->grid_relax_type[cycle_param]; }
      else
      {
         num_sweep = d->num_grid_sweeps[0];
         relax_type = d->user_relax_type;
         if (relax_type == -1) { relax_type = 6; }
      }
      const int *cf = d->CF_marker_array[level] ? d->CF_marker_array[level]->data : nullptr;
      const double *l1 = d->l1_norms[level] ? d->l1_norms[level]->data : nullptr;
      const double *fd = F_array[level]->local_vector->data;
      LevelVec &u = lv[(size_t) level];
      const double w = d->relax_weight[level];

      // replicated tail: from this level down the V-cycle runs on this rank's own copy of the operators
      // (one all-reduce of the right-hand side instead of four halo exchanges per level)
      const bool tail_here = pv->tail != nullptr && level == pv->tail_level;
      if (tail_here)
      {
         err = run_replicated_tail(d, pv, fd, u.home, &cycle_op_count);
         u.cur = u.home;
         zeros[(size_t) level] = 0;
         if (err) { break; }
      }
      // ---- ILU as the level's smoother (par_cycle.c:293-326, 388-393, 477-483, 614-636) ----
      const bool smooth_here = level < snl && !tail_here && !replayed;
      if (smooth_here)
      {
         const long readbacks_before = reduction_readbacks();
         pv->smoother_visits++;
         HYPRE_Solver sm = pv->ilu_smoothers[(size_t) level];
         const double level_ops = A[level]->d_num_nonzeros;
         hypre_Vector uv; hypre_ParVector up;
         wrap(&uv, u.cur, n);
         wrap_par(&up, &uv, A[level]->comm, A[level]->global_num_rows);
         up.all_zeros = zeros[(size_t) level];
         if (pv->smooth_type == 5 || L == 1)
         {
            // smooth_num_sweeps applications on (F, U); a hierarchy of one level takes num_grid_sweeps[0] of them, with
            // either type (the reference's acceleration there works on vectors it never filled)
            const int sweeps = L > 1 ? pv->smooth_num_sweeps : num_sweep;
            for (int j = 0; j < sweeps && !err; j++)
            {
               cycle_op_count += level_ops;
               ilu_solve_core(sm, A[level], F_array[level], &up, false);
               if (hypre_error_flag) { err = 1; }
            }
         }
         else if (!d->Rtemp || !d->Ptemp)
         {
            hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGCycle: smooth_type 15 on a hierarchy the setup did not prepare for it");
            err = 1;
         }
         else
         {
            // conjugate gradients on A with num_sweep ILU applications from zero as the preconditioner, smooth_num_sweeps steps
            hypre_ParVectorSetLocalSize(d->Vtemp, n); hypre_ParVectorSetLocalSize(d->Ztemp, n);
            hypre_ParVectorSetLocalSize(d->Rtemp, n); hypre_ParVectorSetLocalSize(d->Ptemp, n);
            double *R = d->Rtemp->local_vector->data, *Pd = d->Ptemp->local_vector->data, *Z = d->Ztemp->local_vector->data, *V = vtemp;
            const int cg_sweeps = pv->smooth_num_sweeps;
            const bool fused = smoother_fusion() != 0;
            if (!pv->d_cg_scalars) { pv->d_cg_scalars = hypre_TAlloc(double, ILU_CG_SCALARS, HYPRE_MEMORY_DEVICE); }
            double *sc = pv->d_cg_scalars;
            if (zeros[(size_t) level]) { launch_copy(R, fd, (size_t) n, s); }        // F - A 0
            else { dev_par_matvec(-1.0, A[level], u.cur, 1.0, fd, R); }
            if (fused) { launch_set(sc, 0.0, (size_t) ILU_CG_SCALARS, s); }
            launch_set(Z, 0.0, (size_t) n, s);
            double gamma = 0.0, gammaold = 0.0;
            for (int jj = 0; jj < cg_sweeps && !err; jj++)
            {
               // Z = 0: by the set above, then by the update kernel of the sweep before (fused) or by a set of its own
               if (jj > 0 && !fused) { hypre_ParVectorSetConstantValues(d->Ztemp, 0.0); }
               d->Ztemp->all_zeros = 1;
               for (int j = 0; j < num_sweep && !err; j++)
               {
                  cycle_op_count += level_ops;
                  ilu_solve_core(sm, A[level], d->Rtemp, d->Ztemp, false);
                  if (hypre_error_flag) { err = 1; }
               }
               if (err) { break; }
               if (fused)
               {
                  launch_ilu_cg_dot(R, Z, (size_t) n, sc, 0, s);
                  launch_ilu_cg_direction(sc, jj == 0, Z, Pd, (size_t) n, s);
                  dev_par_matvec(1.0, A[level], Pd, 0.0, nullptr, V);
                  launch_ilu_cg_dot(Pd, V, (size_t) n, sc, 1, s);
                  launch_ilu_cg_update(sc, Pd, V, u.cur, R, jj + 1 < cg_sweeps ? Z : nullptr, (size_t) n, s);
               }
               else
               {
                  gammaold = gamma;
                  gamma = hypre_ParVectorInnerProd(d->Rtemp, d->Ztemp);
                  if (gamma == 0.0) { break; }       // a zero right-hand side: U stays (the reference divides 0 by 0)
                  if (jj == 0) { hypre_ParVectorCopy(d->Ztemp, d->Ptemp); }
                  else { launch_ilu_cg_direction_value(gamma / gammaold, Z, Pd, (size_t) n, s); }
                  dev_par_matvec(1.0, A[level], Pd, 0.0, nullptr, V);
                  const double alfa = gamma / hypre_ParVectorInnerProd(d->Ptemp, d->Vtemp);
                  hypre_ParVectorAxpy(alfa, d->Ptemp, &up);
                  hypre_ParVectorAxpy(-alfa, d->Vtemp, d->Rtemp);
               }
            }
            d->Ztemp->all_zeros = 0;
         }
         zeros[(size_t) level] = 0;
         pv->smoother_readbacks += (int) (reduction_readbacks() - readbacks_before);
         if (err) { break; }
      }
      for (int j = 0; j < ((tail_here || replayed || smooth_here) ? 0 : num_sweep); j++)
      {
         int relax_points = 0, relax_local = d->relax_order;
         if (L == 1 && d->max_levels > 1) { relax_points = 0; relax_local = 0; }
         else if (old_version) { relax_points = d->grid_relax_points[cycle_param][j]; }
         // par_cycle.c:413-430: the reference's ("VERY sloppy") operation count behind the printed cycle complexity
         if (old_version && level < L - 1)
         {
            if (relax_points == 1) { cycle_op_count += A[level + 1]->d_num_nonzeros; }
            else if (relax_points == -1) { cycle_op_count += A[level]->d_num_nonzeros - A[level + 1]->d_num_nonzeros; }
         }
         else { cycle_op_count += A[level]->d_num_nonzeros; }
         if (is_ge_type(relax_type))
         {
            // the dense solve reads F[level] and writes the home vector
            hypre_GaussElimSolve(d, level, relax_type);
            u.cur = u.home;
            zeros[(size_t) level] = 0;
         }
         else if (is_jacobi_type(relax_type))
         {
            // point sets of this sweep: all points, or C then F / F then C
            int pts[2] = {relax_points, 0}, npass = 1;
            if (!old_version && relax_local == 1 && cycle_param < 3)
            {
               npass = 2;
               pts[0] = cycle_param < 2 ? 1 : -1; pts[1] = -pts[0];
            }
            const double *dg = l1;
            if (relax_type == 0 || !dg)
            {
               double *dd = pv->level_diag(level, n);
               launch_diag_first(A[level]->diag->i, A[level]->diag->data, dd, n, s);
               dg = dd;
            }
            for (int pss = 0; pss < npass; pss++)
            {
               if (zeros[(size_t) level] && relax_type != 0)
               {
                  if (presmoothed[(size_t) level]) { presmoothed[(size_t) level] = 0; }       // the restriction's epilogue did it
                  else { launch_scaled_div(w, fd, dg, u.cur, pts[pss] ? cf : nullptr, pts[pss], (size_t) n, s); }
               }
               else
               {
                  dev_jacobi_sweep(A[level], fd, cf, pts[pss], w, dg, u.cur, u.other());
                  u.flip();
               }
               zeros[(size_t) level] = 0;
            }
         }
         else if (relax_type == 15)
         {
            // CG smoother (par_cycle.c:517-528, par_relax_more.c:464-493, setup par_amg_setup.c:3551-3567): num_sweep
            // iterations of unpreconditioned CG from the current iterate, once per relaxation call
            if (j == 0)
            {
               if (pv->cg_smoothers.size() < (size_t) L) { pv->cg_smoothers.resize((size_t) L, nullptr); }
               hypre_Vector uv; hypre_ParVector up;
               wrap(&uv, u.cur, n);
               wrap_par(&up, &uv, A[level]->comm, A[level]->global_num_rows);
               up.all_zeros = zeros[(size_t) level];
               HYPRE_Solver &cg = pv->cg_smoothers[(size_t) level];
               if (!cg)
               {
                  HYPRE_ParCSRPCGCreate(A[level]->comm, &cg);
                  HYPRE_PCGSetTwoNorm(cg, 1);
                  HYPRE_ParCSRPCGSetup(cg, A[level], F_array[level], &up);
               }
               HYPRE_PCGSetMaxIter(cg, num_sweep);
               HYPRE_PCGSetTol(cg, 0.0);
               HYPRE_ParCSRPCGSolve(cg, A[level], F_array[level], &up);
               zeros[(size_t) level] = 0;
            }
         }
         else if (relax_type == 17)
         {
            // FCF-Jacobi (par_cycle.c:539-556, par_relax_interface.c:83-117): weighted Jacobi on the F, the C and again
            // the F points; one plain Jacobi sweep on the coarsest level, which has no C/F splitting
            static const int fcf[3] = {-1, 1, -1};
            const int npass = (level == L - 1) ? 1 : 3;
            double *dd = pv->level_diag(level, n);
            launch_diag_first(A[level]->diag->i, A[level]->diag->data, dd, n, s);
            for (int pss = 0; pss < npass; pss++)
            {
               dev_jacobi_sweep(A[level], fd, cf, npass == 1 ? 0 : fcf[pss], w, dd, u.cur, u.other());
               u.flip();
            }
            zeros[(size_t) level] = 0;
         }
         else if (relax_type == 16)
         {
            // Chebyshev polynomial smoothing (par_cycle.c:529-537), in place on the current buffer
            if (!d->cheby_coefs || !d->cheby_coefs[level] || !d->Ptemp || !d->Rtemp)
            {
               hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGCycle: relax 16 on a level the setup did not prepare for it");
               err = 1;
            }
            else
            {
               hypre_Vector uv; hypre_ParVector up;
               wrap(&uv, u.cur, n);
               wrap_par(&up, &uv, A[level]->comm, A[level]->global_num_rows);
               up.all_zeros = zeros[(size_t) level];
               hypre_ParVectorSetLocalSize(d->Vtemp, n);
               hypre_ParVectorSetLocalSize(d->Ztemp, n);
               hypre_ParVectorSetLocalSize(d->Ptemp, n);
               hypre_ParVectorSetLocalSize(d->Rtemp, n);
               hypre_ParCSRRelax_Cheby_Solve(A[level], F_array[level],
                                             d->cheby_ds && d->cheby_ds[level] ? d->cheby_ds[level]->data : nullptr,
                                             d->cheby_coefs[level], d->cheby_order, d->cheby_scale, d->cheby_variant,
                                             &up, d->Vtemp, d->Ztemp, d->Ptemp, d->Rtemp);
               zeros[(size_t) level] = 0;
               if (hypre_error_flag) { err = 1; }
            }
         }
         else
         {
            // in-place smoothers go through the public entry on a view of the current buffer
            hypre_Vector uv; hypre_ParVector up;
            wrap(&uv, u.cur, n);
            wrap_par(&up, &uv, A[level]->comm, A[level]->global_num_rows);
            up.all_zeros = zeros[(size_t) level];
            hypre_ParVectorSetLocalSize(d->Vtemp, n);
            hypre_ParVectorSetLocalSize(d->Ztemp, n);
            if (old_version) { err = hypre_BoomerAMGRelax(A[level], F_array[level], (HYPRE_Int *) cf, relax_type, relax_points, w, d->omega[level], (HYPRE_Real *) l1, &up, d->Vtemp, d->Ztemp); }
            else { err = hypre_BoomerAMGRelaxIF(A[level], F_array[level], (HYPRE_Int *) cf, relax_type, relax_local, cycle_param, w, d->omega[level], (HYPRE_Real *) l1, &up, d->Vtemp, d->Ztemp); }
            zeros[(size_t) level] = 0;
            if (hypre_error_flag) { err = 1; }
         }
         if (err) { break; }
      }
      if (err) { break; }

      if (!replayed) { --lev_counter[(size_t) level]; }
      if (!replayed && lev_counter[(size_t) level] >= 0 && level != L - 1 && !tail_here)
      {
         arrived_down = true;
         // descend: u_c = 0 ; r = f - A u ; f_c = P^T r
         const int fine = level, coarse = level + 1;
         LevelVec &uc = lv[(size_t) coarse];
         uc.cur = uc.home;
         const int nc = A[coarse]->diag->num_rows;
         // the zero-guess sweep on the coarse level overwrites every row it
         // relaxes; rows it skips (CF passes, zero diagonals never occur) must
         // read as zero, so the vector is cleared unless the first coarse
         // operation is known to overwrite all of it
         const int ctype = d->grid_relax_type[coarse == L - 1 ? 3 : 1];
         // (an ILU level smoother adds its correction to the iterate: the zeros have to be there)
         const bool overwrites_all = coarse >= snl &&
                                     ((is_jacobi_type(ctype) && ctype != 0 && !(d->relax_order == 1 && coarse != L - 1) &&
                                       !old_version && d->num_grid_sweeps[coarse == L - 1 ? 3 : 1] > 0) || is_ge_type(ctype));
         if (!overwrites_all) { launch_set(uc.cur, 0.0, (size_t) nc, s); }
         zeros[(size_t) coarse] = 1;
         dev_par_matvec(-1.0, A[fine], u.cur, 1.0, fd, vtemp);
         // One rank, the coarse level starts with a Jacobi-type sweep from zero over all its points (u_c = w f_c ./ d_c, its
         // smoother diagonal at hand): the restriction's epilogue writes that as well — f_c is in its registers — instead of a
         // kernel of its own reading f_c and d_c again (one launch and 8 bytes per coarse row less on every level below the
         // finest; same bits: (w f) / d either way).  Several ranks add the neighbours' contributions to f_c afterwards: not there.
         const int fuse_on = cycle_fusion();
         presmoothed[(size_t) coarse] = 0;
         bool restricted = false;
         if (fuse_on && cycle_nprocs == 1 && overwrites_all && is_jacobi_type(ctype) && d->l1_norms[coarse] && d->l1_norms[coarse]->data &&
             P[fine]->diagT && P[fine]->diagT->memory_location == HYPRE_MEMORY_DEVICE && P[fine]->offd->num_cols == 0)
         {
            restricted = spmv_with_scaled_quotient(P[fine]->diagT, vtemp, F_array[coarse]->local_vector->data, d->relax_weight[coarse],
                                                   d->l1_norms[coarse]->data, uc.cur);
            if (restricted) { presmoothed[(size_t) coarse] = 1; F_array[coarse]->all_zeros = 0; }
         }
         if (!restricted) { dev_par_matvecT(1.0, P[fine], vtemp, 0.0, F_array[coarse]->local_vector->data); }
         ++level;
         lev_counter[(size_t) level] = std::max(lev_counter[(size_t) level], (int) d->cycle_type);
         cycle_param = (level == L - 1) ? 3 : 1;
      }
      else if (level != first || (capturing && level == gl))
      {
         if (capturing && level == gl)
         {
            // the sub-cycle is over: everything enqueued since the tail was entered becomes the graph
            capturing = false;
            hipGraph_t g = nullptr;
            if (hipStreamEndCapture(s, &g) == hipSuccess && g)
            {
               hipGraphExec_t ex = nullptr;
               if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess)
               {
                  pv->graph = g; pv->graph_exec = ex; pv->graph_state = 2;
                  pv->graph_cur.assign((size_t) (L - gl), nullptr);
                  for (int l = gl; l < L; l++) { pv->graph_cur[(size_t) (l - gl)] = lv[(size_t) l].cur; }
                  pv->graph_op_count = cycle_op_count - op_count_at_capture;
                  pv->graph_bytes_csr = handle().bytes_csr - csr_at_capture;
                  pv->graph_bytes_stream = handle().bytes_stream - stream_at_capture;
                  size_t nn = 0;
                  if (hipGraphGetNodes(g, nullptr, &nn) == hipSuccess) { pv->graph_launches = (int) nn; }
                  HIP_CHECK(hipGraphLaunch(ex, s));       // the capture recorded the work, it did not run it
               }
               else { (void) hipGetLastError(); (void) hipGraphDestroy(g); pv->graph_state = 0; err = 1; hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGCycle: the coarse-tail graph could not be instantiated"); }
            }
            else { (void) hipGetLastError(); pv->graph_state = 0; err = 1; hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGCycle: capturing the coarse tail failed"); }
            if (err) { break; }
         }
         if (level == first) { not_finished = false; continue; }      // (entered at the tail's first level: nothing above it here)
         // ascend: u_f += P u_c, written to whichever buffer lets the
         // post-smoothing sweeps end in the level's home vector
         const int fine = level - 1;
         LevelVec &uf = lv[(size_t) fine];
         int flips = 0;
         {
            const int t = d->grid_relax_type[2];
            if (is_jacobi_type(t) && fine >= snl)        // (an ILU level smoother works in place)
            {
               const int passes = (!old_version && d->relax_order == 1) ? 2 : 1;
               flips = d->num_grid_sweeps[2] * passes;
            }
         }
         double *target = (flips % 2 == 0) ? uf.home : uf.alt;
         dev_par_matvec(1.0, P[fine], u.cur, 1.0, uf.cur, target);
         uf.cur = target;
         zeros[(size_t) fine] = 0;
         --level;
         cycle_param = 2;
         if (d->fcycle && fcycle_lev == level)
         {
            lev_counter[(size_t) level] = std::max(lev_counter[(size_t) level], 1);
            fcycle_lev--;
         }
      }
      else
      {
         not_finished = false;
      }
   }
   if (capturing)
   {
      // left the loop (an error) while recording: close the capture so that the stream is usable again
      hipGraph_t g = nullptr;
      (void) hipStreamEndCapture(s, &g);
      if (g) { (void) hipGraphDestroy(g); }
      (void) hipGetLastError();
      pv->graph_state = 0;
   }
   else if (gl >= 0 && pv->graph_state == 0 && !err) { pv->graph_state = 1; }      // warmed up: record at the next cycle
   // the caller's vector must hold the result
   if (lv[(size_t) first].cur != lv[(size_t) first].home)
   {
      launch_copy(lv[(size_t) first].home, lv[(size_t) first].cur, (size_t) A[first]->diag->num_rows, s);
   }
   U_array[first]->all_zeros = 0;
   d->cycle_op_count = cycle_op_count;
   (void) ztemp;
   handle().fp32_values = saved_fp32;
   hypre_amd_CommSetTag(-1);
   handle().gs_threads = saved_gs_threads;
   quiet.restore();
   maybe_sync();
   return err;
}

// ===========================================================================
// several right-hand sides: f and u with num_vectors > 1 (par_amg_solve.c:107-133)
// ===========================================================================
// Why a solve of several columns is refused with the solver's options, or "" when it is served: Jacobi-type sweeps 7 / 18
// and two-stage Gauss-Seidel 11 / 12 over all points, a direct solve on the coarsest level.  The reference refuses hybrid
// Gauss-Seidel, Jacobi 0 and Chebyshev with multicomponent vectors (par_relax.c:219-224, 751-756; par_cheby.c:423); the
// other smoothers, C/F-ordered sweeps, grid_relax_points and mixed precision have no multicomponent path.
static std::string multivector_refusal(const hypre_ParAMGData *d)
{
   const AmgPrivate *pv = (const AmgPrivate *) d->amd_private;
   if (pv && pv->ilu_smoothing()) { return "ILU smoothing doesn't support multicomponent vectors"; }
   if (pv && pv->mixed_precision) { return "hypre_BoomerAMGSolve: mixed precision doesn't support multicomponent vectors"; }
   if (d->grid_relax_points) { return "hypre_BoomerAMGSolve: grid_relax_points don't support multicomponent vectors"; }
   if (d->relax_order != 0) { return "hypre_BoomerAMGSolve: C/F-ordered relaxation doesn't support multicomponent vectors"; }
   // the smoothers the cycle takes (par_cycle.c: down, up, coarsest; the user's type on a one-level hierarchy)
   std::vector<int> types;
   if (d->num_levels > 1) { types = {d->grid_relax_type[1], d->grid_relax_type[2], d->grid_relax_type[3]}; }
   else { types = {d->user_relax_type == -1 ? 6 : d->user_relax_type}; }
   for (size_t k = 0; k < types.size(); k++)
   {
      const int t = types[k];
      const bool coarsest = k == 2 || d->num_levels == 1;
      if (t == 7 || t == 18 || t == 11 || t == 12 || (coarsest && is_ge_type(t))) { continue; }
      if (t == 3 || t == 4 || t == 6 || t == 8 || t == 13 || t == 14 || t == 88 || t == 89)
      {
         return "Hybrid GS relaxation doesn't support multicomponent vectors";
      }
      if (t == 0) { return "Jacobi relaxation doesn't support multicomponent vectors"; }
      return "Requested relaxation type " + std::to_string(t) + " doesn't support multicomponent vectors";
   }
   return "";
}

// ---------------------------------------------------------------------------
// The V-cycle over NV columns with the large matrix passes fused: on levels 0 .. K - 1 every pass over an operator — the
// sweep, the residual, the restriction (with the epilogue that writes the coarse level's sweep from zero), the prolongation,
// the post-sweep — is one launch for a group of 2 - 4 columns (launch_spmv_mv: the multivector form of the kernel the
// single-vector pass takes, so every column keeps the single-vector cycle's bits); from level K down and back up to it each
// column runs the single-column cycle (amg_cycle_from) on the solver's own level vectors: the one-workgroup tail, the
// recorded graph and the dense solve see what they always see.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
int &multivector_cycle()
{
   // (off until the fused cycle has been timed against the column loop on a device: DESIGN.md section 4)
   static int on = [] { const char *e = getenv("HYPRE_AMD_MULTIVECTOR_CYCLE"); return e ? (atoi(e) != 0 ? 1 : 0) : 0; }();
   return on;
}
constexpr int MV_CYCLE_MIN_ROWS = 64;     // levels below this many rows are left to the single-column cycle: nothing to share

// first level of the single-column part, or -1: this solver's cycle is not served (the column loop takes it)
int multivector_cycle_first(const hypre_ParAMGData *d, const AmgPrivate *pv)
{
   const int L = d->num_levels;
   if (L < 2 || d->cycle_type != 1 || d->fcycle || d->grid_relax_points || d->relax_order != 0 || pv->tail || pv->mixed_precision) { return -1; }
   HYPRE_Int np = 1;
   hypre_MPI_Comm_size(d->A_array[0]->comm, &np);
   if (np != 1) { return -1; }
   const int t1 = d->grid_relax_type[1], t2 = d->grid_relax_type[2], t3 = d->grid_relax_type[3];
   if (!(t1 == 7 || t1 == 18) || !(t2 == 7 || t2 == 18) || !is_ge_type(t3)) { return -1; }
   if (d->num_grid_sweeps[1] < 1 || d->num_grid_sweeps[2] < 1 || d->num_grid_sweeps[1] > 4 || d->num_grid_sweeps[2] > 4) { return -1; }
   int K = L - 1;
   for (int l = 1; l < L - 1; l++)
   {
      const hypre_CSRMatrix *Al = d->A_array[l]->diag;
      if (Al->num_rows < MV_CYCLE_MIN_ROWS || (small_tail_on() && pv->small_tail_nnz > 0 && Al->num_nonzeros <= pv->small_tail_nnz) ||
          (pv->graph_rows > 0 && d->A_array[l]->global_num_rows <= (HYPRE_BigInt) pv->graph_rows)) { K = l; break; }
   }
   // never below where the tail kernel or the recorded graph was found to begin
   if (pv->small_tail_level >= 1) { K = std::min(K, pv->small_tail_level); }
   if (pv->graph_rows > 0 && pv->graph_level >= 1) { K = std::min(K, pv->graph_level); }
   for (int l = 0; l < K; l++)
   {
      const hypre_ParCSRMatrix *Al = d->A_array[l], *Pl = d->P_array[l];
      if (Al->diag->memory_location != HYPRE_MEMORY_DEVICE || Al->offd->num_nonzeros != 0 || Al->offd->num_cols != 0) { return -1; }
      if (!Pl || !Pl->diagT || Pl->diagT->memory_location != HYPRE_MEMORY_DEVICE || Pl->diag->memory_location != HYPRE_MEMORY_DEVICE ||
          Pl->offd->num_cols != 0) { return -1; }
   }
   return K;
}

bool ensure_mv_levels(hypre_ParAMGData *d, AmgPrivate *pv, int nv, int K)
{
   bool fits = pv->mv_first == K && pv->mv_cols >= nv && (int) pv->mv_lev.size() == K + 1;
   for (int l = 0; fits && l <= K; l++) { fits = pv->mv_lev[(size_t) l].n == d->A_array[l]->diag->num_rows; }
   if (fits) { return true; }
   HIP_CHECK(hipStreamSynchronize(stream()));
   pv->release_mv_levels();
   pv->mv_lev.resize((size_t) K + 1);
   size_t widest = 0;
   bool ok = true;
   for (int l = 0; ok && l <= K; l++)
   {
      AmgPrivate::MvLevel &m = pv->mv_lev[(size_t) l];
      m.n = d->A_array[l]->diag->num_rows;
      m.stride = ((size_t) m.n + 1) & ~(size_t) 1;
      const size_t bytes = sizeof(double) * ((size_t) nv * m.stride + 8);
      if (l < K) { widest = std::max(widest, m.stride); }
      if (l > 0) { ok = ok && plan_alloc((void **) &m.f, bytes, PLAN_SITE_MV_LEVELS) && plan_alloc((void **) &m.home, bytes, PLAN_SITE_MV_LEVELS); }
      if (l < K) { ok = ok && plan_alloc((void **) &m.alt, bytes, PLAN_SITE_MV_LEVELS); }
   }
   ok = ok && plan_alloc((void **) &pv->mv_vtemp, sizeof(double) * ((size_t) nv * widest + 8), PLAN_SITE_MV_LEVELS);
   if (!ok) { pv->release_mv_levels(); return false; }
   pv->mv_cols = nv; pv->mv_first = K;
   return true;
}

// one cycle of all columns; f and u: the caller's columns, n doubles apart
HYPRE_Int amg_cycle_columns(hypre_ParAMGData *d, AmgPrivate *pv, const double *f, double *u, int n, int nv, int K, int u_zero)
{
   struct Lv
   {
      double *home, *alt, *cur; size_t hs, as;
      size_t cs() const { return cur == home ? hs : as; }
      double *other() const { return cur == home ? alt : home; }
      size_t os() const { return cur == home ? as : hs; }
      void flip() { cur = other(); }
   };
   hipStream_t s = stream();
   hypre_ParCSRMatrix **A = d->A_array, **P = d->P_array;
   const int L = d->num_levels;
   const bool saved_fp32 = handle().fp32_values;
   handle().fp32_values = false;
   std::vector<Lv> lv((size_t) K + 1);
   std::vector<const double *> F((size_t) K + 1);
   std::vector<size_t> fs((size_t) K + 1);
   for (int l = 0; l <= K; l++)
   {
      const AmgPrivate::MvLevel &m = pv->mv_lev[(size_t) l];
      lv[(size_t) l] = Lv{l == 0 ? u : m.home, m.alt, l == 0 ? u : m.home, l == 0 ? (size_t) n : m.stride, m.stride};
      F[(size_t) l] = l == 0 ? f : m.f;
      fs[(size_t) l] = l == 0 ? (size_t) n : m.stride;
   }
   auto diag_of = [&](int l, int relax_type) -> const double *
   {
      const double *dg = d->l1_norms[l] ? d->l1_norms[l]->data : nullptr;
      if (relax_type == 0 || !dg)
      {
         double *dd = pv->level_diag(l, A[l]->diag->num_rows);
         launch_diag_first(A[l]->diag->i, A[l]->diag->data, dd, A[l]->diag->num_rows, s);
         dg = dd;
      }
      return dg;
   };
   double op_count = 0.0;
   std::vector<int> presmoothed((size_t) K + 1, 0);
   double *vtemp = pv->mv_vtemp;
   // ---- down
   for (int l = 0; l < K; l++)
   {
      const int nl = A[l]->diag->num_rows, coarse = l + 1;
      Lv &ul = lv[(size_t) l];
      const double w = d->relax_weight[l];
      const double *dg = diag_of(l, d->grid_relax_type[1]);
      bool zero = l == 0 ? u_zero != 0 : true;
      for (int j = 0; j < d->num_grid_sweeps[1]; j++)
      {
         op_count += A[l]->d_num_nonzeros;
         if (zero)
         {
            if (presmoothed[(size_t) l]) { presmoothed[(size_t) l] = 0; }      // the restriction's epilogue did it
            else
            {
               for (int v = 0; v < nv; v++) { launch_scaled_div(w, F[(size_t) l] + (size_t) v * fs[(size_t) l], dg, ul.cur + (size_t) v * ul.cs(), nullptr, 0, (size_t) nl, s); }
            }
         }
         else
         {
            spmv_columns_jacobi(A[l]->diag, F[(size_t) l], fs[(size_t) l], w, dg, ul.cur, ul.cs(), ul.other(), ul.os(), nv);
            ul.flip();
         }
         zero = false;
      }
      // r = f - A u ; f_c = P^T r (and u_c = w f_c ./ d_c where the single-column cycle fuses it)
      Lv &uc = lv[(size_t) coarse];
      uc.cur = uc.home;
      const size_t vs = pv->mv_lev[(size_t) l].stride;
      spmv_columns(-1.0, A[l]->diag, ul.cur, ul.cs(), 1.0, F[(size_t) l], fs[(size_t) l], vtemp, vs, nv);
      double *fc = pv->mv_lev[(size_t) coarse].f;
      const size_t fcs = pv->mv_lev[(size_t) coarse].stride;
      bool restricted = false;
      if (cycle_fusion() && coarse != L - 1 && d->l1_norms[coarse] && d->l1_norms[coarse]->data)
      {
         restricted = spmv_columns_scaled_quotient(P[l]->diagT, vtemp, vs, fc, fcs, d->relax_weight[coarse], d->l1_norms[coarse]->data,
                                                   uc.cur, uc.hs, nv);
         presmoothed[(size_t) coarse] = restricted ? 1 : 0;
      }
      if (!restricted) { spmv_columns(1.0, P[l]->diagT, vtemp, vs, 0.0, fc, fcs, fc, fcs, nv); }
   }
   // ---- level K and below: column by column on the solver's single-column level vectors
   HYPRE_Int err = 0;
   double tail_count = 0.0;
   {
      const int nK = A[K]->diag->num_rows;
      const AmgPrivate::MvLevel &m = pv->mv_lev[(size_t) K];
      double *fK = d->F_array[K]->local_vector->data, *uK = d->U_array[K]->local_vector->data;
      for (int v = 0; v < nv && !err; v++)
      {
         launch_copy(fK, m.f + (size_t) v * m.stride, (size_t) nK, s);
         if (presmoothed[(size_t) K]) { launch_copy(uK, m.home + (size_t) v * m.stride, (size_t) nK, s); d->F_array[K]->all_zeros = 0; }
         d->U_array[K]->all_zeros = 1;
         d->cycle_op_count = 0;
         err = amg_cycle_from(d, d->F_array, d->U_array, K, presmoothed[(size_t) K]);
         tail_count = d->cycle_op_count;
         launch_copy(m.home + (size_t) v * m.stride, uK, (size_t) nK, s);
      }
      handle().fp32_values = false;
      lv[(size_t) K].cur = lv[(size_t) K].home;
   }
   // ---- up
   for (int l = K - 1; l >= 0 && !err; l--)
   {
      Lv &uf = lv[(size_t) l], &uc = lv[(size_t) (l + 1)];
      const int flips = d->num_grid_sweeps[2];
      double *target = (flips % 2 == 0) ? uf.home : uf.alt;
      const size_t ts = (flips % 2 == 0) ? uf.hs : uf.as;
      spmv_columns(1.0, P[l]->diag, uc.cur, uc.cs(), 1.0, uf.cur, uf.cs(), target, ts, nv);
      uf.cur = target;
      const double w = d->relax_weight[l];
      const double *dg = diag_of(l, d->grid_relax_type[2]);
      for (int j = 0; j < d->num_grid_sweeps[2]; j++)
      {
         op_count += A[l]->d_num_nonzeros;
         spmv_columns_jacobi(A[l]->diag, F[(size_t) l], fs[(size_t) l], w, dg, uf.cur, uf.cs(), uf.other(), uf.os(), nv);
         uf.flip();
      }
   }
   if (!err && lv[0].cur != lv[0].home)
   {
      for (int v = 0; v < nv; v++) { launch_copy(lv[0].home + (size_t) v * lv[0].hs, lv[0].cur + (size_t) v * lv[0].as, (size_t) n, s); }
   }
   d->cycle_op_count = op_count + tail_count;          // (one cycle's count, as with one column)
   handle().fp32_values = saved_fp32;
   return err;
}
}  // namespace
}  // extern "C++"

// Multi-column solves cycle their large levels for all columns at once from now on (1) or column by column (0): speed only,
// same bits.  Nothing recorded is invalidated: a graph only ever sees the single-column vectors.  on < 0: unchanged; returns
// the setting.
HYPRE_Int hypre_amd_SetMultivectorCycle(HYPRE_Int on)
{
   if (on >= 0) { multivector_cycle() = on != 0; }
   return multivector_cycle();
}

// The solve of num_vectors = NV columns stored one after the other.  Every cycle runs column by column on the solver's
// single-column level vectors, with each column a view of the caller's storage: column v of an NV-column cycle is the
// single-vector cycle on column v, bit for bit, launch for launch (coarse-tail graph and one-workgroup tail included).
// The convergence test is the reference's: one residual norm and one right-hand-side norm over all columns, one
// iteration count.  A refused solve sets the error flag before anything is written.
static HYPRE_Int amg_solve_columns(hypre_ParAMGData *d, hypre_ParCSRMatrix *A, hypre_ParVector *f, hypre_ParVector *u)
{
   hypre_Vector *fl = f->local_vector, *ul = u->local_vector;
   const int nv = ul->num_vectors;
   if (fl->num_vectors != nv)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "Error: num_vectors for RHS and LHS do not match!");
      return hypre_error_flag;
   }
   const int n = A->diag->num_rows;
   if (fl->size != n || ul->size != n || fl->idxstride != 1 || ul->idxstride != 1 || fl->vecstride != n || ul->vecstride != n)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGSolve: multicomponent f and u must store their columns one after the "
                                             "other (vecstride = local size, idxstride = 1)");
      return hypre_error_flag;
   }
   const std::string why = multivector_refusal(d);
   if (!why.empty()) { hypre_error_w_msg(HYPRE_ERROR_GENERIC, why.c_str()); return hypre_error_flag; }

   AmgPrivate *pv = (AmgPrivate *) d->amd_private;
   const HYPRE_Real tol = d->tol;
   QuietSync quiet;
   if (d->max_iter > 1) { verify_par_plans(A); }
   d->A_array[0] = A;
   hypre_ParVectorSetLocalSize(d->Vtemp, n);
   std::vector<hypre_Vector> fc((size_t) nv), uc((size_t) nv);
   std::vector<hypre_ParVector> fp((size_t) nv), up((size_t) nv);
   for (int v = 0; v < nv; v++)
   {
      fc[(size_t) v] = *fl; fc[(size_t) v].data = fl->data + (size_t) v * n; fc[(size_t) v].num_vectors = 1; fc[(size_t) v].owns_data = 0;
      uc[(size_t) v] = *ul; uc[(size_t) v].data = ul->data + (size_t) v * n; uc[(size_t) v].num_vectors = 1; uc[(size_t) v].owns_data = 0;
      fp[(size_t) v] = *f; fp[(size_t) v].local_vector = &fc[(size_t) v]; fp[(size_t) v].owns_data = 0;
      up[(size_t) v] = *u; up[(size_t) v].local_vector = &uc[(size_t) v]; up[(size_t) v].owns_data = 0;
   }

   const bool track = d->print_level > 1 || d->logging > 1 || tol > 0.;
   hypre_ParVector *R = nullptr;
   if (track)
   {
      if (pv->mv_resid && (pv->mv_resid_cols < nv || pv->mv_resid->actual_local_size < n))
      {
         hypre_ParVectorDestroy(pv->mv_resid);
         pv->mv_resid = nullptr;
      }
      if (!pv->mv_resid)
      {
         pv->mv_resid = hypre_ParMultiVectorCreate(A->comm, A->global_num_rows, A->row_starts, nv);
         hypre_ParVectorInitialize_v2(pv->mv_resid, HYPRE_MEMORY_DEVICE);
         pv->mv_resid_cols = nv;
      }
      R = pv->mv_resid;
      R->local_vector->num_vectors = nv;
      hypre_ParVectorSetLocalSize(R, n);
   }
   HYPRE_Real resid_nrm = 1.0, resid_nrm_init = 1.0, rhs_norm = 0.0, relative_resid = 1.0, old_resid, conv_factor = 0.0;
   if (track)
   {
      hypre_ParVectorCopy(f, R);
      if (tol > 0) { hypre_ParCSRMatrixMatvec(1.0, A, u, -1.0, R); }
      resid_nrm = std::sqrt(hypre_ParVectorInnerProd(R, R));
      HYPRE_Real ieee_check = 0.;
      if (resid_nrm != 0.) { ieee_check = resid_nrm / resid_nrm; }
      if (ieee_check != ieee_check)
      {
         if (d->print_level > 0) { fprintf(stderr, "ERROR -- hypre_BoomerAMGSolve: INFs and/or NaNs detected in input.\n"); }
         d->F_array[0] = f; d->U_array[0] = u;
         hypre_error(HYPRE_ERROR_GENERIC);
         return hypre_error_flag;
      }
      resid_nrm_init = resid_nrm;
      if (d->converge_type == 0)
      {
         rhs_norm = std::sqrt(hypre_ParVectorInnerProd(f, f));
         relative_resid = rhs_norm ? resid_nrm_init / rhs_norm : resid_nrm_init;
      }
   }
   HYPRE_Int cycle_count = 0;
   while ((relative_resid >= tol || cycle_count < d->min_iter) && cycle_count < d->max_iter)
   {
      // the large levels for all columns at once where this solver's cycle is served and the level vectors are to be had
      const int first_single = multivector_cycle() ? multivector_cycle_first(d, pv) : -1;
      if (first_single >= 1 && ensure_mv_levels(d, pv, nv, first_single))
      {
         d->F_array[0] = &fp[0]; d->U_array[0] = &up[0];
         amg_cycle_columns(d, pv, fl->data, ul->data, n, nv, first_single, u->all_zeros);
      }
      else
      {
         for (int v = 0; v < nv; v++)
         {
            d->cycle_op_count = 0;          // (one cycle's count, as with one column)
            d->F_array[0] = &fp[(size_t) v]; d->U_array[0] = &up[(size_t) v];
            hypre_BoomerAMGCycle(d, d->F_array, d->U_array);
         }
      }
      u->all_zeros = 0;
      if (track)
      {
         old_resid = resid_nrm;
         hypre_ParCSRMatrixMatvecOutOfPlace(1.0, A, u, -1.0, f, R);
         resid_nrm = std::sqrt(hypre_ParVectorInnerProd(R, R));
         conv_factor = old_resid ? resid_nrm / old_resid : resid_nrm;
         if (d->converge_type == 0) { relative_resid = rhs_norm ? resid_nrm / rhs_norm : resid_nrm; }
         else { relative_resid = resid_nrm / resid_nrm_init; }
         d->rel_resid_norm = relative_resid;
      }
      ++cycle_count;
      d->num_iterations = cycle_count;
      if (d->print_level > 1)
      {
         HYPRE_Int rank; hypre_MPI_Comm_rank(A->comm, &rank);
         if (rank == 0) { printf("    Cycle %2d   %e    %f     %e \n", cycle_count, resid_nrm, conv_factor, relative_resid); }
      }
   }
   d->F_array[0] = f; d->U_array[0] = u;        // (no view of a column outlives the call)
   if (cycle_count == d->max_iter && tol > 0.) { hypre_error(HYPRE_ERROR_CONV); }
   quiet.restore();
   maybe_sync();
   return hypre_error_flag;
}

// ===========================================================================
// outer solve loop (par_amg_solve.c:22-424)
// ===========================================================================
HYPRE_Int hypre_BoomerAMGSolve(void *amg_vdata, hypre_ParCSRMatrix *A, hypre_ParVector *f, hypre_ParVector *u)
{
   hypre_ParAMGData *d = (hypre_ParAMGData *) amg_vdata;
   if (!d) { hypre_error_in_arg(1); return hypre_error_flag; }
   if (d->num_levels < 1 || !d->A_array)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_BoomerAMGSolve: setup has not been run");
      return hypre_error_flag;
   }
   HYPRE_AMD_REQUIRE_DEVICE(A->diag->memory_location, "hypre_BoomerAMGSolve(A)");
   HYPRE_AMD_REQUIRE_DEVICE(f->local_vector->memory_location, "hypre_BoomerAMGSolve(f)");
   HYPRE_AMD_REQUIRE_DEVICE(u->local_vector->memory_location, "hypre_BoomerAMGSolve(u)");
   if (f->local_vector->num_vectors != 1 || u->local_vector->num_vectors != 1) { return amg_solve_columns(d, A, f, u); }
   const HYPRE_Real tol = d->tol;
   QuietSync quiet;
   // stand-alone solver (more than one cycle allowed): the fine-level plans are verified against the caller's arrays once
   // per solve (one pass over the CSR arrays; a Krylov method that applies one cycle per iteration does it itself, once per
   // solve — HYPRE_ParCSRPCGSolve / GMRESSolve)
   if (d->max_iter > 1) { verify_par_plans(A); }
   d->A_array[0] = A; d->F_array[0] = f; d->U_array[0] = u;
   hypre_ParVector *Vtemp = d->Vtemp;
   hypre_ParVectorSetLocalSize(Vtemp, A->diag->num_rows);

   HYPRE_Real resid_nrm = 1.0, resid_nrm_init = 1.0, rhs_norm = 0.0, relative_resid = 1.0, old_resid, conv_factor = 0.0;
   HYPRE_Int cycle_count = 0;
   if (d->print_level > 1 || d->logging > 1 || tol > 0.)
   {
      hypre_ParVectorCopy(f, Vtemp);
      // r0 = A u - f: alpha = +1, beta = -1 exactly as the reference forms it (:170-189)
      if (tol > 0) { hypre_ParCSRMatrixMatvec(1.0, A, u, -1.0, Vtemp); }
      resid_nrm = std::sqrt(hypre_ParVectorInnerProd(Vtemp, Vtemp));
      HYPRE_Real ieee_check = 0.;
      if (resid_nrm != 0.) { ieee_check = resid_nrm / resid_nrm; }
      if (ieee_check != ieee_check)
      {
         if (d->print_level > 0)
         {
            fprintf(stderr, "ERROR -- hypre_BoomerAMGSolve: INFs and/or NaNs detected in input.\n");
         }
         hypre_error(HYPRE_ERROR_GENERIC);
         return hypre_error_flag;
      }
      resid_nrm_init = resid_nrm;
      if (d->converge_type == 0)
      {
         rhs_norm = std::sqrt(hypre_ParVectorInnerProd(f, f));
         relative_resid = rhs_norm ? resid_nrm_init / rhs_norm : resid_nrm_init;
      }
      else { relative_resid = 1.0; }
   }
   else { relative_resid = 1.; }

   HYPRE_Int Solve_err_flag = 0;
   while ((relative_resid >= tol || cycle_count < d->min_iter) && cycle_count < d->max_iter)
   {
      d->cycle_op_count = 0;
      AmgPrivate *pv = (AmgPrivate *) d->amd_private;
      if (pv->mixed_precision && !u->all_zeros)
      {
         // Mixed precision from an iterate that is not known to be zero: the cycle's operators carry fp32-rounded
         // values, so it is applied to the error equation — residual with the exact operator in fp64, cycle from a zero
         // guess, correction added in fp64 ("fp32 SpMV / fp64 residual").  From a zero guess (every preconditioner
         // call) the residual is f itself and the cycle runs on (f, u) directly.
         const HYPRE_Int nloc = A->diag->num_rows;
         if (pv->mp_r && pv->mp_r->local_vector->size != nloc)
         {
            hypre_ParVectorDestroy(pv->mp_r); hypre_ParVectorDestroy(pv->mp_e);
            pv->mp_r = pv->mp_e = nullptr;
         }
         if (!pv->mp_r)
         {
            pv->mp_r = hypre_ParVectorCreate(A->comm, A->global_num_rows, A->row_starts);
            pv->mp_e = hypre_ParVectorCreate(A->comm, A->global_num_rows, A->row_starts);
            hypre_ParVectorInitialize_v2(pv->mp_r, HYPRE_MEMORY_DEVICE);
            hypre_ParVectorInitialize_v2(pv->mp_e, HYPRE_MEMORY_DEVICE);
         }
         hypre_ParCSRMatrixMatvecOutOfPlace(-1.0, A, u, 1.0, f, pv->mp_r);
         hypre_ParVectorSetZeros(pv->mp_e);
         d->F_array[0] = pv->mp_r; d->U_array[0] = pv->mp_e;
         hypre_BoomerAMGCycle(d, d->F_array, d->U_array);
         d->F_array[0] = f; d->U_array[0] = u;
         hypre_ParVectorAxpy(1.0, pv->mp_e, u);
      }
      else { hypre_BoomerAMGCycle(d, d->F_array, d->U_array); }
      if (d->print_level > 1 || d->logging > 1 || tol > 0.)
      {
         old_resid = resid_nrm;
         hypre_ParVectorSetLocalSize(Vtemp, A->diag->num_rows);
         hypre_ParCSRMatrixMatvecOutOfPlace(1.0, A, u, -1.0, f, Vtemp);
         resid_nrm = std::sqrt(hypre_ParVectorInnerProd(Vtemp, Vtemp));
         conv_factor = old_resid ? resid_nrm / old_resid : resid_nrm;
         if (d->converge_type == 0) { relative_resid = rhs_norm ? resid_nrm / rhs_norm : resid_nrm; }
         else { relative_resid = resid_nrm / resid_nrm_init; }
         d->rel_resid_norm = relative_resid;
      }
      ++cycle_count;
      d->num_iterations = cycle_count;
      if (d->print_level > 1)
      {
         HYPRE_Int rank; hypre_MPI_Comm_rank(A->comm, &rank);
         if (rank == 0) { printf("    Cycle %2d   %e    %f     %e \n", cycle_count, resid_nrm, conv_factor, relative_resid); }
      }
   }
   if (cycle_count == d->max_iter && tol > 0.)
   {
      Solve_err_flag = 1;
      hypre_error(HYPRE_ERROR_CONV);
   }
   (void) Solve_err_flag;
   quiet.restore();
   maybe_sync();
   return hypre_error_flag;
}

}  // extern "C"
