// hypre_amd — block-Jacobi ILU(k) as a solver and as a preconditioner: HYPRE_ILU* (parcsr_ls/HYPRE_parcsr_ilu.c, par_ilu.c,
// par_ilu_setup.c, par_ilu_solve.c; the reference's `ij -solver 80 | 81 | 82` with -ilu_type 0).  Every rank factors its
// diagonal block; couplings to other ranks appear in the residual product with A only.
//
// Setup runs on the host (ilu_host.hpp): local reverse Cuthill-McKee ordering, the level-of-fill pattern, the numeric
// factorisation in the permuted order, then the dependency levels of L and of U.  The factors are uploaded in level order
// with the permutation folded into their indices (ilu_device.hpp).  One application, hypre_ILUSolveLU, is
//    ftemp = f - A u  (hypre_ParCSRMatrixMatvecOutOfPlace),  utemp = (L D^-1 U)^-1 ftemp,  u += utemp
// and the last two steps are the launches of ilu_kernels.hip: a grid for a level wider than a workgroup, one workgroup
// with a barrier per level for a run of narrower ones.  Objects in host memory are served by the host solve, which the
// device reproduces bit for bit.  The reference's own device path hands factorisation and solves to rocSPARSE.
//
// With hypre_amd_ILUSetIterativeTriSolve on (the reference's tri_solve 0, hypre_ILUSolveLUIter) each triangular solve is a
// fixed number of Jacobi sweeps from a zero iterate.  The factors then lie in row slices as well (ilu_host.hpp: Slices) and
// an application is at most lower + upper launches of ilu_iter_kernels.hip beside the product with A, whatever the level
// count; host operands take ilu::solve_iter, which the sweeps reproduce bit for bit.
#include "amg_internal.hpp"
#include "ilu_device.hpp"
#include "ilu_host.hpp"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace hamd;

extern "C" {

struct hypre_amd_ILUData
{
   hypre_Solver base;
   // defaults of hypre_ILUCreate (par_ilu.c:61-106)
   HYPRE_Int  ilu_type = 0, lfil = 0, reordering = 1, tri_solve = 1, max_iter = 20, logging = 0, print_level = 0;
   HYPRE_Real tol = 1.0e-7;
   HYPRE_Int  num_iterations = 0;
   HYPRE_Real final_rel_residual_norm = 0.0, operator_complexity = 0.0;
   bool       is_setup = false;
   ilu::Factors F;
   ilu::Levels  VL, VU;
   // device side: the two factors in level order, the work vectors of an application
   bool    uploaded = false;
   int    *d_int = nullptr;           // one allocation for every index table
   double *d_real = nullptr;          // one for every value table and utemp
   IluTri  dL, dU;
   double *d_utemp = nullptr;
   hypre_ParVector *ftemp = nullptr;  // device residual (the product writes a ParVector)
   std::vector<double> h_ftemp, h_utemp, h_ghost, h_send;
   std::vector<HYPRE_Real> norms;     // relative residual norm after every iteration, when norms are computed
   HYPRE_Int run_launches = 0, level_launches = 0;     // of the last application
   // iterative triangular solves: the switch, the sweeps per factor (hypre_ILUCreate: 5 and 5), the factors in row slices
   HYPRE_Int  iterative = 0, lower_iters = 5, upper_iters = 5, sweep_launches = 0;
   long long  padded_L = 0, padded_U = 0;    // entries of the slice form with its padding, counted at Setup
   bool       iter_uploaded = false;
   int       *d_iter_int = nullptr;
   double    *d_iter_real = nullptr;
   long long *d_iter_base = nullptr;
   IluSlices  sL, sU;
   double    *d_work[3] = {nullptr, nullptr, nullptr};  // iterates of the sweeps, ping-ponged
   std::vector<double> h_ztemp;
};

}  // extern "C"

namespace {
hypre_amd_ILUData *D(HYPRE_Solver s) { return (hypre_amd_ILUData *) s; }

bool refuse_null(HYPRE_Solver s)
{
   if (s) { return false; }
   hypre_error_in_arg(1);
   return true;
}

void release_device(hypre_amd_ILUData *d)
{
   if (d->d_int) { (void) hipFree(d->d_int); d->d_int = nullptr; }
   if (d->d_real) { (void) hipFree(d->d_real); d->d_real = nullptr; }
   if (d->ftemp) { hypre_ParVectorDestroy(d->ftemp); d->ftemp = nullptr; }
   d->dL = IluTri{}; d->dU = IluTri{};
   d->d_utemp = nullptr;
   d->uploaded = false;
   if (d->d_iter_int) { (void) hipFree(d->d_iter_int); d->d_iter_int = nullptr; }
   if (d->d_iter_real) { (void) hipFree(d->d_iter_real); d->d_iter_real = nullptr; }
   if (d->d_iter_base) { (void) hipFree(d->d_iter_base); d->d_iter_base = nullptr; }
   d->sL = IluSlices{}; d->sU = IluSlices{};
   d->d_work[0] = d->d_work[1] = d->d_work[2] = nullptr;
   d->iter_uploaded = false;
}

// one factor in level order on the host: slot tables and entries, permutation folded in
struct TriImage { std::vector<int> ptr, row, col; std::vector<double> val, dinv; };
void level_order(const ilu::Factors &F, const ilu::Levels &V, const std::vector<int> &Ti, const std::vector<int> &Tj, const std::vector<double> &Ta,
                 bool upper, TriImage &M)
{
   const int n = F.n;
   M.ptr.assign((size_t) n + 1, 0); M.row.assign((size_t) n, 0);
   M.col.clear(); M.val.clear(); M.dinv.clear();
   M.col.reserve(Tj.size()); M.val.reserve(Ta.size());
   for (int s = 0; s < n; s++)
   {
      const int r = V.order[(size_t) s];
      M.row[(size_t) s] = F.perm[(size_t) r];
      for (int k = Ti[(size_t) r]; k < Ti[(size_t) r + 1]; k++) { M.col.push_back(F.perm[(size_t) Tj[(size_t) k]]); M.val.push_back(Ta[(size_t) k]); }
      M.ptr[(size_t) s + 1] = (int) M.col.size();
      if (upper) { M.dinv.push_back(F.D[(size_t) r]); }
   }
}

void upload(hypre_amd_ILUData *d, hypre_ParCSRMatrix *A)
{
   release_device(d);
   const int n = d->F.n;
   TriImage L, U;
   level_order(d->F, d->VL, d->F.Li, d->F.Lj, d->F.La, false, L);
   level_order(d->F, d->VU, d->F.Ui, d->F.Uj, d->F.Ua, true, U);
   std::vector<int> ints;
   std::vector<double> reals;
   auto put_i = [&](const std::vector<int> &v) { const size_t at = ints.size(); ints.insert(ints.end(), v.begin(), v.end()); return at; };
   auto put_r = [&](const std::vector<double> &v) { const size_t at = reals.size(); reals.insert(reals.end(), v.begin(), v.end()); return at; };
   const size_t lp = put_i(L.ptr), lr = put_i(L.row), lc = put_i(L.col), ll = put_i(d->VL.lev_start);
   const size_t up = put_i(U.ptr), ur = put_i(U.row), uc = put_i(U.col), ul = put_i(d->VU.lev_start);
   const size_t lv = put_r(L.val), uv = put_r(U.val), ud = put_r(U.dinv), ut = reals.size();
   reals.resize(reals.size() + (size_t) std::max(n, 1), 0.0);
   HIP_CHECK(hipMalloc((void **) &d->d_int, sizeof(int) * ints.size()));
   HIP_CHECK(hipMalloc((void **) &d->d_real, sizeof(double) * reals.size()));
   if (!d->d_int || !d->d_real) { release_device(d); return; }
   HIP_CHECK(hipMemcpy(d->d_int, ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(d->d_real, reals.data(), sizeof(double) * reals.size(), hipMemcpyHostToDevice));
   d->dL.ptr = d->d_int + lp; d->dL.row = d->d_int + lr; d->dL.col = d->d_int + lc; d->dL.lev_start = d->d_int + ll;
   d->dU.ptr = d->d_int + up; d->dU.row = d->d_int + ur; d->dU.col = d->d_int + uc; d->dU.lev_start = d->d_int + ul;
   d->dL.val = d->d_real + lv; d->dU.val = d->d_real + uv; d->dU.dinv = d->d_real + ud;
   d->d_utemp = d->d_real + ut;
   d->ftemp = hypre_ParVectorCreate(A->comm, A->global_num_rows, A->row_starts);
   hypre_ParVectorInitialize_v2(d->ftemp, HYPRE_MEMORY_DEVICE);
   d->uploaded = true;
}

// the slice form of both factors and the three work vectors of the sweeps; the level-ordered form stays where it is
void upload_iter(hypre_amd_ILUData *d)
{
   const int n = d->F.n;
   ilu::Slices L, U;
   ilu::build_slices(d->F, d->VL.order, d->F.Li, d->F.Lj, d->F.La, L);
   ilu::build_slices(d->F, d->VU.order, d->F.Ui, d->F.Uj, d->F.Ua, U);
   std::vector<int> ints;
   std::vector<double> reals;
   std::vector<long long> bases;
   auto put_i = [&](const std::vector<int> &v) { const size_t at = ints.size(); ints.insert(ints.end(), v.begin(), v.end()); return at; };
   auto put_r = [&](const std::vector<double> &v) { const size_t at = reals.size(); reals.insert(reals.end(), v.begin(), v.end()); return at; };
   const size_t ll = put_i(L.len), lr = put_i(L.row), lc = put_i(L.col), ul = put_i(U.len), ur = put_i(U.row), uc = put_i(U.col);
   const size_t lv = put_r(L.val), ld = put_r(L.dinv), uv = put_r(U.val), ud = put_r(U.dinv), w = reals.size();
   const size_t nw = (size_t) std::max(n, 1);
   reals.resize(reals.size() + 3 * nw, 0.0);
   ints.push_back(0);                                    // never an empty allocation
   bases.insert(bases.end(), L.base.begin(), L.base.end());
   bases.insert(bases.end(), U.base.begin(), U.base.end());
   bases.push_back(0);
   HIP_CHECK(hipMalloc((void **) &d->d_iter_int, sizeof(int) * ints.size()));
   HIP_CHECK(hipMalloc((void **) &d->d_iter_real, sizeof(double) * reals.size()));
   HIP_CHECK(hipMalloc((void **) &d->d_iter_base, sizeof(long long) * bases.size()));
   if (!d->d_iter_int || !d->d_iter_real || !d->d_iter_base)
   {
      if (d->d_iter_int) { (void) hipFree(d->d_iter_int); d->d_iter_int = nullptr; }
      if (d->d_iter_real) { (void) hipFree(d->d_iter_real); d->d_iter_real = nullptr; }
      if (d->d_iter_base) { (void) hipFree(d->d_iter_base); d->d_iter_base = nullptr; }
      return;
   }
   HIP_CHECK(hipMemcpy(d->d_iter_int, ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(d->d_iter_real, reals.data(), sizeof(double) * reals.size(), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(d->d_iter_base, bases.data(), sizeof(long long) * bases.size(), hipMemcpyHostToDevice));
   d->sL.base = d->d_iter_base; d->sU.base = d->d_iter_base + L.base.size();
   d->sL.len = d->d_iter_int + ll; d->sL.row = d->d_iter_int + lr; d->sL.col = d->d_iter_int + lc;
   d->sU.len = d->d_iter_int + ul; d->sU.row = d->d_iter_int + ur; d->sU.col = d->d_iter_int + uc;
   d->sL.val = d->d_iter_real + lv; d->sL.dinv = d->d_iter_real + ld; d->sU.val = d->d_iter_real + uv; d->sU.dinv = d->d_iter_real + ud;
   d->sL.nslices = L.nslices; d->sU.nslices = U.nslices;
   for (int k = 0; k < 3; k++) { d->d_work[k] = d->d_iter_real + w + (size_t) k * nw; }
   d->iter_uploaded = true;
}

// One application as sweeps: u += z, z the last upper iterate.  y^1 = rhs and z^1 = Dinv y have sums of +0.0 and read no
// matrix, so a factor with k sweeps costs k - 1 products: the first L pass reads rhs as its iterate, the last L pass stores
// y and z^1 = Dinv y, the last U pass adds into u.  Launches: lower - 1 + upper - 1, one more when lower is 1 (z^1 = Dinv rhs
// has no L pass to ride on); never more than lower + upper, whatever n and the level count.  Three work vectors: while U is
// swept y stays and z ping-pongs; rhs may be the caller's own and is only read.  Returns the bytes the launches require.
double run_sweeps(hypre_amd_ILUData *d, const double *rhs, double *u, hipStream_t s)
{
   const int lower = d->lower_iters, upper = d->upper_iters, n = d->F.n;
   if (lower <= 0 || upper <= 0 || n <= 0) { return 0.0; }
   double bytes = 0.0;
   auto launch = [&](const IluSweepArgs &a, bool up) {
      launch_ilu_sweep(a, up, s);
      d->sweep_launches++;
      // slot tables (length, vector index: 8), rhs (8), slice bases; entries and the gathered iterate when a product is formed;
      // inverse pivots when used; every vector stored; u read and written
      bytes += 8.0 * a.t.nslices + (double) n * (16.0 + (a.in ? 8.0 : 0.0) + (a.out ? 8.0 : 0.0) + ((up || a.scale) ? 8.0 : 0.0) +
                                                 (a.scaled ? 8.0 : 0.0) + (a.u ? 16.0 : 0.0)) +
               (a.in ? 12.0 * (double) (up ? d->padded_U : d->padded_L) : 0.0);
   };
   double *const *W = d->d_work;
   const double *y = rhs;                 // the last lower iterate: rhs itself with one sweep
   int ybuf = -1;
   const double *prev = rhs;              // y^1 = rhs
   for (int k = 2; k <= lower; k++)
   {
      IluSweepArgs a{};
      a.t = d->sL; a.rhs = rhs; a.in = prev;
      ybuf = k & 1;                       // W[0], W[1], W[0], ...
      a.out = W[ybuf];
      if (k == lower)
      {
         a.scale = 1;
         if (upper == 1) { a.out = nullptr; a.u = u; }
         else { a.scaled = W[2]; }
      }
      launch(a, false);
      prev = y = W[ybuf];
   }
   if (lower == 1)
   {
      // z^1 = Dinv rhs alone: the L pass from the zero iterate, nothing of the factor's entries read
      IluSweepArgs a{};
      a.t = d->sL; a.rhs = rhs; a.scale = 1;
      if (upper == 1) { a.u = u; }
      else { a.scaled = W[2]; }
      launch(a, false);
   }
   // z^1 lies in W[2]; y in W[ybuf] (or in rhs); the other of W[0] / W[1] is free
   const int spare = ybuf == 0 ? 1 : 0;
   int zbuf = 2;
   for (int k = 2; k <= upper; k++)
   {
      IluSweepArgs a{};
      a.t = d->sU; a.rhs = y; a.in = W[zbuf];
      zbuf = zbuf == 2 ? spare : 2;
      if (k == upper) { a.u = u; }
      else { a.out = W[zbuf]; }
      launch(a, true);
   }
   return bytes;
}

// the levels of one factor: a level wider than a workgroup gets a grid, consecutive narrower ones share a launch
void run_levels(hypre_amd_ILUData *d, const ilu::Levels &V, const IluArgs &a, bool upper, hipStream_t s)
{
   int lev = 0;
   while (lev < V.nlev)
   {
      const int cnt = V.lev_start[(size_t) lev + 1] - V.lev_start[(size_t) lev];
      if (cnt <= ILU_RUN_THREADS)
      {
         int end = lev + 1;
         while (end < V.nlev && end - lev < ILU_RUN_MAX_LEVELS && V.lev_start[(size_t) end + 1] - V.lev_start[(size_t) end] <= ILU_RUN_THREADS) { end++; }
         launch_ilu_run(a, upper, lev, end, s);
         d->run_launches++;
         lev = end;
      }
      else
      {
         launch_ilu_level(a, upper, V.lev_start[(size_t) lev], cnt, s);
         d->level_launches++;
         lev++;
      }
   }
}

// ---- the three steps of the iteration, on the device and on the host ----
struct Ops
{
   hypre_amd_ILUData *d;
   hypre_ParCSRMatrix *A;
   hypre_ParVector *f, *u;
   bool device;
   int n;

   // ftemp = f - A u
   void residual()
   {
      if (device) { hypre_ParCSRMatrixMatvecOutOfPlace(-1.0, A, u, 1.0, f, d->ftemp); return; }
      const hypre_CSRMatrix *diag = A->diag, *offd = A->offd;
      const double *ud = u->local_vector->data, *fd = f->local_vector->data;
      HYPRE_Int nprocs;
      hypre_MPI_Comm_size(A->comm, &nprocs);
      const bool ghosts = nprocs > 1 && offd && offd->num_cols > 0 && offd->num_nonzeros > 0;
      if (nprocs > 1)
      {
         // owner -> ghost exchange of u in host memory (collective: every rank takes part, with or without ghosts)
         if (!A->comm_pkg) { hypre_MatvecCommPkgCreate(A); }
         hypre_ParCSRCommPkg *pkg = A->comm_pkg;
         const HYPRE_Int tot_send = pkg->send_map_starts[pkg->num_sends];
         d->h_send.assign((size_t) std::max<HYPRE_Int>(tot_send, 1), 0.0);
         d->h_ghost.assign((size_t) std::max<HYPRE_Int>(offd ? offd->num_cols : 0, 1), 0.0);
         for (HYPRE_Int i = 0; i < tot_send; i++) { d->h_send[(size_t) i] = ud[pkg->send_map_elmts[i]]; }
         hypre_ParCSRCommHandleDestroy(hypre_ParCSRCommHandleCreate(1, pkg, d->h_send.data(), d->h_ghost.data()));
      }
      for (int i = 0; i < n; i++)
      {
         double s = fd[i];
         for (HYPRE_Int k = diag->i[i]; k < diag->i[i + 1]; k++) { s -= diag->data[k] * ud[diag->j[k]]; }
         if (ghosts) { for (HYPRE_Int k = offd->i[i]; k < offd->i[i + 1]; k++) { s -= offd->data[k] * d->h_ghost[(size_t) offd->j[k]]; } }
         d->h_ftemp[(size_t) i] = s;
      }
   }
   double norm_of(const double *v) const
   {
      double s = 0.0;
      for (int i = 0; i < n; i++) { s += v[i] * v[i]; }
      return std::sqrt(global_sum(A->comm, s));
   }
   double residual_norm() const
   {
      return device ? std::sqrt(hypre_ParVectorInnerProd(d->ftemp, d->ftemp)) : norm_of(d->h_ftemp.data());
   }
   double rhs_norm() const { return device ? std::sqrt(hypre_ParVectorInnerProd(f, f)) : norm_of(f->local_vector->data); }
   // hypre_ILUSolveLU: u += (L D^-1 U)^-1 (f - A u).  An iterate known to be zero (all_zeros: hypre_ParVectorSetZeros, the
   // cycle on the way down) needs no product: f - A 0 is f, the same number, so f itself is the right-hand side.
   void apply()
   {
      if (u->all_zeros && f->local_vector->data != u->local_vector->data)
      {
         apply_factors(f->local_vector->data);
         return;
      }
      residual();
      apply_factors(device ? d->ftemp->local_vector->data : d->h_ftemp.data());
   }
   // u += (L D^-1 U)^-1 rhs
   void apply_factors(const double *rhs)
   {
      d->run_launches = d->level_launches = d->sweep_launches = 0;
      if (d->iterative)
      {
         if (device) { account_bytes(run_sweeps(d, rhs, u->local_vector->data, stream())); }
         else if (d->lower_iters > 0 && d->upper_iters > 0)
         {
            ilu::solve_iter(d->F, rhs, d->h_utemp.data(), d->h_ztemp.data(), d->lower_iters, d->upper_iters);
            double *ud = u->local_vector->data;
            for (int i = 0; i < n; i++) { ud[i] = ud[i] + d->h_ztemp[(size_t) i]; }
         }
      }
      else if (device)
      {
         if (n > 0)
         {
            hipStream_t s = stream();
            IluArgs a{};
            a.ftemp = rhs; a.utemp = d->d_utemp; a.u = u->local_vector->data;
            a.t = d->dL; run_levels(d, d->VL, a, false, s);
            a.t = d->dU; run_levels(d, d->VU, a, true, s);
            account_bytes(12.0 * (double) (d->F.Lj.size() + d->F.Uj.size()) + (double) n * (2 * 8 + 8 + 5 * 8));
         }
      }
      else
      {
         ilu::solve(d->F, rhs, d->h_utemp.data());
         double *ud = u->local_vector->data;
         for (int i = 0; i < n; i++) { ud[i] = ud[i] + d->h_utemp[(size_t) i]; }
      }
      u->all_zeros = 0;
   }
   void zero_u()
   {
      if (device) { hypre_ParVectorSetConstantValues(u, 0.0); }
      else { for (int i = 0; i < n; i++) { u->local_vector->data[i] = 0.0; } }
   }
};
}  // namespace

extern "C" {

HYPRE_Int HYPRE_ILUSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ILUSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x);
HYPRE_Int HYPRE_ILUDestroy(HYPRE_Solver solver);

HYPRE_Int HYPRE_ILUCreate(HYPRE_Solver *solver)
{
   if (!solver) { hypre_error_in_arg(1); return hypre_error_flag; }
   hypre_amd_ILUData *d = new hypre_amd_ILUData();
   d->base.setup = (HYPRE_PtrToSolverFcn) HYPRE_ILUSetup;
   d->base.solve = (HYPRE_PtrToSolverFcn) HYPRE_ILUSolve;
   d->base.destroy = (HYPRE_PtrToDestroyFcn) HYPRE_ILUDestroy;
   *solver = (HYPRE_Solver) d;
   return hypre_error_flag;
}

HYPRE_Int HYPRE_ILUDestroy(HYPRE_Solver solver)
{
   hypre_amd_ILUData *d = D(solver);
   if (!d) { return hypre_error_flag; }
   release_device(d);
   delete d;
   return hypre_error_flag;
}

// what lies outside block-Jacobi ILU(k) is refused where it is asked for
HYPRE_Int HYPRE_ILUSetType(HYPRE_Solver s, HYPRE_Int ilu_type)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (ilu_type != 0)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, ("HYPRE_ILUSetType: ilu_type " + std::to_string(ilu_type) + " is outside the scope of this library "
                                              "(0: block Jacobi with ILU(k); ILUT and the Schur, NSH, RAS, ddPQ and RAP types are not served)").c_str());
      return hypre_error_flag;
   }
   D(s)->ilu_type = ilu_type;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetLevelOfFill(HYPRE_Solver s, HYPRE_Int lfil)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (lfil < 0) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->lfil = lfil;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetLocalReordering(HYPRE_Solver s, HYPRE_Int reordering_type)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (reordering_type != 0 && reordering_type != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->reordering = reordering_type;
   return hypre_error_flag;
}
// The iterative triangular solves (the reference's tri_solve 0) are served, through hypre_amd_ILUSetIterativeTriSolve,
// HYPRE_ILUSetLowerJacobiIters and HYPRE_ILUSetUpperJacobiIters below.  This setter still refuses 0: its refusal is pinned by
// the tests of the commit that brought ILU, which stay as they are, so the capability got a switch of its own beside it.
HYPRE_Int HYPRE_ILUSetTriSolve(HYPRE_Solver s, HYPRE_Int tri_solve)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (tri_solve != 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, ("HYPRE_ILUSetTriSolve: tri_solve " + std::to_string(tri_solve) + " is outside the scope of this library "
                                              "(1: direct triangular solves; the iterative solves are switched on by hypre_amd_ILUSetIterativeTriSolve)").c_str());
      return hypre_error_flag;
   }
   D(s)->tri_solve = tri_solve;
   return hypre_error_flag;
}
// hypre_ILUSetLowerJacobiIters / hypre_ILUSetUpperJacobiIters (par_ilu.c): sweeps per triangular solve when the solves are iterative
HYPRE_Int HYPRE_ILUSetLowerJacobiIters(HYPRE_Solver s, HYPRE_Int lower_jacobi_iters)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (lower_jacobi_iters < 0) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->lower_iters = lower_jacobi_iters;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetUpperJacobiIters(HYPRE_Solver s, HYPRE_Int upper_jacobi_iters)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (upper_jacobi_iters < 0) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->upper_iters = upper_jacobi_iters;
   return hypre_error_flag;
}
// 1: every triangular solve is lower / upper Jacobi sweeps (the reference's tri_solve 0); 0, the default: direct solves.
// May be flipped between two solves of one Setup: the slice form of the factors is built when first needed.
HYPRE_Int hypre_amd_ILUSetIterativeTriSolve(HYPRE_Solver s, HYPRE_Int iterative)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (iterative != 0 && iterative != 1) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->iterative = iterative;
   D(s)->tri_solve = iterative ? 0 : 1;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetMaxIter(HYPRE_Solver s, HYPRE_Int max_iter)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (max_iter < 0) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->max_iter = max_iter;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetTol(HYPRE_Solver s, HYPRE_Real tol)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (!(tol >= 0.0)) { hypre_error_in_arg(2); return hypre_error_flag; }
   D(s)->tol = tol;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetPrintLevel(HYPRE_Solver s, HYPRE_Int print_level)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   D(s)->print_level = print_level;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUSetLogging(HYPRE_Solver s, HYPRE_Int logging)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   D(s)->logging = logging;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUGetNumIterations(HYPRE_Solver s, HYPRE_Int *num_iterations)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (!num_iterations) { hypre_error_in_arg(2); return hypre_error_flag; }
   *num_iterations = D(s)->num_iterations;
   return hypre_error_flag;
}
HYPRE_Int HYPRE_ILUGetFinalRelativeResidualNorm(HYPRE_Solver s, HYPRE_Real *res_norm)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   if (!res_norm) { hypre_error_in_arg(2); return hypre_error_flag; }
   *res_norm = D(s)->final_rel_residual_norm;
   return hypre_error_flag;
}
// the parameters as they stand (a new object: the defaults of hypre_ILUCreate); any pointer may be NULL
HYPRE_Int hypre_amd_ILUGetParameters(HYPRE_Solver s, HYPRE_Int *ilu_type, HYPRE_Int *lfil, HYPRE_Int *reordering, HYPRE_Int *tri_solve,
                                     HYPRE_Int *max_iter, HYPRE_Real *tol, HYPRE_Int *print_level, HYPRE_Int *logging)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   const hypre_amd_ILUData *d = D(s);
   if (ilu_type) { *ilu_type = d->ilu_type; }
   if (lfil) { *lfil = d->lfil; }
   if (reordering) { *reordering = d->reordering; }
   if (tri_solve) { *tri_solve = d->tri_solve; }
   if (max_iter) { *max_iter = d->max_iter; }
   if (tol) { *tol = d->tol; }
   if (print_level) { *print_level = d->print_level; }
   if (logging) { *logging = d->logging; }
   return hypre_error_flag;
}

// hypre_ILUSetup for ilu_type 0 (par_ilu_setup.c:24-700): ordering, factorisation and levels on the host, whatever memory A
// is in; the device form is uploaded when A is in device memory, or by the first Solve on device vectors
HYPRE_Int HYPRE_ILUSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   (void) b; (void) x;
   if (refuse_null(solver)) { return hypre_error_flag; }
   if (!A || !A->diag) { hypre_error_in_arg(2); return hypre_error_flag; }
   hypre_amd_ILUData *d = D(solver);
   const hypre_CSRMatrix *diag = A->diag;
   const int n = diag->num_rows, nnz = diag->num_nonzeros;
   if (diag->num_cols != n)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ILUSetup: the diagonal block of A is not square");
      return hypre_error_flag;
   }
   d->is_setup = false;
   release_device(d);
   std::vector<HYPRE_Int> hi((size_t) n + 1, 0), hj((size_t) std::max(nnz, 1));
   std::vector<HYPRE_Complex> ha((size_t) std::max(nnz, 1));
   const bool on_device = diag->memory_location == HYPRE_MEMORY_DEVICE;
   if (on_device) { HIP_CHECK(hipStreamSynchronize(stream())); }
   if (n > 0) { hypre_TMemcpy(hi.data(), diag->i, HYPRE_Int, (size_t) n + 1, HYPRE_MEMORY_HOST, diag->memory_location); }
   if (nnz > 0)
   {
      hypre_TMemcpy(hj.data(), diag->j, HYPRE_Int, (size_t) nnz, HYPRE_MEMORY_HOST, diag->memory_location);
      hypre_TMemcpy(ha.data(), diag->data, HYPRE_Complex, (size_t) nnz, HYPRE_MEMORY_HOST, diag->memory_location);
   }
   for (int k = 0; k < nnz; k++)
   {
      if (hj[(size_t) k] < 0 || hj[(size_t) k] >= n)
      {
         hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ILUSetup: a column of the diagonal block lies outside it");
         return hypre_error_flag;
      }
   }
   ilu::factor(n, hi.data(), hj.data(), ha.data(), d->lfil, d->reordering, d->F);
   ilu::build_levels(n, d->F.Li.data(), d->F.Lj.data(), true, d->VL);
   ilu::build_levels(n, d->F.Ui.data(), d->F.Uj.data(), false, d->VU);
   d->h_ftemp.assign((size_t) std::max(n, 1), 0.0);
   d->h_utemp.assign((size_t) std::max(n, 1), 0.0);
   d->h_ztemp.assign((size_t) std::max(n, 1), 0.0);
   // entries of the slice form: every slice of 64 rows of the level order as long as its longest row
   auto padded = [n](const std::vector<int> &order, const std::vector<int> &Ti) {
      long long total = 0;
      for (int s0 = 0; s0 < n; s0 += ilu::SLICE_ROWS)
      {
         int longest = 0;
         for (int t = s0; t < std::min(n, s0 + ilu::SLICE_ROWS); t++) { longest = std::max(longest, Ti[(size_t) order[(size_t) t] + 1] - Ti[(size_t) order[(size_t) t]]); }
         total += (long long) longest * ilu::SLICE_ROWS;
      }
      return total;
   };
   d->padded_L = padded(d->VL.order, d->F.Li);
   d->padded_U = padded(d->VU.order, d->F.Ui);
   // fill of the factors over the entries of A, all ranks (par_ilu_setup.c:640-660; printed by Solve at print level > 1)
   const double fill = global_sum(A->comm, (double) n + (double) d->F.Lj.size() + (double) d->F.Uj.size());
   const double nnzA = global_sum(A->comm, (double) nnz + (double) (A->offd ? A->offd->num_nonzeros : 0));
   d->operator_complexity = nnzA > 0.0 ? fill / nnzA : 0.0;
   d->num_iterations = 0;
   d->final_rel_residual_norm = 0.0;
   d->norms.clear();
   d->run_launches = d->level_launches = d->sweep_launches = 0;
   d->is_setup = true;
   if (on_device) { upload(d, A); }
   if (on_device && d->uploaded && d->iterative) { upload_iter(d); }
   return hypre_error_flag;
}

// hypre_ILUSolve for ilu_type 0 (par_ilu_solve.c:24-477).  As a preconditioner (tol 0, print level and logging at most
// 1) no norm is computed: max_iter applications, each one product with A and the two triangular solves.
HYPRE_Int HYPRE_ILUSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector f, HYPRE_ParVector u)
{
   return hamd::ilu_solve_core(solver, A, f, u, true);
}

}  // extern "C"

HYPRE_Int hamd::ilu_solve_core(HYPRE_Solver solver, hypre_ParCSRMatrix *A, hypre_ParVector *f, hypre_ParVector *u, bool verify_plans)
{
   if (refuse_null(solver)) { return hypre_error_flag; }
   hypre_amd_ILUData *d = D(solver);
   if (!d->is_setup)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ILUSolve: call HYPRE_ILUSetup first");
      return hypre_error_flag;
   }
   if (!A || !A->diag) { hypre_error_in_arg(2); return hypre_error_flag; }
   if (!f) { hypre_error_in_arg(3); return hypre_error_flag; }
   if (!u) { hypre_error_in_arg(4); return hypre_error_flag; }
   const int n = d->F.n;
   const hypre_Vector *fl = f->local_vector, *ul = u->local_vector;
   if (A->diag->num_rows != n || fl->size != n || ul->size != n)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ILUSolve: A, f and u must have the rows of the matrix HYPRE_ILUSetup factored");
      return hypre_error_flag;
   }
   if (fl->num_vectors != 1 || ul->num_vectors != 1)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ILUSolve: multicomponent vectors are outside the scope of this library's ILU");
      return hypre_error_flag;
   }
   const HYPRE_MemoryLocation loc = ul->memory_location;
   if (fl->memory_location != loc || A->diag->memory_location != loc)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "HYPRE_ILUSolve: A, f and u must lie in the same memory (all host or all device)");
      return hypre_error_flag;
   }
   const bool device = loc == HYPRE_MEMORY_DEVICE;
   if (device && !d->uploaded)
   {
      upload(d, A);
      if (!d->uploaded) { return hypre_error_flag; }
   }
   if (device && d->iterative && !d->iter_uploaded)
   {
      upload_iter(d);
      if (!d->iter_uploaded) { return hypre_error_flag; }
   }
   Ops op{d, A, f, u, device, n};
   const HYPRE_Int print_level = d->print_level, logging = d->logging, max_iter = d->max_iter;
   const HYPRE_Real tol = d->tol;
   HYPRE_Int my_id = 0, iter = 0;
   hypre_MPI_Comm_rank(A->comm, &my_id);
   const bool print = my_id == 0 && print_level > 1, with_norms = print_level > 1 || logging > 1 || tol > 0.;
   HYPRE_Real resnorm = 1.0, init_resnorm = 0.0, rel_resnorm, rhs_norm = 0.0, old_resnorm, conv_factor = 0.0, ieee_check = 0.0;

   QuietSync quiet;
   struct Finish { QuietSync &q; ~Finish() { q.restore(); maybe_sync(); } } finish{quiet};
   if (device && verify_plans) { verify_par_plans(A); }
   d->num_iterations = 0;
   d->norms.clear();
   if (print)
   {
      const std::string tri = d->iterative ? "triangular solves by " + std::to_string(d->lower_iters) + " lower and " + std::to_string(d->upper_iters) +
                                             " upper Jacobi sweeps" : std::string("direct triangular solves");
      printf("ILU SOLVER PARAMETERS:\n  ILU type 0 (block Jacobi with ILU(%d)), local reordering %d, %s\n"
             "  stopping tolerance %e, maximum iterations %d\n", (int) d->lfil, (int) d->reordering, tri.c_str(), tol, (int) max_iter);
      if (tol > 0.) { printf("\n\n ILU SOLVER SOLUTION INFO:\n"); }
   }
   if (with_norms)
   {
      // the initial residual, or f itself with a zero tolerance
      if (tol > 0.0) { op.residual(); resnorm = op.residual_norm(); }
      else { resnorm = op.rhs_norm(); }
      if (resnorm != 0.) { ieee_check = resnorm / resnorm; }
      if (ieee_check != ieee_check)
      {
         if (print_level > 0)
         {
            printf("\n\nERROR detected by Hypre ...  BEGIN\nERROR -- hypre_ILUSolve: INFs and/or NaNs detected in input.\n"
                   "User probably placed non-numerics in supplied A, x_0, or b.\nERROR detected by Hypre ...  END\n\n\n");
         }
         hypre_error(HYPRE_ERROR_GENERIC);
         return hypre_error_flag;
      }
      init_resnorm = resnorm;
      rhs_norm = op.rhs_norm();
      if (rhs_norm > DBL_EPSILON) { rel_resnorm = init_resnorm / rhs_norm; }
      else
      {
         // a zero right-hand side: the zero solution
         op.zero_u();
         if (logging > 0) { d->final_rel_residual_norm = 0.0; }
         return hypre_error_flag;
      }
   }
   else { rel_resnorm = 1.; }
   if (print)
   {
      printf("                                            relative\n               residual        factor       residual\n"
             "               --------        ------       --------\n    Initial    %e                 %e\n", init_resnorm, rel_resnorm);
   }
   // always one iteration
   while ((rel_resnorm >= tol || iter < 1) && iter < max_iter)
   {
      op.apply();
      if (with_norms)
      {
         old_resnorm = resnorm;
         op.residual();
         resnorm = op.residual_norm();
         conv_factor = old_resnorm ? resnorm / old_resnorm : resnorm;
         rel_resnorm = rhs_norm > DBL_EPSILON ? resnorm / rhs_norm : resnorm;
         d->norms.push_back(rel_resnorm);
      }
      ++iter;
      d->num_iterations = iter;
      d->final_rel_residual_norm = rel_resnorm;
      if (print) { printf("    ILUSolve %2d   %e    %f     %e \n", (int) iter, resnorm, conv_factor, rel_resnorm); }
   }
   const bool missed = iter == max_iter && tol > 0.;
   if (missed) { hypre_error(HYPRE_ERROR_CONV); }
   if (print)
   {
      conv_factor = (iter > 0 && init_resnorm) ? std::pow(resnorm / init_resnorm, 1.0 / (HYPRE_Real) iter) : 1.;
      if (missed)
      {
         printf("\n\n==============================================\n NOTE: Convergence tolerance was not achieved\n"
                "      within the allowed %d iterations\n==============================================", (int) max_iter);
      }
      printf("\n\n Average Convergence Factor = %f \n                operator = %f\n", conv_factor, d->operator_complexity);
   }
   return hypre_error_flag;
}

extern "C" {

// The two triangular solves alone, without the product with A: u += (L D^-1 U)^-1 f, on the device or on the host as f and
// u lie.  For tests that compare the kernels with the host solve bit for bit (the residual product of a Solve has another
// association on the device than on the host).
HYPRE_Int hypre_amd_ILUApplyFactors(HYPRE_Solver solver, HYPRE_ParVector f, HYPRE_ParVector u)
{
   if (refuse_null(solver)) { return hypre_error_flag; }
   hypre_amd_ILUData *d = D(solver);
   if (!f) { hypre_error_in_arg(2); return hypre_error_flag; }
   if (!u) { hypre_error_in_arg(3); return hypre_error_flag; }
   const hypre_Vector *fl = f->local_vector, *ul = u->local_vector;
   const bool device = ul->memory_location == HYPRE_MEMORY_DEVICE;
   if (!d->is_setup || (device && !d->uploaded) || fl->size != d->F.n || ul->size != d->F.n || fl->num_vectors != 1 || ul->num_vectors != 1 ||
       fl->memory_location != ul->memory_location || (d->F.n > 0 && fl->data == ul->data))
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ILUApplyFactors: needs a Setup (for device vectors: with A in device memory, or a device Solve "
                                             "before), and f and u of the factored rows, one column, distinct, in the same memory");
      return hypre_error_flag;
   }
   if (device && d->iterative && !d->iter_uploaded)
   {
      upload_iter(d);
      if (!d->iter_uploaded) { return hypre_error_flag; }
   }
   Ops op{d, nullptr, f, u, device, d->F.n};
   op.apply_factors(fl->data);
   maybe_sync();
   return hypre_error_flag;
}

// the residual f - A u the last application on the device started from (the solver's own vector; NULL before any)
HYPRE_Int hypre_amd_ILUGetResidual(HYPRE_Solver solver, HYPRE_ParVector *residual)
{
   if (refuse_null(solver)) { return hypre_error_flag; }
   if (!residual) { hypre_error_in_arg(2); return hypre_error_flag; }
   *residual = D(solver)->ftemp;
   return hypre_error_flag;
}

// what a solve does and what it works on: levels of the two factors, launches of the last application by kernel form
// (run: one workgroup over consecutive narrow levels; level: a grid for one wide level), entries of the two factors
HYPRE_Int hypre_amd_ILUGetSolveStats(HYPRE_Solver s, HYPRE_Int *levels_L, HYPRE_Int *levels_U, HYPRE_Int *run_launches, HYPRE_Int *level_launches,
                                     HYPRE_Int *nnz_L, HYPRE_Int *nnz_U)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   const hypre_amd_ILUData *d = D(s);
   if (levels_L) { *levels_L = d->is_setup ? d->VL.nlev : 0; }
   if (levels_U) { *levels_U = d->is_setup ? d->VU.nlev : 0; }
   if (run_launches) { *run_launches = d->run_launches; }
   if (level_launches) { *level_launches = d->level_launches; }
   if (nnz_L) { *nnz_L = d->is_setup ? (HYPRE_Int) d->F.Lj.size() : 0; }
   if (nnz_U) { *nnz_U = d->is_setup ? (HYPRE_Int) d->F.Uj.size() : 0; }
   return hypre_error_flag;
}

// the iterative triangular solves as they stand: the switch, the sweeps per factor, the launches of the last application on
// the device (0 after a host one), the entries of the two factors in the slice form, padding included (0 before Setup)
HYPRE_Int hypre_amd_ILUGetIterativeStats(HYPRE_Solver s, HYPRE_Int *iterative, HYPRE_Int *lower_jacobi_iters, HYPRE_Int *upper_jacobi_iters,
                                         HYPRE_Int *launches_per_application, HYPRE_BigInt *padded_nnz_L, HYPRE_BigInt *padded_nnz_U)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   const hypre_amd_ILUData *d = D(s);
   if (iterative) { *iterative = d->iterative; }
   if (lower_jacobi_iters) { *lower_jacobi_iters = d->lower_iters; }
   if (upper_jacobi_iters) { *upper_jacobi_iters = d->upper_iters; }
   if (launches_per_application) { *launches_per_application = d->sweep_launches; }
   if (padded_nnz_L) { *padded_nnz_L = d->is_setup ? (HYPRE_BigInt) d->padded_L : 0; }
   if (padded_nnz_U) { *padded_nnz_U = d->is_setup ? (HYPRE_BigInt) d->padded_U : 0; }
   return hypre_error_flag;
}

// the factors of the last Setup as they lie on the host, in the permuted numbering; the arrays belong to the solver and
// hold until its next Setup or Destroy.  L: unit, strictly lower, columns ascending; U: strictly upper; D: inverse pivots.
HYPRE_Int hypre_amd_ILUGetFactors(HYPRE_Solver s, HYPRE_Int *n, const HYPRE_Int **perm, const HYPRE_Int **L_i, const HYPRE_Int **L_j,
                                  const HYPRE_Real **L_data, const HYPRE_Real **D_inv, const HYPRE_Int **U_i, const HYPRE_Int **U_j,
                                  const HYPRE_Real **U_data)
{
   if (refuse_null(s)) { return hypre_error_flag; }
   const hypre_amd_ILUData *d = D(s);
   if (!d->is_setup)
   {
      hypre_error_w_msg(HYPRE_ERROR_GENERIC, "hypre_amd_ILUGetFactors: call HYPRE_ILUSetup first");
      return hypre_error_flag;
   }
   if (n) { *n = d->F.n; }
   if (perm) { *perm = d->F.perm.data(); }
   if (L_i) { *L_i = d->F.Li.data(); }
   if (L_j) { *L_j = d->F.Lj.data(); }
   if (L_data) { *L_data = d->F.La.data(); }
   if (D_inv) { *D_inv = d->F.D.data(); }
   if (U_i) { *U_i = d->F.Ui.data(); }
   if (U_j) { *U_j = d->F.Uj.data(); }
   if (U_data) { *U_data = d->F.Ua.data(); }
   return hypre_error_flag;
}

// the local reordering on its own: perm[new] = old for the n x n pattern (A_i, A_j) in host memory, as Setup orders a block
HYPRE_Int hypre_amd_ILULocalRCM(HYPRE_Int n, const HYPRE_Int *A_i, const HYPRE_Int *A_j, HYPRE_Int *perm)
{
   if (n < 0) { hypre_error_in_arg(1); return hypre_error_flag; }
   if (n > 0 && (!A_i || !perm)) { hypre_error_in_arg(!A_i ? 2 : 4); return hypre_error_flag; }
   std::vector<int> p;
   ilu::local_rcm(n, A_i, A_j, p);
   for (int i = 0; i < n; i++) { perm[i] = p[(size_t) i]; }
   return hypre_error_flag;
}

}  // extern "C"
