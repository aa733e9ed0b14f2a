// hypre_amd — the iteration of right-preconditioned restarted GMRES with every vector operation behind a callback: the
// Hessenberg matrix, the Givens rotations, the triangular solve and all the decisions live here, on the host, and know
// nothing of where the vectors are.  One loop serves GMRES (krylov/gmres.c:274-908, hypre_GMRESSolve), COGMRES
// (krylov/cogmres.c:278-900, hypre_COGMRESSolve) and FlexGMRES (krylov/flexgmres.c:290-750, hypre_FlexGMRESSolve); what
// tells them apart is a field of GMRESParams, never the name of the caller.  par_gmres.cpp runs it on ParVectors on the
// device; a stand-alone host program can run it on plain arrays (tests/host/gmres_host_check.cpp does, under the address
// and undefined-behaviour sanitizers).
//
// Ops provides, for vector handles V:
//    matvec(alpha, x, beta, y)        y = alpha A x + beta y
//    inner(x, y)                      <x, y>, one scalar on the host
//    copy(x, y)  scale(a, y)  axpy(a, x, y)
//    axpy_dot(a, x, y, z)             y += a x, returns <z, y> of the updated y (z may be y)
//    mass_axpy(a, xs, y, k, unroll)   y += a[0] xs[0], then += a[1] xs[1], ... in that order
//    mass_inner(x, ys, k, unroll, out)               out[j] = <x, ys[j]>
//    mass_dot_two(x, y, zs, k, unroll, outx, outy)   outx[j] = <x, zs[j]>, outy[j] = <y, zs[j]>
//    precond(iter, rel_norm, rhs, sol)  clears sol, lets the caller change the preconditioner, applies it
//    solution_changed(x)
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace hamd {

// how step i makes the new direction p[i] orthogonal to p[0..i-1]
enum class GMRESOrtho
{
   MGS,          // modified Gram-Schmidt: inner then axpy for j = 0..i-1, then the norm (gmres.c:541-547, flexgmres.c:562-573)
   MGS_FUSED,    // the same sums and roundings: one inner, then i axpy_dot, the last giving the squared norm; the
                 // correction of a restart cycle goes through one mass_axpy
   CGS,          // classical Gram-Schmidt, batched: mass_inner, mass_axpy, the norm (cogmres.c:568-577)
   CGS2          // mass_dot_two and the reorthogonalising correction of cogmres.c:550-566, then as CGS
};

struct GMRESParams
{
   int k_dim = 5, min_iter = 0, max_iter = 1000;
   double tol = 1e-6, a_tol = 0.0;
   GMRESOrtho ortho = GMRESOrtho::MGS;
   int unroll = 0;                           // handed to the mass operations
   // true: the preconditioned directions are kept in pre[] and the correction is their sum (flexgmres.c:549-556, 660-665);
   // false: the preconditioner writes into r, the correction is summed from p[] and unwound through the preconditioner
   // once more (gmres.c:538-539, 754-762); pre is not touched and may be null
   bool flexible = false;
   int skip_real_r_check = 0;                // accept the recurrence's norm without recomputing b - A x (gmres.c:769, cogmres.c:778)
   // after a cycle whose recomputed residual is above the tolerance: end with converged = 1 when it did not fall below
   // that of the cycle before (gmres.c:841-850, cogmres.c:843-852); flexgmres.c has no such exit
   bool stop_when_residual_grows = true;
   // a residual of exactly zero returns at once, the reported norm left alone; gmres.c:486-498 and flexgmres.c:495-510
   // store the iteration count on the way, cogmres.c:488-500 does not
   bool count_at_zero_residual = true;
   // gmres.c:903, cogmres.c:896 and flexgmres.c:743 report "not converged" only when epsilon > 0; with this set a run that
   // ends at max_iter above its tolerance is "not converged" also when both tolerances are zero (a fixed number of
   // iterations), so callers of such runs clear the flag
   bool conv_error_at_zero_tol = false;
   // gmres.c:597-615: after every step, give up when the weighted average convergence factor of the recurrence's norm
   // exceeds cf_tol (0: never).  The rule is the caller's (krylov_common.hpp has the one copy PCG and BiCGSTAB use too):
   // cf_exit(factor now, factor one step ago, cf_tol).  The correction of the cycle under way is not added to x.
   double cf_tol = 0.0;
   bool (*cf_exit)(double, double, double) = nullptr;
   // the diagonally scaled phase of the hybrid solver may end at max_iter without "not converged" (gmres.c:901, hybrid == -1)
   bool quiet_at_max_iter = false;
};

enum { GMRES_OK = 0, GMRES_NOT_A_NUMBER = 1, GMRES_NOT_CONVERGED = 2 };

struct GMRESResult
{
   int status = GMRES_OK, iterations = 0, converged = 0;
   bool iterations_set = false;            // false after a not-a-number return, and after the r_norm == 0 return if so asked
   bool norm_set = false;                  // false after either early return, which leave the reported norm alone
   double rel_residual_norm = 0.0;
   long fused_steps = 0, plain_dots = 0, plain_axpys = 0;     // launches of the modified Gram-Schmidt steps
};

// ---- the steps gmres_iterate and lgmres_iterate (lgmres_core.hpp) share: each stands here once, so that the two loops
// cannot drift apart in a rounding or a check

template <class V, class Ops> double krylov_norm(Ops &ops, V v) { return std::sqrt(ops.inner(v, v)); }

// |b - A x|, the residual left in r (gmres.c:776-778, lgmres.c:798-800)
template <class V, class Ops> double true_residual(Ops &ops, V b, V x, V r) { ops.copy(b, r); ops.matvec(-1.0, x, 1.0, r); return krylov_norm(ops, r); }

// b - A x into p0, the norms, the not-a-number checks and the stopping threshold (gmres.c:359-457, cogmres.c:368-459,
// flexgmres.c:372-463, lgmres.c:413-504); after a not-a-number in b the norm of p0 is not taken
struct KrylovStart { double b_norm = 0.0, r_norm = 0.0, den_norm = 0.0, epsilon = 0.0; bool not_a_number = true; };
template <class V, class Ops> KrylovStart krylov_start(Ops &ops, V b, V x, V p0, double tol, double a_tol)
{
   KrylovStart st;
   double ieee_check = 0.;
   ops.copy(b, p0);
   ops.matvec(-1.0, x, 1.0, p0);
   st.b_norm = krylov_norm(ops, b);
   if (st.b_norm != 0.) { ieee_check = st.b_norm / st.b_norm; }
   if (ieee_check != ieee_check) { return st; }
   st.r_norm = krylov_norm(ops, p0);
   if (st.r_norm != 0.) { ieee_check = st.r_norm / st.r_norm; }
   if (ieee_check != ieee_check) { return st; }
   st.not_a_number = false;
   st.den_norm = (st.b_norm > 0.0) ? st.b_norm : st.r_norm;
   st.epsilon = std::max(a_tol, tol * st.den_norm);
   return st;
}

// modified Gram-Schmidt of p[i] against p[0..i-1], the products into h[0..i-1]; returns |p[i]| (gmres.c:541-547,
// flexgmres.c:562-573, lgmres.c:642-647).  fused: the projection on p[j] leaves in the same pass the product with
// p[j + 1], the last one the squared norm; the same sums and roundings as the plain inner / axpy sequence.
template <class V, class Ops> double mgs_step(Ops &ops, V *p, int i, double *h, bool fused, GMRESResult &res)
{
   double t;
   if (fused)
   {
      t = ops.inner(p[0], p[i]);
      res.plain_dots++;
      for (int j = 0; j < i; j++)
      {
         h[j] = t;
         t = ops.axpy_dot(-t, p[j], p[i], j + 1 < i ? p[j + 1] : p[i]);
         res.fused_steps++;
      }
      return std::sqrt(t);
   }
   for (int j = 0; j < i; j++)
   {
      h[j] = ops.inner(p[j], p[i]);
      ops.axpy(-h[j], p[j], p[i]);
   }
   res.plain_dots += i + 1;
   res.plain_axpys += i;
   return krylov_norm(ops, p[i]);
}

// the Hessenberg matrix of a restart cycle of up to `cols` steps, its Givens rotations and the right-hand side rs of the
// least-squares problem; hh(row, col) is hh[col * ld + row].  (Hidden: not a dynamic symbol of a library built from this.)
struct __attribute__((visibility("hidden"))) Hessenberg
{
   size_t ld;
   std::vector<double> hh, rs, c, s;
   explicit Hessenberg(size_t cols) : ld(cols + 1), hh(ld * cols, 0.0), rs(ld, 0.0), c(cols, 0.0), s(cols, 0.0) {}
   double *column(int i) { return &hh[(size_t) (i - 1) * ld]; }      // column i - 1, the one step i fills: h[j] is hh(j, i - 1)
   // the new column's last entry is t = |p[i]|, and p[i] becomes a unit vector unless it is zero; then the rotations so far
   // on the column and the one that clears h[i].  Returns the norm the recurrence gives the residual (gmres.c:548-576,
   // lgmres.c:648-675)
   template <class V, class Ops> double close_column(Ops &ops, V pi, int i, double t)
   {
      const double epsmac = 1.e-16;
      double *h = column(i), gamma;
      h[i] = t;
      if (t != 0.0) { t = 1.0 / t; ops.scale(t, pi); }
      for (int j = 1; j < i; j++)
      {
         t = h[j - 1];
         h[j - 1] = s[j - 1] * h[j] + c[j - 1] * t;
         h[j] = -s[j - 1] * t + c[j - 1] * h[j];
      }
      t = h[i] * h[i];
      t += h[i - 1] * h[i - 1];
      gamma = std::sqrt(t);
      if (gamma == 0.0) { gamma = epsmac; }
      c[i - 1] = h[i - 1] / gamma;
      s[i - 1] = h[i] / gamma;
      rs[i] = -h[i] * rs[i - 1];
      rs[i] /= gamma;
      rs[i - 1] = c[i - 1] * rs[i - 1];
      h[i - 1] = s[i - 1] * h[i] + c[i - 1] * h[i - 1];
      return std::fabs(rs[i]);
   }
   // the upper triangular solve after i steps: rs[0..i-1] become the coefficients of the correction (gmres.c:740-750,
   // lgmres.c:724-734)
   void solve(int i)
   {
      rs[i - 1] = rs[i - 1] / column(i)[i - 1];
      for (int k = i - 2; k >= 0; k--)
      {
         double t = 0.0;
         for (int j = k + 1; j < i; j++) { t -= hh[(size_t) j * ld + (size_t) k] * rs[j]; }
         t += rs[k];
         rs[k] = t / hh[(size_t) k * ld + (size_t) k];
      }
   }
};

// residual vector of the restart into p[0]: rs[0..i] become its coefficients in p[0..i], then the sum (gmres.c:864-880,
// cogmres.c:864-881, flexgmres.c:707-723, lgmres.c:830-846); nothing to do after a restart from the true residual (i == 0)
template <class V, class Ops> void restart_residual(Ops &ops, V *p, int i, Hessenberg &H)
{
   std::vector<double> &rs = H.rs;
   for (int j = i; j > 0; j--)
   {
      rs[j - 1] = -H.s[j - 1] * rs[j];
      rs[j] = H.c[j - 1] * rs[j];
   }
   if (!i) { return; }
   ops.axpy(rs[i] - 1.0, p[i], p[i]);
   for (int j = i - 1; j > 0; j--) { ops.axpy(rs[j], p[j], p[i]); }
   ops.axpy(rs[0] - 1.0, p[0], p[0]);
   ops.axpy(1.0, p[i], p[0]);
}

// what a solve that ran its loop reports (gmres.c:903, cogmres.c:896, flexgmres.c:743, lgmres.c:918; see GMRESParams)
inline void krylov_finish(GMRESResult &res, int iter, double r_norm, double b_norm, double epsilon, int max_iter, bool conv_error_at_zero_tol)
{
   res.iterations = iter;
   res.iterations_set = res.norm_set = true;
   res.rel_residual_norm = (b_norm > 0.0) ? r_norm / b_norm : r_norm;
   if (iter >= max_iter && r_norm > epsilon && (epsilon > 0 || conv_error_at_zero_tol)) { res.status = GMRES_NOT_CONVERGED; }
}

// p (and pre, if flexible) hold k_dim + 1 vectors; r and w are work vectors
template <class V, class Ops>
GMRESResult gmres_iterate(const GMRESParams &prm, Ops &ops, V b, V x, V r, V w, V *p, V *pre)
{
   GMRESResult res;
   const int k_dim = prm.k_dim, min_iter = prm.min_iter, max_iter = prm.max_iter, unroll = prm.unroll;
   Hessenberg H((size_t) k_dim);
   std::vector<double> &rs = H.rs;
   const size_t ld = H.ld;
   std::vector<double> coef((size_t) k_dim, 0.0), rv((size_t) k_dim, 0.0), uu(prm.ortho == GMRESOrtho::CGS2 ? ld * (size_t) k_dim : 0, 0.0);
   std::vector<V> terms((size_t) k_dim);
   V *dir = prm.flexible ? pre : p;                  // what the correction is summed from
   int i = 0, j, k, iter = 0;

   const KrylovStart st = krylov_start(ops, b, x, p[0], prm.tol, prm.a_tol);
   if (st.not_a_number) { res.status = GMRES_NOT_A_NUMBER; return res; }
   const double b_norm = st.b_norm, den_norm = st.den_norm, epsilon = st.epsilon;
   double t, r_norm = st.r_norm, real_r_norm_old = b_norm, cf_ave_0 = 0.0, cf_ave_1 = 0.0;
   const double r_norm_0 = st.r_norm;
   const bool watch_cf = prm.cf_tol > 0.0 && prm.cf_exit;
   bool gave_up = false;

   while (iter < max_iter)
   {
      rs[0] = r_norm;
      if (r_norm == 0.0)
      {
         res.iterations = iter;
         res.iterations_set = prm.count_at_zero_residual;
         return res;
      }
      if (r_norm <= epsilon && iter >= min_iter)
      {
         r_norm = true_residual(ops, b, x, r);
         if (r_norm <= epsilon) { break; }
      }
      t = 1.0 / r_norm;
      ops.scale(t, p[0]);
      i = 0;
      while (i < k_dim && iter < max_iter)
      {
         i++;
         iter++;
         double *h = H.column(i);
         V Ap = prm.flexible ? pre[i - 1] : r;
         ops.precond(iter, r_norm / den_norm, p[i - 1], Ap);
         ops.matvec(1.0, Ap, 0.0, p[i]);
         switch (prm.ortho)
         {
            case GMRESOrtho::MGS_FUSED:
            case GMRESOrtho::MGS:
               t = mgs_step(ops, p, i, h, prm.ortho == GMRESOrtho::MGS_FUSED, res);
               break;
            case GMRESOrtho::CGS2:
            {
               double *u = &uu[(size_t) (i - 1) * ld];        // u[j] = <p[i - 1], p[j]>: column i - 1 of the symmetric uu
               ops.mass_dot_two(p[i], p[i - 1], p, i, unroll, h, u);
               for (j = 0; j < i - 1; j++) { uu[(size_t) j * ld + (size_t) i - 1] = u[j]; }
               for (j = 0; j < i; j++) { rv[j] = h[j]; }
               for (k = 0; k < i; k++)
               {
                  for (j = 0; j < i; j++) { h[j] -= (uu[(size_t) k * ld + (size_t) j] * rv[j]); }
               }
               for (j = 0; j < i; j++) { h[j] = -rv[j] - h[j]; }
               ops.mass_axpy(h, p, p[i], i, unroll);
               for (j = 0; j < i; j++) { h[j] = -h[j]; }
               t = krylov_norm(ops, p[i]);
               break;
            }
            case GMRESOrtho::CGS:
               ops.mass_inner(p[i], p, i, unroll, h);
               for (j = 0; j < i; j++) { h[j] = -h[j]; }
               ops.mass_axpy(h, p, p[i], i, unroll);
               for (j = 0; j < i; j++) { h[j] = -h[j]; }
               t = krylov_norm(ops, p[i]);
               break;
         }
         r_norm = H.close_column(ops, p[i], i, t);
         if (watch_cf)
         {
            cf_ave_0 = cf_ave_1;
            cf_ave_1 = std::pow(r_norm / r_norm_0, 1.0 / (2.0 * iter));
            if (prm.cf_exit(cf_ave_1, cf_ave_0, prm.cf_tol)) { gave_up = true; break; }
         }
         if (r_norm <= epsilon && iter >= min_iter) { break; }
      }
      if (gave_up) { break; }
      H.solve(i);
      // the correction, last direction first
      ops.copy(dir[i - 1], w);
      ops.scale(rs[i - 1], w);
      if (prm.ortho == GMRESOrtho::MGS_FUSED)
      {
         for (j = i - 2, k = 0; j >= 0; j--, k++) { coef[k] = rs[j]; terms[k] = dir[j]; }
         if (k) { ops.mass_axpy(coef.data(), terms.data(), w, k, unroll); }
      }
      else
      {
         for (j = i - 2; j >= 0; j--) { ops.axpy(rs[j], dir[j], w); }
      }
      if (prm.flexible) { ops.axpy(1.0, w, x); }          // summed from the preconditioned vectors: nothing to unwind
      else
      {
         ops.precond(iter, r_norm / den_norm, w, r);
         ops.axpy(1.0, r, x);
      }
      ops.solution_changed(x);
      if (r_norm <= epsilon && iter >= min_iter)
      {
         if (prm.skip_real_r_check) { res.converged = 1; break; }
         r_norm = true_residual(ops, b, x, r);
         if (r_norm <= epsilon) { res.converged = 1; break; }
         if (prm.stop_when_residual_grows)
         {
            if (r_norm >= real_r_norm_old) { res.converged = 1; break; }
            real_r_norm_old = r_norm;
         }
         ops.copy(r, p[0]);             // "false convergence 2" (gmres.c:855-859, flexgmres.c:695-703): restart from the true residual
         i = 0;
      }
      restart_residual(ops, p, i, H);
   }
   krylov_finish(res, iter, r_norm, b_norm, epsilon, max_iter, prm.conv_error_at_zero_tol);
   if (prm.quiet_at_max_iter && res.status == GMRES_NOT_CONVERGED) { res.status = GMRES_OK; }
   return res;
}

}  // namespace hamd
