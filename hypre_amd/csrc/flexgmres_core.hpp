// hypre_amd — the iteration of flexible GMRES (krylov/flexgmres.c:330-760, hypre_FlexGMRESSolve) with every vector
// operation behind a callback: the Hessenberg matrix, the Givens rotations, the triangular solve and all the decisions
// live here, on the host, and know nothing of where the vectors are.  par_flexgmres.cpp runs it on ParVectors on the
// device; a stand-alone host program can run it on plain arrays (tests/host/flexgmres_host_check.cpp does, under the
// address and undefined-behaviour sanitizers).
//
// Ops provides, for vector handles V:
//    matvec(alpha, x, beta, y)        y = alpha A x + beta y
//    inner(x, y)                      <x, y>, one scalar on the host
//    copy(x, y)  scale(a, y)  axpy(a, x, y)
//    axpy_dot(a, x, y, z)             y += a x, returns <z, y> of the updated y (z may be y)
//    mass_axpy(a, xs, y, k)           y += a[0] xs[0], then += a[1] xs[1], ... in that order
//    precond(iter, rel_norm, rhs, sol)  clears sol, lets the caller change the preconditioner, applies it
//    solution_changed(x)
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace hamd {

struct FlexGMRESParams
{
   int k_dim = 20, min_iter = 0, max_iter = 1000;
   double tol = 1e-6, a_tol = 0.0;
   int fused = 1;          // 1: Gram-Schmidt steps through axpy_dot, the correction through mass_axpy; 0: inner / axpy only
};

enum { FLEXGMRES_OK = 0, FLEXGMRES_NOT_A_NUMBER = 1, FLEXGMRES_NOT_CONVERGED = 2 };

struct FlexGMRESResult
{
   int status = FLEXGMRES_OK, iterations = 0, converged = 0;
   bool norm_set = false;                  // false after the r_norm == 0 return, which leaves the reported norm alone
   double rel_residual_norm = 0.0;
   long fused_steps = 0, plain_dots = 0, plain_axpys = 0;     // launches of the Gram-Schmidt steps
};

// p and pre hold k_dim + 1 vectors each; r and w are work vectors
template <class V, class Ops>
FlexGMRESResult flexgmres_iterate(const FlexGMRESParams &prm, Ops &ops, V b, V x, V r, V w, V *p, V *pre)
{
   FlexGMRESResult res;
   const int k_dim = prm.k_dim, min_iter = prm.min_iter, max_iter = prm.max_iter;
   const double epsmac = 1.e-16;
   std::vector<double> rs((size_t) k_dim + 1, 0.0), c((size_t) k_dim, 0.0), s((size_t) k_dim, 0.0), coef((size_t) k_dim, 0.0);
   std::vector<std::vector<double>> hh((size_t) k_dim + 1, std::vector<double>((size_t) k_dim, 0.0));
   std::vector<V> terms((size_t) k_dim);
   int i = 0, j, k, iter = 0;
   double t, gamma, r_norm, b_norm, den_norm, epsilon, ieee_check = 0.;
   auto norm = [&](V v) { return std::sqrt(ops.inner(v, v)); };

   ops.copy(b, p[0]);
   ops.matvec(-1.0, x, 1.0, p[0]);
   b_norm = norm(b);
   if (b_norm != 0.) { ieee_check = b_norm / b_norm; }
   if (ieee_check != ieee_check) { res.status = FLEXGMRES_NOT_A_NUMBER; return res; }
   r_norm = norm(p[0]);
   if (r_norm != 0.) { ieee_check = r_norm / r_norm; }
   if (ieee_check != ieee_check) { res.status = FLEXGMRES_NOT_A_NUMBER; return res; }
   den_norm = (b_norm > 0.0) ? b_norm : r_norm;
   epsilon = std::max(prm.a_tol, prm.tol * den_norm);

   while (iter < max_iter)
   {
      rs[0] = r_norm;
      if (r_norm == 0.0) { res.iterations = iter; return res; }      // flexgmres.c:495-510
      if (r_norm <= epsilon && iter >= min_iter)
      {
         ops.copy(b, r);
         ops.matvec(-1.0, x, 1.0, r);
         r_norm = norm(r);
         if (r_norm <= epsilon) { break; }
      }
      t = 1.0 / r_norm;
      ops.scale(t, p[0]);
      i = 0;
      while (i < k_dim && iter < max_iter)
      {
         i++;
         iter++;
         ops.precond(iter, r_norm / den_norm, p[i - 1], pre[i - 1]);        // flexgmres.c:549-556
         ops.matvec(1.0, pre[i - 1], 0.0, p[i]);
         // modified Gram-Schmidt (flexgmres.c:562-573)
         if (prm.fused)
         {
            // the projection on p[j] leaves in the same pass the product with p[j + 1], the last one the squared norm
            t = ops.inner(p[0], p[i]);
            res.plain_dots++;
            for (j = 0; j < i; j++)
            {
               hh[j][i - 1] = t;
               t = ops.axpy_dot(-t, p[j], p[i], j + 1 < i ? p[j + 1] : p[i]);
               res.fused_steps++;
            }
            t = std::sqrt(t);
         }
         else
         {
            for (j = 0; j < i; j++)
            {
               hh[j][i - 1] = ops.inner(p[j], p[i]);
               ops.axpy(-hh[j][i - 1], p[j], p[i]);
            }
            t = norm(p[i]);
            res.plain_dots += i + 1;
            res.plain_axpys += i;
         }
         hh[i][i - 1] = t;
         if (t != 0.0) { t = 1.0 / t; ops.scale(t, p[i]); }
         for (j = 1; j < i; j++)
         {
            t = hh[j - 1][i - 1];
            hh[j - 1][i - 1] = s[j - 1] * hh[j][i - 1] + c[j - 1] * t;
            hh[j][i - 1] = -s[j - 1] * t + c[j - 1] * hh[j][i - 1];
         }
         t = hh[i][i - 1] * hh[i][i - 1];
         t += hh[i - 1][i - 1] * hh[i - 1][i - 1];
         gamma = std::sqrt(t);
         if (gamma == 0.0) { gamma = epsmac; }
         c[i - 1] = hh[i - 1][i - 1] / gamma;
         s[i - 1] = hh[i][i - 1] / gamma;
         rs[i] = -hh[i][i - 1] * rs[i - 1];
         rs[i] /= gamma;
         rs[i - 1] = c[i - 1] * rs[i - 1];
         hh[i - 1][i - 1] = s[i - 1] * hh[i][i - 1] + c[i - 1] * hh[i - 1][i - 1];
         r_norm = std::fabs(rs[i]);
         if (r_norm <= epsilon && iter >= min_iter) { break; }
      }
      // upper triangular solve
      rs[i - 1] = rs[i - 1] / hh[i - 1][i - 1];
      for (k = i - 2; k >= 0; k--)
      {
         t = 0.0;
         for (j = k + 1; j < i; j++) { t -= hh[k][j] * rs[j]; }
         t += rs[k];
         rs[k] = t / hh[k][k];
      }
      // the correction from the stored preconditioned vectors, last one first (flexgmres.c:660-665); nothing to unwind
      ops.copy(pre[i - 1], w);
      ops.scale(rs[i - 1], w);
      if (prm.fused)
      {
         for (j = i - 2, k = 0; j >= 0; j--, k++) { coef[k] = rs[j]; terms[k] = pre[j]; }
         if (k) { ops.mass_axpy(coef.data(), terms.data(), w, k); }
      }
      else
      {
         for (j = i - 2; j >= 0; j--) { ops.axpy(rs[j], pre[j], w); }
      }
      ops.axpy(1.0, w, x);
      ops.solution_changed(x);
      if (r_norm <= epsilon && iter >= min_iter)
      {
         ops.copy(b, r);
         ops.matvec(-1.0, x, 1.0, r);
         r_norm = norm(r);
         if (r_norm <= epsilon) { res.converged = 1; break; }
         ops.copy(r, p[0]);             // "false convergence 2" (flexgmres.c:695-703): restart from the true residual
         i = 0;
      }
      // residual vector of the restart (flexgmres.c:707-723)
      for (j = i; j > 0; j--)
      {
         rs[j - 1] = -s[j - 1] * rs[j];
         rs[j] = c[j - 1] * rs[j];
      }
      if (i) { ops.axpy(rs[i] - 1.0, p[i], p[i]); }
      for (j = i - 1; j > 0; j--) { ops.axpy(rs[j], p[j], p[i]); }
      if (i)
      {
         ops.axpy(rs[0] - 1.0, p[0], p[0]);
         ops.axpy(1.0, p[i], p[0]);
      }
   }
   res.iterations = iter;
   res.norm_set = true;
   res.rel_residual_norm = (b_norm > 0.0) ? r_norm / b_norm : r_norm;
   // flexgmres.c:743 reports this only when epsilon > 0; here a run that ends at max_iter above its tolerance is "not
   // converged" also when both tolerances are zero (a fixed number of iterations), so callers of such runs clear the flag
   if (iter >= max_iter && r_norm > epsilon) { res.status = FLEXGMRES_NOT_CONVERGED; }
   return res;
}

}  // namespace hamd
