// hypre_amd — the iteration of LGMRES (krylov/lgmres.c:326-934, hypre_LGMRESSolve; Baker, Jessup, Manteuffel, "A technique
// for accelerating the convergence of restarted GMRES", 2005): right-preconditioned restarted GMRES whose restart cycle of
// k_dim steps ends in up to aug_dim steps that are not Arnoldi steps but bring back the corrections of the cycles before
// (the augmentation vectors z_j, kept with A z_j, so they cost no matrix and no preconditioner application).  A sibling of
// gmres_iterate (gmres_core.hpp) in the same style: every vector operation is a callback, and the Arnoldi-or-augmentation
// decision, the order of the augmentation vectors and every exit live here, on the host.  It is a loop of its own because
// it_arnoldi, it_aug and aug_ct thread through the whole cycle, the correction and the restart included.  The steps that
// are the same arithmetic in both loops (the start-up, the modified Gram-Schmidt step, the Hessenberg column and its
// rotation, the triangular solve, the residual vector of the restart, the closing of the result) are the functions of
// gmres_core.hpp, called from both.  par_gmres.cpp runs it on ParVectors on the device,
// tests/host/lgmres_host_check.cpp on plain arrays under the sanitizers.
//
// What lgmres.c does differently from gmres.c, kept: no "residual did not fall" exit after a false convergence (:812-820);
// the new augmentation vector is the correction w before the preconditioner is unwound (:784); a residual of exactly
// zero returns at once and stores neither count nor norm (:545-558); "not converged" only when epsilon > 0 (:918).  The
// relative-change and convergence-factor exits (rel_change, cf_tol) are not carried, as for the other three.
//
// Ops provides what gmres_iterate asks for (matvec, inner, copy, scale, axpy, axpy_dot, mass_axpy, precond,
// solution_changed; see gmres_core.hpp) and, used only when LGMRESParams::fused is set:
//    scaled_copy(a, x, y)      y = a x                    the bits of copy(x, y); scale(a, y)
//    copy_norm2(x, y)          y = x, returns <x, x>      the bits of copy(x, y); inner(y, y)
//    scaled_diff(a, x, y, z)   z = a (x - y)              the bits of copy(x, z); scale(-1, z); axpy(1, y, z); scale(-a, z)
#pragma once
#include "gmres_core.hpp"

namespace hamd {

// k_dim, min_iter, max_iter, tol, a_tol and unroll (handed to mass_axpy) are those of GMRESParams; its other switches
// (ortho, flexible, skip_real_r_check, stop_when_residual_grows, count_at_zero_residual, conv_error_at_zero_tol) are not
// read by lgmres_iterate, whose behaviour in their place is the list above
struct LGMRESParams : GMRESParams
{
   // hypre_LGMRESCreate (lgmres.c:83-105)
   LGMRESParams() { k_dim = 20; }
   int aug_dim = 2;
   // 1: a cycle has k_dim steps also while fewer than aug_dim augmentation vectors exist (more Arnoldi steps make up for
   // them); 0: always k_dim - aug_dim Arnoldi steps (lgmres.c:593-600)
   int approx_constant = 1;
   // true: Gram-Schmidt through axpy_dot, the correction through scaled_copy and one mass_axpy, the end of a cycle through
   // scaled_copy, copy_norm2 and scaled_diff; false: the reference's sequence of copy / scale / inner / axpy calls.  The
   // same roundings in the same order either way.
   bool fused = true;
};

struct LGMRESResult : GMRESResult
{
   // what forms the correction and ends a restart cycle: launches of scaled_copy / copy_norm2 / scaled_diff, and the
   // copy / scale / inner / axpy calls of the reference in their place.  A cycle that restarts counts (5, 0) fused and
   // (0, 12) plain when aug_dim > 0; the last cycle of a converged solve (2, 0) and (0, 3).
   long fused_updates = 0, plain_updates = 0;
};

// p holds k_dim + 1 vectors, aug aug_dim + 1 (the last one a temporary), a_aug aug_dim; r and w are work vectors
template <class V, class Ops>
LGMRESResult lgmres_iterate(const LGMRESParams &prm, Ops &ops, V b, V x, V r, V w, V *p, V *aug, V *a_aug)
{
   LGMRESResult res;
   const int k_dim = prm.k_dim, aug_dim = prm.aug_dim, min_iter = prm.min_iter, max_iter = prm.max_iter;
   const size_t cols = (size_t) k_dim + (size_t) aug_dim;
   Hessenberg H(cols);
   std::vector<double> &rs = H.rs;
   std::vector<double> coef(cols, 0.0);
   std::vector<V> terms(cols);
   std::vector<int> aug_order((size_t) aug_dim, 0);     // aug_order[spot]: how many cycles ago aug[spot] was the correction
   int i = 0, j, k, ii, iter = 0, aug_ct = 0, spot = 0, it_arnoldi, it_total, it_aug, first;
   // the first slot whose vector is `order` cycles old; before aug_ct reaches aug_dim the unused slots hold duplicates
   auto slot_of = [&](int order) { for (int q = 0; q < aug_dim; q++) { if (aug_order[(size_t) q] == order) { spot = q; break; } } return spot; };

   const KrylovStart st = krylov_start(ops, b, x, p[0], prm.tol, prm.a_tol);
   if (st.not_a_number) { res.status = GMRES_NOT_A_NUMBER; return res; }
   const double b_norm = st.b_norm, den_norm = st.den_norm, epsilon = st.epsilon;
   double t, r_norm = st.r_norm, r_norm_last, tmp_norm, w_squared = 0.0;

   while (iter < max_iter)
   {
      rs[0] = r_norm;
      if (r_norm == 0.0) { res.iterations = iter; return res; }
      if (r_norm <= epsilon && iter >= min_iter)
      {
         r_norm = true_residual(ops, b, x, r);
         if (r_norm <= epsilon) { break; }
      }
      t = 1.0 / r_norm;
      r_norm_last = r_norm;
      ops.scale(t, p[0]);
      i = 0;
      it_arnoldi = prm.approx_constant ? k_dim - aug_ct : k_dim - aug_dim;
      it_total = it_arnoldi + aug_ct;
      it_aug = 0;
      while (i < it_total && iter < max_iter)
      {
         i++;
         iter++;
         if (i <= it_arnoldi)
         {
            ops.precond(iter, r_norm / den_norm, p[i - 1], r);
            ops.matvec(1.0, r, 0.0, p[i]);
         }
         else
         {
            // augmentation step: A z of the vector that is i - it_arnoldi - 1 cycles old stands in for the product
            it_aug++;
            ops.copy(a_aug[slot_of(i - it_arnoldi - 1)], p[i]);
         }
         t = mgs_step(ops, p, i, H.column(i), prm.fused, res);
         r_norm = H.close_column(ops, p[i], i, t);
         if (r_norm <= epsilon && iter >= min_iter) { break; }
      }
      H.solve(i);
      if (it_arnoldi > i) { it_arnoldi = i; }             // the cycle ended before all its Arnoldi steps
      // the correction w (lgmres.c:746-780): without augmentation steps the last direction first, as GMRES sums it; with
      // them p[0] first, the other Arnoldi directions upwards, then the augmentation vectors from the newest
      k = 0;
      if (!it_aug)
      {
         first = i - 1;
         for (j = i - 2; j >= 0; j--, k++) { coef[k] = rs[j]; terms[k] = p[j]; }
      }
      else
      {
         first = 0;
         for (j = 1; j < it_arnoldi; j++, k++) { coef[k] = rs[j]; terms[k] = p[j]; }
         for (ii = 0; ii < it_aug; ii++, k++) { coef[k] = rs[it_arnoldi + ii]; terms[k] = aug[slot_of(ii)]; }
      }
      if (prm.fused)
      {
         ops.scaled_copy(rs[first], p[first], w);
         res.fused_updates++;
         if (k) { ops.mass_axpy(coef.data(), terms.data(), w, k, prm.unroll); }
      }
      else
      {
         ops.copy(p[first], w);
         ops.scale(rs[first], w);
         res.plain_updates += 2;
         for (j = 0; j < k; j++) { ops.axpy(coef[j], terms[j], w); }
      }
      // the next augmentation vector is w, before the preconditioner is unwound; its squared norm is taken along when
      // it will be asked for
      if (prm.fused && aug_dim > 0) { w_squared = ops.copy_norm2(w, aug[aug_dim]); res.fused_updates++; }
      else { ops.copy(w, aug[aug_dim]); res.plain_updates++; }
      ops.precond(iter, r_norm / den_norm, w, r);
      ops.axpy(1.0, r, x);
      ops.solution_changed(x);
      if (r_norm <= epsilon && iter >= min_iter)
      {
         r_norm = true_residual(ops, b, x, r);
         if (r_norm <= epsilon) { res.converged = 1; break; }
         ops.copy(r, p[0]);             // "false convergence 2": restart from the true residual
         i = 0;
      }
      // r0, not scaled, into w (lgmres.c:826-827); then the residual vector of the restart into p[0] as GMRES forms it
      if (prm.fused) { ops.scaled_copy(r_norm_last, p[0], w); res.fused_updates++; }
      else { ops.copy(p[0], w); ops.scale(r_norm_last, w); res.plain_updates += 2; }
      restart_residual(ops, p, i, H);
      if (aug_dim > 0)
      {
         // where the new vector goes (lgmres.c:852-874): the next free slot, or that of the oldest one
         if (aug_ct < aug_dim) { spot = aug_ct; aug_ct++; }
         else
         {
            for (ii = 0; ii < aug_dim; ii++) { if (aug_order[(size_t) ii] == aug_dim - 1) { spot = ii; } }
         }
         // z = w / |w|
         if (prm.fused)
         {
            tmp_norm = 1.0 / std::sqrt(w_squared);
            ops.scaled_copy(tmp_norm, aug[aug_dim], aug[spot]);
            res.fused_updates++;
         }
         else
         {
            ops.copy(aug[aug_dim], aug[spot]);
            tmp_norm = 1.0 / krylov_norm(ops, aug[spot]);
            ops.scale(tmp_norm, aug[spot]);
            res.plain_updates += 3;
         }
         for (ii = 0; ii < aug_dim; ii++) { aug_order[(size_t) ii]++; }
         aug_order[(size_t) spot] = 0;
         // A z = (r0 - r_m) / |w|: r0 is in w, the new residual in p[0]; needs neither matrix nor preconditioner
         if (prm.fused) { ops.scaled_diff(tmp_norm, w, p[0], a_aug[spot]); res.fused_updates++; }
         else
         {
            ops.copy(w, a_aug[spot]);
            ops.scale(-1.0, a_aug[spot]);
            ops.axpy(1.0, p[0], a_aug[spot]);
            ops.scale(-tmp_norm, a_aug[spot]);
            res.plain_updates += 4;
         }
      }
   }
   krylov_finish(res, iter, r_norm, b_norm, epsilon, max_iter, false);       // lgmres.c:918: only when epsilon > 0
   return res;
}

}  // namespace hamd
