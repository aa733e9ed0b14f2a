// Stand-alone host check of the LGMRES iteration (hypre_amd/csrc/lgmres_core.hpp): the Hessenberg / Givens logic, the
// Arnoldi-or-augmentation decision, the order of the augmentation vectors and the restart, with plain arrays behind the
// vector callbacks, on dense systems of 60 unknowns (one symmetric positive definite, one not symmetric) behind a Jacobi
// preconditioner.  Meant to be built with
//    c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I hypre_amd/csrc
// and run once (tests/test_lgmres_host.py does): any index past hh / rs / c / s / coef / terms / aug_order or past the
// k_dim + 1 basis vectors, the aug_dim + 1 augmentation vectors and the aug_dim products ends the program.  It also checks
// what it computes: k_dim 2 with aug_dim 1; k_dim 5 with aug_dim 2 over more than five cycles (fill phase and truncation);
// approx_constant both ways; fused against plain, bit for bit; an iteration limit inside an augmentation step;
// convergence inside the first cycle; a zero right-hand side; a NaN; and aug_dim 0, which is GMRES.
#include "lgmres_core.hpp"
#include "dense_ops.hpp"
#include <string>

struct Run { hamd::LGMRESResult res; Vec x; int arnoldi, cycles, fused_calls; std::uint64_t trace; };

static Run solve(const Vec &A, const Vec &b_in, int n, const hamd::LGMRESParams &prm)
{
   Vec b = b_in, x((size_t) n, 0.0), r((size_t) n), w((size_t) n);
   // exactly as many vectors as Setup gives
   VecPool pool;
   std::vector<Vec *> p = pool.several(prm.k_dim + 1, n), aug = pool.several(prm.aug_dim + 1, n), a_aug = pool.several(prm.aug_dim, n);
   DenseOps ops(n, A);
   ops.w = &w;
   ops.name(&b, DenseOps::B); ops.name(&x, DenseOps::X); ops.name(&r, DenseOps::R); ops.name(&w, DenseOps::W);
   ops.name(p, DenseOps::P); ops.name(aug, DenseOps::AUG); ops.name(a_aug, DenseOps::A_AUG);
   Run out;
   out.res = hamd::lgmres_iterate<Vec *>(prm, ops, &b, &x, &r, &w, p.data(), aug.data(), a_aug.data());
   out.x = x; out.arnoldi = ops.arnoldi; out.cycles = ops.cycles; out.fused_calls = ops.fused_calls;
   out.trace = ops.trace_end(x, out.res, out.res.fused_updates, out.res.plain_updates);
   return out;
}

// iterations that are augmentation steps when nothing cuts a cycle short: cycle c (from 0) has min(c, aug_dim) of them at
// its end (approx_constant or not: the vectors that exist are used)
static int expected_aug_steps(int iterations, const hamd::LGMRESParams &prm)
{
   int steps = 0, done = 0;
   for (int cyc = 0; done < iterations; cyc++)
   {
      const int have = std::min(cyc, prm.aug_dim);
      const int arnoldi = prm.approx_constant ? prm.k_dim - have : prm.k_dim - prm.aug_dim;
      const int len = std::min(arnoldi + have, iterations - done);
      steps += std::max(0, len - arnoldi);
      done += len;
   }
   return steps;
}

int main()
{
   const int n = 60;
   Vec spd((size_t) n * n, 0.0), nonsym((size_t) n * n), b((size_t) n);
   unsigned s = 50510u;
   auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double) (s >> 8) / (double) (1u << 24) - 0.5; };
   for (int i = 0; i < n; i++)
   {
      spd[(size_t) i * n + i] = 2.1 + 0.01 * (i % 7);          // a shifted 1-D Laplacian: restarted GMRES with a short basis is slow on it
      if (i) { spd[(size_t) i * n + i - 1] = spd[(size_t) (i - 1) * n + i] = -1.0; }
      for (int j = 0; j < n; j++) { nonsym[(size_t) i * n + j] = 0.3 * rnd(); }
      nonsym[(size_t) i * n + i] += 4.0 + 0.1 * i;                // not symmetric, diagonally dominant
      b[i] = rnd();
   }
   struct { const char *name; const Vec &A; } systems[] = {{"spd", spd}, {"nonsymmetric", nonsym}};

   for (const auto &sys : systems)
   {
      const Vec &A = sys.A;
      for (int approx = 1; approx >= 0; approx--)
      {
         for (int shape = 0; shape < 2; shape++)
         {
            hamd::LGMRESParams q;
            q.k_dim = shape ? 5 : 2; q.aug_dim = shape ? 2 : 1; q.approx_constant = approx;
            q.tol = 1e-10; q.max_iter = 2000; q.fused = true;
            const Run f = solve(A, b, n, q);
            q.fused = false;
            const Run g = solve(A, b, n, q);
            const double rel = true_rel_residual(A, b, f.x, n);
            std::printf("%-12s k_dim %d aug_dim %d approx_constant %d: %4d iterations in %3d cycles, reported %.6e, recomputed %.6e\n",
                        sys.name, q.k_dim, q.aug_dim, approx, f.res.iterations, f.cycles, f.res.rel_residual_norm, rel);
            CHECK(f.res.status == hamd::GMRES_OK && f.res.converged == 1 && f.res.iterations_set && f.res.norm_set);
            // both are |b - A x| / |b| of the same x, summed in different orders: 60 terms of size |A| |x| each rounded to 1e-16
            CHECK(rel <= 1e-10 && std::fabs(rel - f.res.rel_residual_norm) <= 1e-13);
            // fused and plain: the same bits, and the counters say which ran
            CHECK(g.res.iterations == f.res.iterations && g.res.rel_residual_norm == f.res.rel_residual_norm && g.x == f.x);
            CHECK(g.cycles == f.cycles && g.arnoldi == f.arnoldi);
            CHECK(f.res.plain_updates == 0 && f.res.fused_updates == 5L * (f.cycles - 1) + 2 && f.fused_calls == f.res.fused_updates);
            CHECK(g.res.fused_updates == 0 && g.res.plain_updates == 12L * (g.cycles - 1) + 3 && g.fused_calls == 0);
            CHECK(f.res.fused_steps > 0 && f.res.plain_axpys == 0 && g.res.fused_steps == 0 && g.res.plain_axpys == f.res.fused_steps);
            // augmentation steps cost no preconditioner application: one per Arnoldi step, one more per cycle
            CHECK(f.arnoldi == f.res.iterations - expected_aug_steps(f.res.iterations, q));
            if (&A == &spd)
            {
               CHECK(f.cycles > 5 && f.arnoldi < f.res.iterations);           // past the fill phase (aug_dim cycles) into truncation
               // for the reader, not a check (nothing guarantees it): restarted GMRES with the same basis, aug_dim 0
               hamd::LGMRESParams q0 = q;
               q0.aug_dim = 0;
               const Run plain_gmres = solve(A, b, n, q0);
               std::printf("%-12s k_dim %d aug_dim 0:                   %4d iterations\n", sys.name, q0.k_dim, plain_gmres.res.iterations);
               CHECK(plain_gmres.res.converged == 1);
            }
         }
      }

      // aug_dim 0 is GMRES: the iteration count, the norm and the iterate of gmres_iterate with the plain Gram-Schmidt
      {
         hamd::LGMRESParams q;
         q.k_dim = 5; q.aug_dim = 0; q.tol = 1e-10; q.max_iter = 2000; q.fused = false;
         const Run l = solve(A, b, n, q);
         DenseOps gops(n, A);
         hamd::GMRESParams gp;
         gp.k_dim = 5; gp.tol = 1e-10; gp.max_iter = 2000; gp.stop_when_residual_grows = false;
         Vec bb = b, x((size_t) n, 0.0), r((size_t) n), w((size_t) n);
         VecPool pool;
         std::vector<Vec *> p = pool.several(gp.k_dim + 1, n);
         const hamd::GMRESResult gr = hamd::gmres_iterate<Vec *>(gp, gops, &bb, &x, &r, &w, p.data(), (Vec **) nullptr);
         std::printf("%-12s aug_dim 0: %d iterations, GMRES %d\n", sys.name, l.res.iterations, gr.iterations);
         CHECK(l.res.converged == 1 && gr.converged == 1 && l.res.iterations > q.k_dim);
         CHECK(l.res.iterations == gr.iterations && l.res.rel_residual_norm == gr.rel_residual_norm && l.x == x);
         q.fused = true;
         const Run lf = solve(A, b, n, q);
         CHECK(lf.res.iterations == l.res.iterations && lf.x == l.x);
      }

      // the iteration limit inside an augmentation step: with k_dim 5, aug_dim 2 the cycles are 5 | 4 + 1 | 3 + 2 steps, so
      // iteration 14 is the first of the two augmentation steps of the third cycle; 10 is the last step of the second
      for (int limit : {14, 10, 15, 3})
      {
         hamd::LGMRESParams q;
         q.k_dim = 5; q.aug_dim = 2; q.tol = 1e-14; q.max_iter = limit;
         const Run e = solve(A, b, n, q);
         const double rel = true_rel_residual(A, b, e.x, n);
         std::printf("%-12s max_iter %2d: reported %.6e, recomputed %.6e\n", sys.name, limit, e.res.rel_residual_norm, rel);
         CHECK(e.res.iterations == limit && e.res.converged == 0 && e.res.status == hamd::GMRES_NOT_CONVERGED);
         CHECK(e.arnoldi == limit - expected_aug_steps(limit, q) && e.cycles == (limit + 4) / 5);
         CHECK(rel < 1.0 && std::fabs(rel - e.res.rel_residual_norm) <= 1e-13);
         q.fused = false;
         const Run ep = solve(A, b, n, q);
         CHECK(ep.x == e.x && ep.res.rel_residual_norm == e.res.rel_residual_norm);
         // without a tolerance the same end is not an error (lgmres.c:918)
         q.tol = 0.0;
         const Run e0 = solve(A, b, n, q);
         CHECK(e0.res.iterations == limit && e0.res.status == hamd::GMRES_OK && e0.x == e.x);
      }

      // convergence inside the first cycle: no restart, no augmentation vector ever used.  A basis as long as the system:
      // the minimal residual over 59 directions of a system whose preconditioned spectrum lies in [0.05, 2] is below 1e-3
      {
         hamd::LGMRESParams q;
         q.k_dim = n; q.aug_dim = 3; q.tol = 1e-3; q.max_iter = 100;
         const Run e = solve(A, b, n, q);
         CHECK(e.res.converged == 1 && e.res.iterations < q.k_dim && e.cycles == 1 && e.arnoldi == e.res.iterations);
         CHECK(e.res.fused_updates == 2);
         CHECK(true_rel_residual(A, b, e.x, n) <= 1e-3);
      }

      // zero right-hand side, zero guess: returns at once, count and norm left alone; a NaN in b: reported, nothing iterated
      {
         hamd::LGMRESParams q;
         q.k_dim = 5; q.aug_dim = 2;
         const Run z0 = solve(A, Vec((size_t) n, 0.0), n, q);
         CHECK(z0.res.status == hamd::GMRES_OK && z0.res.iterations == 0 && !z0.res.iterations_set && !z0.res.norm_set && z0.arnoldi == 0 && z0.cycles == 0);
         Vec bad = b; bad[3] = std::nan("");
         const Run n0 = solve(A, bad, n, q);
         CHECK(n0.res.status == hamd::GMRES_NOT_A_NUMBER && !n0.res.iterations_set && !n0.res.norm_set && n0.arnoldi == 0);
      }
   }

   // the traces compared with the recorded ones: both systems, fused and plain, aug_dim 0 and 2, approx_constant both ways,
   // and a run that max_iter ends at the first of the two augmentation steps of the third cycle
   for (const auto &sys : systems)
   {
      for (int fused = 1; fused >= 0; fused--)
      {
         hamd::LGMRESParams q;
         q.k_dim = 5; q.tol = 1e-10; q.max_iter = 2000; q.fused = fused != 0;
         for (int aug_dim : {0, 2})
         {
            for (int approx : {0, 1})
            {
               q.aug_dim = aug_dim; q.approx_constant = approx;
               const std::string variant = std::string(fused ? "fused" : "plain") + " aug_dim " + std::to_string(aug_dim) + " approx_constant " + std::to_string(approx);
               print_trace(sys.name, variant.c_str(), solve(sys.A, b, n, q).trace);
            }
         }
         q.tol = 1e-14; q.max_iter = 14;
         print_trace(sys.name, fused ? "fused max_iter 14" : "plain max_iter 14", solve(sys.A, b, n, q).trace);
      }
   }
   std::printf("lgmres host check ok: 2 systems\n");
   return 0;
}
