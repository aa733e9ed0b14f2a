// Stand-alone host check of the restarted-GMRES iteration (hypre_amd/csrc/gmres_core.hpp): the Hessenberg / Givens /
// restart logic that par_gmres.cpp runs for GMRES, COGMRES and FlexGMRES, with plain arrays behind the vector callbacks,
// on a dense non-symmetric system of 50 unknowns.  Meant to be built with
//    c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I hypre_amd/csrc
// and run once (tests/test_gmres_host.py does): any out-of-bounds index into hh / uu / rv / rs / c / s, the basis arrays
// or the coefficient lists of the batched operations ends the program.  It also checks what it computes, for every
// combination of flexible / not and Gram-Schmidt variant that an entry point uses: convergence across several restarts,
// the true residual, the same bits with the fused and the plain Gram-Schmidt, the basis of one vector, a cycle cut short,
// the "not converged" end, the zero right-hand side, a NaN, the exit on a residual that stopped falling, and for the
// flexible variant the modify_pc protocol with a preconditioner that changes every iteration.
#include "gmres_core.hpp"
#include "dense_ops.hpp"

using hamd::GMRESOrtho;

struct Run { hamd::GMRESResult res; Vec x; int calls; bool in_order; std::uint64_t trace; };

static Run solve(const Vec &A, const Vec &b_in, int n, const hamd::GMRESParams &prm, int wrong_from = 0)
{
   Vec b = b_in, x((size_t) n, 0.0), r((size_t) n), w((size_t) n);
   // exactly k_dim + 1 vectors each; a solver that is not flexible gets no pre at all
   VecPool pool;
   std::vector<Vec *> p = pool.several(prm.k_dim + 1, n), z = pool.several(prm.flexible ? prm.k_dim + 1 : 0, n);
   DenseOps ops(n, A);
   ops.k_dim = prm.k_dim; ops.vary = prm.flexible; ops.wrong_from = wrong_from;
   ops.name(&b, DenseOps::B); ops.name(&x, DenseOps::X); ops.name(&r, DenseOps::R); ops.name(&w, DenseOps::W);
   ops.name(p, DenseOps::P); ops.name(z, DenseOps::PRE);
   Run out;
   out.res = hamd::gmres_iterate<Vec *>(prm, ops, &b, &x, &r, &w, p.data(), prm.flexible ? z.data() : nullptr);
   out.x = x; out.calls = ops.calls; out.in_order = ops.rel_in_order; out.trace = ops.trace_end(x, out.res);
   return out;
}

// the parameters the three Create functions of par_gmres.cpp fill in, and the one combination no entry point uses yet
struct Config { const char *name; bool flexible; GMRESOrtho ortho; };
static const Config configs[] = {
   {"gmres, plain mgs", false, GMRESOrtho::MGS},
   {"cogmres, cgs 1", false, GMRESOrtho::CGS},
   {"cogmres, cgs 2", false, GMRESOrtho::CGS2},
   {"flexgmres, fused mgs", true, GMRESOrtho::MGS_FUSED},
   {"flexgmres, plain mgs", true, GMRESOrtho::MGS},
};
static hamd::GMRESParams params(const Config &cf)
{
   hamd::GMRESParams prm;
   prm.flexible = cf.flexible;
   prm.ortho = cf.ortho;
   prm.stop_when_residual_grows = !cf.flexible;
   prm.conv_error_at_zero_tol = cf.flexible;
   prm.count_at_zero_residual = !(cf.ortho == GMRESOrtho::CGS || cf.ortho == GMRESOrtho::CGS2);
   return prm;
}

int main()
{
   const int n = 50;
   Vec A((size_t) n * n), b((size_t) n);
   unsigned s = 12345u;
   auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double) (s >> 8) / (double) (1u << 24) - 0.5; };
   for (int i = 0; i < n; i++)
   {
      for (int j = 0; j < n; j++) { A[(size_t) i * n + j] = 0.3 * rnd(); }
      A[(size_t) i * n + i] += 4.0 + 0.1 * i;                  // non-symmetric, diagonally dominant
      b[i] = rnd();
   }
   hamd::GMRESParams prm = params(configs[3]);
   prm.k_dim = 7; prm.tol = 1e-10; prm.max_iter = 200;
   const Run f = solve(A, b, n, prm);
   prm.ortho = GMRESOrtho::MGS;
   const Run g = solve(A, b, n, prm);
   CHECK(f.res.status == hamd::GMRES_OK && f.res.converged == 1 && f.res.norm_set);
   CHECK(f.res.iterations > prm.k_dim);                                            // more than one restart cycle
   CHECK(f.calls == f.res.iterations && f.in_order);
   const double rel = true_rel_residual(A, b, f.x, n);
   std::printf("relative residual: reported %.6e, recomputed %.6e\n", f.res.rel_residual_norm, rel);
   // both are |b - A x| / |b| of the same x, summed in different orders: 50 terms of size |A| |x| each rounded to 1e-16
   CHECK(rel <= 1e-10 && std::fabs(rel - f.res.rel_residual_norm) <= 1e-13);
   // fused and plain: the same bits
   CHECK(g.res.iterations == f.res.iterations && g.res.rel_residual_norm == f.res.rel_residual_norm && g.x == f.x);
   long steps = 0;
   for (int it = 1; it <= f.res.iterations; it++) { steps += (it - 1) % prm.k_dim + 1; }
   CHECK(f.res.fused_steps == steps && f.res.plain_dots == f.res.iterations && f.res.plain_axpys == 0);
   CHECK(g.res.fused_steps == 0 && g.res.plain_dots == steps + g.res.iterations && g.res.plain_axpys == steps);
   // a fixed number of iterations: the full basis (i == k_dim) and a cycle cut short by max_iter
   prm.ortho = GMRESOrtho::MGS_FUSED; prm.tol = 0.0; prm.max_iter = 10;
   const Run h = solve(A, b, n, prm);
   CHECK(h.res.status == hamd::GMRES_NOT_CONVERGED && h.res.iterations == 10 && h.res.converged == 0);
   prm.k_dim = 1; prm.max_iter = 3;
   const Run h1 = solve(A, b, n, prm);
   CHECK(h1.res.iterations == 3);
   // zero right-hand side, zero guess: returns at once
   prm.k_dim = 7; prm.tol = 1e-10; prm.max_iter = 200;
   const Run zr = solve(A, Vec((size_t) n, 0.0), n, prm);
   CHECK(zr.res.status == hamd::GMRES_OK && zr.res.iterations == 0 && !zr.res.norm_set && zr.calls == 0);
   // a NaN in b is reported, nothing is iterated
   Vec bad = b; bad[3] = std::nan("");
   const Run nn = solve(A, bad, n, prm);
   CHECK(nn.res.status == hamd::GMRES_NOT_A_NUMBER && nn.calls == 0);
   std::printf("flexgmres host check ok: %d iterations, relative residual %.3e, %ld fused steps\n", f.res.iterations, rel, steps);

   // every configuration; the preconditioner is fixed for those that are not flexible
   for (const Config &cf : configs)
   {
      hamd::GMRESParams q = params(cf);
      q.k_dim = 7; q.tol = 1e-10; q.max_iter = 200;
      const Run a = solve(A, b, n, q);
      const double ra = true_rel_residual(A, b, a.x, n);
      std::printf("%-22s %3d iterations, reported %.6e, recomputed %.6e\n", cf.name, a.res.iterations, a.res.rel_residual_norm, ra);
      CHECK(a.res.status == hamd::GMRES_OK && a.res.converged == 1 && a.res.iterations_set && a.res.norm_set);
      CHECK(a.res.iterations > q.k_dim);
      CHECK(ra <= 1e-10 && std::fabs(ra - a.res.rel_residual_norm) <= 1e-13);       // the bound derived above
      if (cf.flexible) { CHECK(a.calls == a.res.iterations && a.in_order); }
      else { CHECK(a.calls == a.res.iterations + (a.res.iterations + q.k_dim - 1) / q.k_dim); }   // one unwinding per cycle
      // a basis of one vector
      q.k_dim = 1; q.tol = 0.0; q.max_iter = 3;
      const Run e1 = solve(A, b, n, q);
      CHECK(e1.res.iterations == 3 && e1.res.converged == 0);
      // the full basis, then a cycle cut short at i = 3, where the uu copy of cgs 2 indexes furthest; at tol 0 only the
      // flexible solver calls the end at max_iter "not converged"
      q.k_dim = 7; q.max_iter = 10;
      const Run e2 = solve(A, b, n, q);
      CHECK(e2.res.iterations == 10 && e2.res.converged == 0 && e2.res.norm_set);
      CHECK(e2.res.status == (cf.flexible ? hamd::GMRES_NOT_CONVERGED : hamd::GMRES_OK));
      // zero right-hand side: returns at once, the norm left alone, the count stored or not
      q.tol = 1e-10; q.max_iter = 200;
      const Run z0 = solve(A, Vec((size_t) n, 0.0), n, q);
      CHECK(z0.res.status == hamd::GMRES_OK && z0.res.iterations == 0 && !z0.res.norm_set && z0.calls == 0);
      CHECK(z0.res.iterations_set == q.count_at_zero_residual);
      // a NaN in b: reported, no count, no norm, no preconditioner call
      const Run n0 = solve(A, bad, n, q);
      CHECK(n0.res.status == hamd::GMRES_NOT_A_NUMBER && !n0.res.iterations_set && !n0.res.norm_set && n0.calls == 0);
   }

   // fused against plain where the solver is not flexible: the core allows it, no entry point uses it yet
   {
      hamd::GMRESParams q = params(configs[0]);
      q.k_dim = 7; q.tol = 1e-10; q.max_iter = 200;
      const Run plain = solve(A, b, n, q);
      q.ortho = GMRESOrtho::MGS_FUSED;
      const Run fused = solve(A, b, n, q);
      CHECK(fused.res.iterations == plain.res.iterations && fused.res.rel_residual_norm == plain.res.rel_residual_norm && fused.x == plain.x);
      CHECK(fused.res.converged == 1 && fused.res.fused_steps > 0 && plain.res.fused_steps == 0);
   }

   // The exit on a residual that did not fall (gmres.c:841-850).  From iteration 4 on, in the middle of the first cycle,
   // the preconditioner answers 100 times too large.  The basis and the Hessenberg matrix do not depend on where the
   // correction goes, so both variants claim convergence at the same iteration.  The solver that is not flexible unwinds
   // the whole correction through the changed preconditioner, lands about 100 |b| away, sees |b - A x| >= |b| and stops
   // with converged = 1.  The flexible one sums the vectors it kept and is right to rounding, which at tol 1e-18 is not
   // enough: it restarts from the true residual again and again until max_iter, having no such exit.
   {
      hamd::GMRESParams q = params(configs[0]);
      q.k_dim = 7; q.tol = 1e-18; q.max_iter = 80;
      const Run stuck = solve(A, b, n, q, 4);
      const double rs = true_rel_residual(A, b, stuck.x, n);
      std::printf("residual stopped falling: %d iterations, reported %.6e, recomputed %.6e\n", stuck.res.iterations, stuck.res.rel_residual_norm, rs);
      CHECK(stuck.res.status == hamd::GMRES_OK && stuck.res.converged == 1 && stuck.res.iterations < q.max_iter);
      CHECK(stuck.res.rel_residual_norm >= 1.0 && rs > q.tol);
      q = params(configs[3]);
      q.k_dim = 7; q.tol = 1e-18; q.max_iter = 80;
      const Run on = solve(A, b, n, q, 4);
      const double ro = true_rel_residual(A, b, on.x, n);
      std::printf("the same, flexible:       %d iterations, reported %.6e, recomputed %.6e\n", on.res.iterations, on.res.rel_residual_norm, ro);
      CHECK(on.res.status == hamd::GMRES_NOT_CONVERGED && on.res.converged == 0 && on.res.iterations == q.max_iter);
      CHECK(on.res.iterations > stuck.res.iterations && ro < 1e-13);
   }

   // the traces compared with the recorded ones: every configuration at k_dim 5 across several restarts, a cycle cut short
   // at i = 3 by max_iter with no tolerance, the end at max_iter above a tolerance, the zero right-hand side; then the exit
   // on a residual that stopped falling, and the flexible solver in its place
   for (const Config &cf : configs)
   {
      hamd::GMRESParams q = params(cf);
      q.k_dim = 5; q.tol = 1e-13; q.max_iter = 200;
      const Run restarts = solve(A, b, n, q);
      CHECK(restarts.res.converged == 1 && restarts.res.iterations > 2 * q.k_dim);
      print_trace(cf.name, "restarts", restarts.trace);
      print_trace(cf.name, "zero_rhs", solve(A, Vec((size_t) n, 0.0), n, q).trace);
      q.tol = 1e-14; q.max_iter = 12;
      const Run limit = solve(A, b, n, q);
      CHECK(limit.res.status == hamd::GMRES_NOT_CONVERGED && limit.res.iterations == 12);
      print_trace(cf.name, "max_iter", limit.trace);
      q.k_dim = 7; q.tol = 0.0; q.max_iter = 10;
      print_trace(cf.name, "cut_short", solve(A, b, n, q).trace);
   }
   for (int which : {0, 3})
   {
      hamd::GMRESParams q = params(configs[which]);
      q.k_dim = 7; q.tol = 1e-18; q.max_iter = 80;
      print_trace(configs[which].name, "residual_stopped_falling", solve(A, b, n, q, 4).trace);
   }
   std::printf("gmres host check ok: %d configurations\n", (int) (sizeof(configs) / sizeof(configs[0])));
   return 0;
}
