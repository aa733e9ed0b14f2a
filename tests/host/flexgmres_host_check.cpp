// Stand-alone host check of the FlexGMRES iteration (hypre_amd/csrc/flexgmres_core.hpp): the Hessenberg / Givens /
// restart logic of par_flexgmres.cpp with plain arrays behind the vector callbacks, on a dense non-symmetric system of
// 50 unknowns with a preconditioner that changes every iteration.  Meant to be built with
//    c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hypre_amd/csrc
// and run once (tests/test_flexgmres_host.py does): any out-of-bounds index into hh / rs / c / s, the basis arrays or the
// coefficient lists of the batched correction ends the program.  It also checks what it computes: convergence across
// several restarts, the true residual, the same bits with the fused and the plain Gram-Schmidt, the "not converged" end,
// the zero right-hand side and the modify_pc protocol.
#include "flexgmres_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <memory>

using Vec = std::vector<double>;

struct DenseOps
{
   int n;
   const Vec &A;                      // row-major n x n
   double omega = 1.0;                // damping of the Jacobi preconditioner, changed by every precond call
   int calls = 0;
   double last_rel = 0.0;
   bool rel_in_order = true;
   int k_dim;
   void matvec(double alpha, Vec *x, double beta, Vec *y)
   {
      for (int i = 0; i < n; i++)
      {
         double t = 0.0;
         for (int j = 0; j < n; j++) { t += A[(size_t) i * n + j] * (*x)[j]; }
         (*y)[i] = alpha * t + beta * (*y)[i];
      }
   }
   double inner(Vec *x, Vec *y) { double t = 0.0; for (int i = 0; i < n; i++) { t += (*x)[i] * (*y)[i]; } return t; }
   void copy(Vec *x, Vec *y) { *y = *x; }
   void scale(double a, Vec *y) { for (double &v : *y) { v *= a; } }
   void axpy(double a, Vec *x, Vec *y) { for (int i = 0; i < n; i++) { (*y)[i] += a * (*x)[i]; } }
   double axpy_dot(double a, Vec *x, Vec *y, Vec *z) { axpy(a, x, y); return inner(z, y); }
   void mass_axpy(double *a, Vec **xs, Vec *y, int k) { for (int j = 0; j < k; j++) { axpy(a[j], xs[j], y); } }
   void precond(int iter, double rel, Vec *rhs, Vec *sol)
   {
      calls++;
      if (iter != calls) { rel_in_order = false; }
      if ((iter - 1) % k_dim != 0 && rel > last_rel) { rel_in_order = false; }      // non-increasing inside a restart cycle
      last_rel = rel;
      omega = (iter % 2) ? 1.0 : 0.6;
      for (int i = 0; i < n; i++) { (*sol)[i] = omega * (*rhs)[i] / A[(size_t) i * n + i]; }
   }
   void solution_changed(Vec *) {}
};

struct Run { hamd::FlexGMRESResult res; Vec x; int calls; bool in_order; };

static Run solve(const Vec &A, const Vec &b_in, int n, const hamd::FlexGMRESParams &prm)
{
   Vec b = b_in, x((size_t) n, 0.0), r((size_t) n), w((size_t) n);
   // exactly k_dim + 1 vectors each, allocated one by one: an index past the end is a heap overflow the sanitizer sees
   std::vector<std::unique_ptr<Vec>> ps, zs;
   std::vector<Vec *> p, z;
   for (int i = 0; i <= prm.k_dim; i++)
   {
      ps.emplace_back(new Vec((size_t) n, 0.0)); zs.emplace_back(new Vec((size_t) n, 0.0));
      p.push_back(ps.back().get()); z.push_back(zs.back().get());
   }
   DenseOps ops{n, A, 1.0, 0, 0.0, true, prm.k_dim};
   Run out;
   out.res = hamd::flexgmres_iterate<Vec *>(prm, ops, &b, &x, &r, &w, p.data(), z.data());
   out.x = x; out.calls = ops.calls; out.in_order = ops.rel_in_order;
   return out;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

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
   hamd::FlexGMRESParams prm;
   prm.k_dim = 7; prm.tol = 1e-10; prm.max_iter = 200;
   prm.fused = 1;
   const Run f = solve(A, b, n, prm);
   prm.fused = 0;
   const Run g = solve(A, b, n, prm);
   CHECK(f.res.status == hamd::FLEXGMRES_OK && f.res.converged == 1 && f.res.norm_set);
   CHECK(f.res.iterations > prm.k_dim);                                            // more than one restart cycle
   CHECK(f.calls == f.res.iterations && f.in_order);
   double rr = 0.0, bb = 0.0;
   for (int i = 0; i < n; i++)
   {
      double t = b[i];
      for (int j = 0; j < n; j++) { t -= A[(size_t) i * n + j] * f.x[j]; }
      rr += t * t; bb += b[i] * b[i];
   }
   const double rel = std::sqrt(rr / bb);
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
   prm.fused = 1; prm.tol = 0.0; prm.max_iter = 10;
   const Run h = solve(A, b, n, prm);
   CHECK(h.res.status == hamd::FLEXGMRES_NOT_CONVERGED && h.res.iterations == 10 && h.res.converged == 0);
   prm.k_dim = 1; prm.max_iter = 3;
   const Run h1 = solve(A, b, n, prm);
   CHECK(h1.res.iterations == 3);
   // zero right-hand side, zero guess: returns at once
   prm.k_dim = 7; prm.tol = 1e-10; prm.max_iter = 200;
   const Run zr = solve(A, Vec((size_t) n, 0.0), n, prm);
   CHECK(zr.res.status == hamd::FLEXGMRES_OK && zr.res.iterations == 0 && !zr.res.norm_set && zr.calls == 0);
   // a NaN in b is reported, nothing is iterated
   Vec bad = b; bad[3] = std::nan("");
   const Run nn = solve(A, bad, n, prm);
   CHECK(nn.res.status == hamd::FLEXGMRES_NOT_A_NUMBER && nn.calls == 0);
   std::printf("flexgmres host check ok: %d iterations, relative residual %.3e, %ld fused steps\n", f.res.iterations, rel, steps);
   return 0;
}
