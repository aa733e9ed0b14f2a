// What the stand-alone host checks of the Krylov iterations share (gmres_host_check.cpp, lgmres_host_check.cpp): the vector
// callbacks of gmres_core.hpp / lgmres_core.hpp on plain arrays with a dense matrix and a Jacobi preconditioner, the probes
// the checks read, and a trace.  The trace is a 64-bit FNV-1a hash that every callback folds its name, the positions of its
// operand vectors, the bits of its scalar arguments and the bits of any scalar it returns into; trace_end folds in the
// iterate and the result.  Two builds of an iteration that print the same hash made the same calls in the same order with
// the same numbers: tests/golden/krylov_host_traces.json holds the hashes of a recorded commit.  Built with
// -ffp-contract=off and no -march, the hashes depend on IEEE double arithmetic and a correctly rounded sqrt only.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <utility>
#include <vector>

using Vec = std::vector<double>;

struct Trace
{
   std::uint64_t hash = 14695981039346656037ull;
   void bytes(const void *p, size_t len)
   {
      const unsigned char *c = (const unsigned char *) p;
      for (size_t i = 0; i < len; i++) { hash ^= c[i]; hash *= 1099511628211ull; }
   }
   void text(const char *s) { bytes(s, std::strlen(s)); }
   void integer(long long v) { bytes(&v, sizeof v); }
   void real(double v) { bytes(&v, sizeof v); }
};

struct DenseOps
{
   int n;
   const Vec &A;                      // row-major n x n
   // probes of the GMRES check
   double omega = 1.0;                // damping of the Jacobi preconditioner
   int calls = 0;
   double last_rel = 0.0;
   bool rel_in_order = true;
   int k_dim = 1;
   bool vary = false;                 // omega changes with every precond call: only a flexible solver may be given that
   int wrong_from = 0;                // from this iteration on the preconditioner answers 100 times too large (0: never)
   // probes of the LGMRES check
   const Vec *w = nullptr;            // the correction vector: a preconditioner call on it is the unwinding that ends a cycle
   int arnoldi = 0, cycles = 0, fused_calls = 0;

   Trace trace;
   enum { B = 1, X, R, W, P = 100, PRE = 200, AUG = 300, A_AUG = 400 };     // an array's vector i is its base + i
   std::vector<std::pair<const Vec *, int>> ids;

   DenseOps(int n_, const Vec &A_) : n(n_), A(A_) {}
   void name(const Vec *v, int id) { ids.emplace_back(v, id); }
   void name(const std::vector<Vec *> &vs, int base) { for (size_t i = 0; i < vs.size(); i++) { name(vs[i], base + (int) i); } }
   int id(const Vec *v) const { for (const auto &e : ids) { if (e.first == v) { return e.second; } } return 0; }
   void call(const char *what, std::initializer_list<const Vec *> vs, std::initializer_list<double> scalars = {})
   {
      trace.text(what);
      for (const Vec *v : vs) { trace.integer(id(v)); }
      for (double a : scalars) { trace.real(a); }
   }
   double returns(double v) { trace.real(v); return v; }
   template <class Result>
   std::uint64_t trace_end(const Vec &x, const Result &res, long fused_updates = 0, long plain_updates = 0)
   {
      for (double v : x) { trace.real(v); }
      for (long long v : {(long long) res.status, (long long) res.iterations, (long long) res.converged, (long long) res.iterations_set,
                          (long long) res.norm_set, (long long) res.fused_steps, (long long) res.plain_dots, (long long) res.plain_axpys,
                          (long long) fused_updates, (long long) plain_updates}) { trace.integer(v); }
      trace.real(res.rel_residual_norm);
      return trace.hash;
   }

   double dot(const Vec *x, const Vec *y) const { double t = 0.0; for (int i = 0; i < n; i++) { t += (*x)[i] * (*y)[i]; } return t; }
   void add(double a, const Vec *x, Vec *y) const { for (int i = 0; i < n; i++) { (*y)[i] += a * (*x)[i]; } }

   void matvec(double alpha, Vec *x, double beta, Vec *y)
   {
      call("matvec", {x, y}, {alpha, beta});
      for (int i = 0; i < n; i++)
      {
         double t = 0.0;
         for (int j = 0; j < n; j++) { t += A[(size_t) i * n + j] * (*x)[j]; }
         (*y)[i] = alpha * t + beta * (*y)[i];
      }
   }
   double inner(Vec *x, Vec *y) { call("inner", {x, y}); return returns(dot(x, y)); }
   void copy(Vec *x, Vec *y) { call("copy", {x, y}); *y = *x; }
   void scale(double a, Vec *y) { call("scale", {y}, {a}); for (double &v : *y) { v *= a; } }
   void axpy(double a, Vec *x, Vec *y) { call("axpy", {x, y}, {a}); add(a, x, y); }
   double axpy_dot(double a, Vec *x, Vec *y, Vec *z) { call("axpy_dot", {x, y, z}, {a}); add(a, x, y); return returns(dot(z, y)); }
   void mass_axpy(double *a, Vec **xs, Vec *y, int k, int unroll)
   {
      call("mass_axpy", {y}, {(double) k, (double) unroll});
      for (int j = 0; j < k; j++) { call("", {xs[j]}, {a[j]}); add(a[j], xs[j], y); }
   }
   void mass_inner(Vec *x, Vec **ys, int k, int unroll, double *out)
   {
      call("mass_inner", {x}, {(double) k, (double) unroll});
      for (int j = 0; j < k; j++) { call("", {ys[j]}); out[j] = returns(dot(x, ys[j])); }
   }
   void mass_dot_two(Vec *x, Vec *y, Vec **zs, int k, int unroll, double *outx, double *outy)
   {
      call("mass_dot_two", {x, y}, {(double) k, (double) unroll});
      for (int j = 0; j < k; j++) { call("", {zs[j]}); outx[j] = returns(dot(x, zs[j])); outy[j] = returns(dot(y, zs[j])); }
   }
   void scaled_copy(double a, Vec *x, Vec *y) { call("scaled_copy", {x, y}, {a}); fused_calls++; for (int i = 0; i < n; i++) { (*y)[i] = a * (*x)[i]; } }
   double copy_norm2(Vec *x, Vec *y) { call("copy_norm2", {x, y}); fused_calls++; *y = *x; return returns(dot(y, y)); }
   void scaled_diff(double a, Vec *x, Vec *y, Vec *z)
   {
      call("scaled_diff", {x, y, z}, {a});
      fused_calls++;
      for (int i = 0; i < n; i++) { (*z)[i] = ((*y)[i] - (*x)[i]) * -a; }
   }
   void precond(int iter, double rel, Vec *rhs, Vec *sol)
   {
      call("precond", {rhs, sol}, {(double) iter, rel});
      calls++;
      if (rhs == w) { cycles++; } else { arnoldi++; }
      if (iter != calls) { rel_in_order = false; }
      if ((iter - 1) % k_dim != 0 && rel > last_rel) { rel_in_order = false; }      // non-increasing inside a restart cycle
      last_rel = rel;
      if (vary) { omega = (iter % 2) ? 1.0 : 0.6; }
      const double f = (wrong_from && iter >= wrong_from) ? 100.0 * omega : omega;
      for (int i = 0; i < n; i++) { (*sol)[i] = f * (*rhs)[i] / A[(size_t) i * n + i]; }
   }
   void solution_changed(Vec *x) { call("solution_changed", {x}); }
};

// vectors allocated one by one: an index past the end of an array of them is a heap overflow the sanitizer sees
struct VecPool
{
   std::vector<std::unique_ptr<Vec>> own;
   std::vector<Vec *> several(int count, int n)
   {
      std::vector<Vec *> v;
      for (int i = 0; i < count; i++) { own.emplace_back(new Vec((size_t) n, 0.0)); v.push_back(own.back().get()); }
      return v;
   }
};

static inline double true_rel_residual(const Vec &A, const Vec &b, const Vec &x, int n)
{
   double rr = 0.0, bb = 0.0;
   for (int i = 0; i < n; i++)
   {
      double t = b[i];
      for (int j = 0; j < n; j++) { t -= A[(size_t) i * n + j] * x[j]; }
      rr += t * t; bb += b[i] * b[i];
   }
   return std::sqrt(rr / bb);
}

static inline void print_trace(const char *run, const char *variant, std::uint64_t hash)
{
   std::printf("trace %s/%s %016llx\n", run, variant, (unsigned long long) hash);
}

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
