// Stand-alone host program: the local reverse Cuthill-McKee ordering, the ILU(k) pattern and the numeric factorisation of
// hypre_amd/csrc/ilu_host.hpp on small matrices, built with the address and undefined-behaviour sanitizers
// (tests/test_ilu_host.py).  Checked here: the ordering is a permutation and puts a path graph in path order; the factors
// reproduce the permuted matrix on their own pattern (the defining property of an incomplete factorisation); ILU(0) of a
// tridiagonal matrix solves it; the levels are a valid schedule; a tiny pivot is replaced.
#include "ilu_host.hpp"
#include <cstdio>
#include <cstdlib>

using namespace hamd::ilu;

namespace {
struct Csr { int n = 0; std::vector<int> i, j; std::vector<double> a; };

void fail(const char *what) { printf("FAILED: %s\n", what); exit(1); }

Csr stencil(int nx, int ny, int nz, bool full, double conv)
{
   Csr A;
   A.n = nx * ny * nz;
   A.i.push_back(0);
   for (int z = 0; z < nz; z++) for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++)
   {
      const int r = (z * ny + y) * nx + x;
      A.j.push_back(r); A.a.push_back(full ? 26.0 : 6.0 + conv);
      for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++)
      {
         const int m = abs(dx) + abs(dy) + abs(dz);
         if (m == 0 || (!full && m != 1)) { continue; }
         const int X = x + dx, Y = y + dy, Z = z + dz;
         if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) { continue; }
         A.j.push_back((Z * ny + Y) * nx + X);
         A.a.push_back((dx + dy + dz > 0) ? -1.0 + conv / 3.0 : -1.0);       // conv != 0: a non-symmetric operator
      }
      A.i.push_back((int) A.j.size());
   }
   return A;
}

// (L + I) D (I + U)-style product of the stored factors, entry (r, c) in the permuted numbering: sum_k L_rk u_kc with
// u_kk = 1 / Dinv_k (the factorisation is L (D + U) with unit L, D = 1 / Dinv)
double product_entry(const Factors &F, int r, int c)
{
   auto U_at = [&](int k, int col) {
      if (col == k) { return 1.0 / F.D[(size_t) k]; }
      for (int q = F.Ui[(size_t) k]; q < F.Ui[(size_t) k + 1]; q++) { if (F.Uj[(size_t) q] == col) { return F.Ua[(size_t) q]; } }
      return 0.0;
   };
   double s = U_at(r, c) * (c >= r ? 1.0 : 0.0);
   for (int q = F.Li[(size_t) r]; q < F.Li[(size_t) r + 1]; q++)
   {
      const int k = F.Lj[(size_t) q];
      if (k <= c) { s += F.La[(size_t) q] * U_at(k, c); }
   }
   return s;
}

void check(const Csr &A, int lfil, int reordering, const char *name)
{
   Factors F;
   factor(A.n, A.i.data(), A.j.data(), A.a.data(), lfil, reordering, F);
   const int n = A.n;
   std::vector<int> seen((size_t) n, 0), rperm((size_t) n, 0);
   for (int i = 0; i < n; i++)
   {
      const int p = F.perm[(size_t) i];
      if (p < 0 || p >= n || seen[(size_t) p]++) { fail("perm is not a permutation"); }
      rperm[(size_t) p] = i;
   }
   for (int i = 0; i < n; i++)
   {
      for (int q = F.Li[(size_t) i]; q < F.Li[(size_t) i + 1]; q++)
      {
         if (F.Lj[(size_t) q] >= i || (q > F.Li[(size_t) i] && F.Lj[(size_t) q] <= F.Lj[(size_t) q - 1])) { fail("L is not strictly lower with ascending columns"); }
      }
      for (int q = F.Ui[(size_t) i]; q < F.Ui[(size_t) i + 1]; q++) { if (F.Uj[(size_t) q] <= i) { fail("U is not strictly upper"); } }
   }
   // on the pattern of A the product of the factors is A (any level of fill keeps A's entries)
   double worst = 0.0;
   for (int i = 0; i < n; i++)
   {
      const int r = F.perm[(size_t) i];
      for (int q = A.i[(size_t) r]; q < A.i[(size_t) r + 1]; q++)
      {
         worst = std::max(worst, std::fabs(product_entry(F, i, rperm[(size_t) A.j[(size_t) q]]) - A.a[(size_t) q]));
      }
   }
   if (worst > 1e-12) { printf("%s: product off by %.3e\n", name, worst); fail("L (D + U) differs from A on A's pattern"); }
   // levels: every row after the rows it reads
   Levels VL, VU;
   build_levels(n, F.Li.data(), F.Lj.data(), true, VL);
   build_levels(n, F.Ui.data(), F.Uj.data(), false, VU);
   for (int pass = 0; pass < 2; pass++)
   {
      const Levels &V = pass ? VU : VL;
      const std::vector<int> &Ti = pass ? F.Ui : F.Li, &Tj = pass ? F.Uj : F.Lj;
      std::vector<int> lev_of((size_t) std::max(n, 1), -1);
      if ((int) V.order.size() != n || V.lev_start.back() != n) { fail("levels do not cover the rows"); }
      for (int l = 0; l < V.nlev; l++) for (int s = V.lev_start[(size_t) l]; s < V.lev_start[(size_t) l + 1]; s++) { lev_of[(size_t) V.order[(size_t) s]] = l; }
      for (int i = 0; i < n; i++) for (int q = Ti[(size_t) i]; q < Ti[(size_t) i + 1]; q++)
      {
         if (lev_of[(size_t) Tj[(size_t) q]] >= lev_of[(size_t) i]) { fail("a row is scheduled before a row it reads"); }
      }
   }
   // one solve runs and gives finite numbers
   std::vector<double> f((size_t) n, 1.0), u((size_t) n, 0.0);
   solve(F, f.data(), u.data());
   for (double v : u) { if (!(v == v) || std::fabs(v) > 1e300) { fail("solve gave a non-number"); } }
   printf("%-28s lfil %d reordering %d: nnz L %zu U %zu, levels %d / %d, product error %.2e\n", name, lfil, reordering, F.Lj.size(), F.Uj.size(),
          VL.nlev, VU.nlev, worst);
}
}  // namespace

int main()
{
   // a path graph in scrambled numbering comes out in path order
   {
      const int n = 9, label[n] = {4, 0, 7, 2, 8, 1, 5, 3, 6};          // node at position p of the path
      std::vector<std::vector<int>> adj((size_t) n);
      for (int p = 0; p + 1 < n; p++) { adj[(size_t) label[p]].push_back(label[p + 1]); adj[(size_t) label[p + 1]].push_back(label[p]); }
      Csr A; A.n = n; A.i.push_back(0);
      for (int r = 0; r < n; r++) { A.j.push_back(r); for (int c : adj[(size_t) r]) { A.j.push_back(c); } A.i.push_back((int) A.j.size()); }
      std::vector<int> perm;
      local_rcm(n, A.i.data(), A.j.data(), perm);
      bool fwd = true, bwd = true;
      for (int p = 0; p < n; p++) { fwd = fwd && perm[(size_t) p] == label[p]; bwd = bwd && perm[(size_t) p] == label[n - 1 - p]; }
      if (!fwd && !bwd) { fail("RCM of a path is not the path"); }
      // no off-diagonal entry, one row, no row: identity
      Csr D; D.n = 4; D.i = {0, 1, 2, 3, 4}; D.j = {0, 1, 2, 3};
      local_rcm(4, D.i.data(), D.j.data(), perm);
      for (int p = 0; p < 4; p++) { if (perm[(size_t) p] != p) { fail("RCM of a diagonal matrix is not the identity"); } }
      const int one_i[2] = {0, 1}, one_j[1] = {0}, none_i[1] = {0};
      local_rcm(1, one_i, one_j, perm);
      if (perm.size() != 1 || perm[0] != 0) { fail("RCM of one row"); }
      local_rcm(0, none_i, nullptr, perm);
      if (!perm.empty()) { fail("RCM of no row"); }
   }
   const Csr grid = stencil(8, 8, 1, false, 0.0), box = stencil(4, 4, 4, true, 0.0), conv = stencil(5, 4, 3, false, 0.9), tri = stencil(30, 1, 1, false, 0.0);
   for (int lfil = 0; lfil <= 2; lfil++) for (int reordering = 0; reordering <= 1; reordering++)
   {
      check(grid, lfil, reordering, "8x8 5-point");
      check(box, lfil, reordering, "4^3 27-point");
      check(conv, lfil, reordering, "non-symmetric 5x4x3");
      check(tri, lfil, reordering, "tridiagonal 30");
   }
   // ILU(0) of a tridiagonal matrix is its LU: one solve is the solution
   {
      Factors F;
      factor(tri.n, tri.i.data(), tri.j.data(), tri.a.data(), 0, 1, F);
      std::vector<double> x((size_t) tri.n), f((size_t) tri.n, 0.0), u((size_t) tri.n, 0.0);
      for (int i = 0; i < tri.n; i++) { x[(size_t) i] = 1.0 + 0.25 * i; }
      for (int i = 0; i < tri.n; i++) for (int q = tri.i[(size_t) i]; q < tri.i[(size_t) i + 1]; q++) { f[(size_t) i] += tri.a[(size_t) q] * x[(size_t) tri.j[(size_t) q]]; }
      solve(F, f.data(), u.data());
      for (int i = 0; i < tri.n; i++) { if (std::fabs(u[(size_t) i] - x[(size_t) i]) > 1e-12 * x[(size_t) i]) { fail("ILU(0) of a tridiagonal matrix does not solve it"); } }
   }
   // a pivot below 1e-14 becomes 1e-6; empty matrix
   {
      Csr S; S.n = 2; S.i = {0, 2, 4}; S.j = {0, 1, 0, 1}; S.a = {1.0e-15, 1.0, 1.0, 2.0};
      Factors F;
      factor(2, S.i.data(), S.j.data(), S.a.data(), 0, 0, F);
      if (F.D[0] != 1.0 / PIVOT_SUBSTITUTE) { fail("small pivot not replaced"); }
      const int none_i[1] = {0};
      factor(0, none_i, nullptr, nullptr, 1, 1, F);
      Levels V;
      build_levels(0, F.Li.data(), F.Lj.data(), true, V);
      if (F.n != 0 || V.nlev != 0) { fail("empty matrix"); }
      solve(F, nullptr, nullptr);
   }
   printf("ilu host check ok\n");
   return 0;
}
