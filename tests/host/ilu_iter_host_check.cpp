// Stand-alone host program: the iterative triangular solves of hypre_amd/csrc/ilu_host.hpp (solve_iter) and the row-slice
// form the device sweeps read (build_slices), built with the address and undefined-behaviour sanitizers
// (tests/test_ilu_iter_host.py).  Checked here, all bit for bit: solve_iter against Jacobi sweeps written out of place with
// two buffers; a walk over the slices the way a lane of the device kernel walks them (entry k of lane l at
// base + 64 k + l, a short row stopping at its own length, every index bounds-checked) against solve_iter; sweeps beyond the
// nilpotency index of a tridiagonal factor against each other and against the direct solve; the slice tables themselves.
#include "ilu_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace hamd::ilu;

namespace {
struct Csr { int n = 0; std::vector<int> i, j; std::vector<double> a; };

void fail(const char *what) { printf("FAILED: %s\n", what); exit(1); }

double value(unsigned &state)
{
   state = state * 1664525u + 1013904223u;
   return (double) (state >> 8) / (double) (1u << 24) - 0.5;
}

Csr stencil(int nx, int ny, int nz, bool full, double conv)
{
   Csr A;
   A.n = nx * ny * nz;
   A.i.push_back(0);
   unsigned st = 7u;
   for (int z = 0; z < nz; z++) for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++)
   {
      const int r = (z * ny + y) * nx + x;
      A.j.push_back(r); A.a.push_back((full ? 26.0 : 6.0) + conv + 0.1 * value(st));
      for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++)
      {
         const int m = abs(dx) + abs(dy) + abs(dz);
         if (m == 0 || (!full && m != 1)) { continue; }
         const int X = x + dx, Y = y + dy, Z = z + dz;
         if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) { continue; }
         A.j.push_back((Z * ny + Y) * nx + X);
         A.a.push_back(((dx + dy + dz > 0) ? -1.0 + conv / 3.0 : -1.0) + 0.1 * value(st));
      }
      A.i.push_back((int) A.j.size());
   }
   return A;
}

Csr diagonal(int n)
{
   Csr A; A.n = n; A.i.push_back(0);
   for (int r = 0; r < n; r++) { A.j.push_back(r); A.a.push_back(1.5 + r); A.i.push_back(r + 1); }
   return A;
}

bool same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
   return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

// the specification with two buffers: iterate k is written beside iterate k - 1, in the permuted index space
std::vector<double> sweeps_out_of_place(const Factors &F, const std::vector<double> &f, int lower, int upper)
{
   const int n = F.n;
   std::vector<double> y((size_t) n, 0.0), z((size_t) n, 0.0), next((size_t) n, 0.0), out((size_t) n, 0.0);
   if (lower <= 0 || upper <= 0) { return out; }
   for (int k = 0; k < lower; k++)
   {
      for (int i = 0; i < n; i++)
      {
         double sum = 0.0;
         for (int q = F.Li[(size_t) i]; q < F.Li[(size_t) i + 1]; q++) { sum += F.La[(size_t) q] * y[(size_t) F.Lj[(size_t) q]]; }
         next[(size_t) i] = f[(size_t) F.perm[(size_t) i]] - sum;
      }
      y.swap(next);
   }
   for (int k = 0; k < upper; k++)
   {
      for (int i = 0; i < n; i++)
      {
         double sum = 0.0;
         for (int q = F.Ui[(size_t) i]; q < F.Ui[(size_t) i + 1]; q++) { sum += F.Ua[(size_t) q] * z[(size_t) F.Uj[(size_t) q]]; }
         next[(size_t) i] = F.D[(size_t) i] * (y[(size_t) i] - sum);
      }
      z.swap(next);
   }
   for (int i = 0; i < n; i++) { out[(size_t) F.perm[(size_t) i]] = z[(size_t) i]; }
   return out;
}

// one sweep over a factor in slices, a lane at a time: x_r = rhs_r - sum, times dinv for U; vectors in the vector numbering
void slice_sweep(const Slices &M, int n, bool upper, const std::vector<double> &rhs, const std::vector<double> *in, std::vector<double> &out)
{
   for (int slot = 0; slot < M.nslices * SLICE_ROWS; slot++)
   {
      const int r = M.row.at((size_t) slot);
      if (r < 0) { continue; }
      if (r >= n) { fail("a slot names a row outside the vectors"); }
      const int len = in ? M.len.at((size_t) slot) : 0;
      const size_t first = (size_t) M.base.at((size_t) (slot / SLICE_ROWS)) + (size_t) (slot % SLICE_ROWS);
      double sum = 0.0;
      for (int k = 0; k < len; k++)
      {
         const size_t at = first + (size_t) k * SLICE_ROWS;
         sum += M.val.at(at) * in->at((size_t) M.col.at(at));
      }
      double x = rhs.at((size_t) r) - sum;
      if (upper) { x = M.dinv.at((size_t) slot) * x; }
      out.at((size_t) r) = x;
   }
}

void check(const Csr &A, int lfil, int reordering, const char *name)
{
   Factors F;
   factor(A.n, A.i.data(), A.j.data(), A.a.data(), lfil, reordering, F);
   const int n = A.n;
   Levels VL, VU;
   build_levels(n, F.Li.data(), F.Lj.data(), true, VL);
   build_levels(n, F.Ui.data(), F.Uj.data(), false, VU);
   Slices SL, SU;
   build_slices(F, VL.order, F.Li, F.Lj, F.La, SL);
   build_slices(F, VU.order, F.Ui, F.Uj, F.Ua, SU);
   // the tables: every row once, its length, a slice as long as its longest row, every entry in its stored order
   for (int pass = 0; pass < 2; pass++)
   {
      const Slices &M = pass ? SU : SL;
      const std::vector<int> &Ti = pass ? F.Ui : F.Li, &Tj = pass ? F.Uj : F.Lj;
      const std::vector<double> &Ta = pass ? F.Ua : F.La;
      const std::vector<int> &order = pass ? VU.order : VL.order;
      if (M.nslices != (n + SLICE_ROWS - 1) / SLICE_ROWS || (long long) M.col.size() != M.padded || M.val.size() != M.col.size()) { fail("slice counts"); }
      if (M.padded < (long long) Tj.size()) { fail("padded entries below stored entries"); }
      long long expect_base = 0;
      for (int s = 0; s < M.nslices; s++)
      {
         if (M.base[(size_t) s] != expect_base) { fail("slice base"); }
         int longest = 0;
         for (int l = 0; l < SLICE_ROWS; l++)
         {
            const int t = s * SLICE_ROWS + l;
            if (t >= n)
            {
               if (M.row[(size_t) t] != -1 || M.len[(size_t) t] != 0) { fail("a slot past the last row is not marked"); }
               continue;
            }
            const int r = order[(size_t) t];
            if (M.row[(size_t) t] != F.perm[(size_t) r] || M.len[(size_t) t] != Ti[(size_t) r + 1] - Ti[(size_t) r] || M.dinv[(size_t) t] != F.D[(size_t) r]) { fail("slot tables"); }
            longest = std::max(longest, M.len[(size_t) t]);
            for (int k = 0; k < M.len[(size_t) t]; k++)
            {
               const size_t at = (size_t) expect_base + (size_t) k * SLICE_ROWS + (size_t) l;
               if (M.col[at] != F.perm[(size_t) Tj[(size_t) Ti[(size_t) r] + (size_t) k]] || M.val[at] != Ta[(size_t) Ti[(size_t) r] + (size_t) k]) { fail("slice entry"); }
            }
         }
         expect_base += (long long) longest * SLICE_ROWS;
      }
      if (expect_base != M.padded) { fail("padded entry count"); }
   }
   unsigned st = 11u + (unsigned) n;
   std::vector<double> f((size_t) n);
   for (double &v : f) { v = value(st); }
   const int pairs[8][2] = {{0, 0}, {0, 3}, {3, 0}, {1, 1}, {1, 2}, {2, 1}, {5, 5}, {3, 7}};
   for (const auto &p : pairs)
   {
      const int lower = p[0], upper = p[1];
      std::vector<double> y((size_t) n, 9.0), z((size_t) n, 9.0);
      solve_iter(F, f.data(), y.data(), z.data(), lower, upper);
      if (!same_bits(z, sweeps_out_of_place(F, f, lower, upper))) { printf("%s %d %d\n", name, lower, upper); fail("solve_iter differs from out-of-place sweeps"); }
      // the slices, swept as the device sweeps them: y^1 = f and z^1 = Dinv y without a product
      std::vector<double> zs((size_t) n, 0.0);
      if (lower > 0 && upper > 0)
      {
         std::vector<double> a(f), b((size_t) n, 0.0);
         for (int k = 2; k <= lower; k++) { slice_sweep(SL, n, false, f, &a, b); a.swap(b); }
         std::vector<double> zk((size_t) n, 0.0), zn((size_t) n, 0.0);
         slice_sweep(SU, n, true, a, nullptr, zk);
         for (int k = 2; k <= upper; k++) { slice_sweep(SU, n, true, a, &zk, zn); zk.swap(zn); }
         zs = zk;
      }
      if (!same_bits(z, zs)) { printf("%s %d %d\n", name, lower, upper); fail("sweeps over the slices differ from solve_iter"); }
   }
   printf("%-28s lfil %d reordering %d: nnz L %zu U %zu, padded L %lld U %lld\n", name, lfil, reordering, F.Lj.size(), F.Uj.size(), SL.padded, SU.padded);
}
}  // namespace

int main()
{
   const Csr grid = stencil(17, 13, 1, false, 0.0), box = stencil(6, 6, 6, true, 0.0), conv = stencil(7, 6, 5, false, 0.9), diag = diagonal(130),
             one = diagonal(1), none = diagonal(0), tri = stencil(300, 1, 1, false, 0.0);
   for (int lfil = 0; lfil <= 1; lfil++) for (int reordering = 0; reordering <= 1; reordering++)
   {
      check(grid, lfil, reordering, "17x13 5-point");
      check(conv, lfil, reordering, "non-symmetric 7x6x5");
      check(diag, lfil, reordering, "diagonal 130");
      check(one, lfil, reordering, "one row");
      check(none, lfil, reordering, "no row");
   }
   check(box, 1, 1, "6^3 27-point");
   check(tri, 0, 0, "tridiagonal 300");
   // a strictly triangular matrix of 300 levels is nilpotent of index 300: sweeps beyond that change nothing, and the
   // result is the direct solve (rows of one entry: 0 + p and f - p round as the direct chain does)
   {
      Factors F;
      factor(tri.n, tri.i.data(), tri.j.data(), tri.a.data(), 0, 0, F);
      const size_t n = (size_t) tri.n;
      unsigned st = 3u;
      std::vector<double> f(n), y(n), z300(n), z303(n), direct(n, 0.0);
      for (double &v : f) { v = value(st); }
      solve_iter(F, f.data(), y.data(), z300.data(), 300, 300);
      solve_iter(F, f.data(), y.data(), z303.data(), 303, 303);
      solve(F, f.data(), direct.data());
      if (!same_bits(z300, z303)) { fail("sweeps past the nilpotency index change the result"); }
      if (!same_bits(z300, direct)) { fail("300 sweeps of a 300-level factor are not the direct solve"); }
      solve_iter(F, f.data(), y.data(), z303.data(), 2, 2);
      if (same_bits(z300, z303)) { fail("two sweeps already give the direct solve: the count is not the sweep count"); }
   }
   printf("ilu iter host check ok\n");
   return 0;
}
