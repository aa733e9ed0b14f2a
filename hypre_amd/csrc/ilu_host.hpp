// hypre_amd — block-Jacobi ILU(k) on the host: the local reverse Cuthill-McKee ordering, the symbolic and the numeric
// factorisation of a rank's diagonal block, the two triangular solves (direct, and as Jacobi sweeps), the dependency levels the direct device solve runs by
// and the row slices the device sweeps read (par_ilu.cpp, ilu_kernels.hip, ilu_iter_kernels.hip).  Plain C++ on plain arrays: tests/host/ilu_host_check.cpp builds it on its own.
//
// Reference: parcsr_ls/par_ilu.c:2121-2999 (hypre_ILUGetLocalPerm, hypre_ILULocalRCM*), par_ilu_setup.c:2171-2517
// (hypre_ILUSetupILU0), :2872-3114 (hypre_ILUSetupILUKSymbolic), :3299-3583 (hypre_ILUSetupILUK), par_ilu_solve.c:829-950
// (hypre_ILUSolveLU), :960-1110 (hypre_ILUSolveLUIter).  Factors live in the permuted numbering: row ii of L, D and U is row perm[ii] of A.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace hamd {
namespace ilu {

constexpr double MAT_TOL = 1e-14;            // par_ilu.h:256: a pivot below it in magnitude ...
constexpr double PIVOT_SUBSTITUTE = 1.0e-6;  // ... is replaced by this (par_ilu_setup.c:2479-2483, 3578-3582)

struct Factors
{
   int n = 0;
   std::vector<int> perm;                    // [n] row ii of the factors is row perm[ii] of A (identity without reordering)
   std::vector<int> Li, Lj, Ui, Uj;          // unit L strictly below the diagonal (columns ascending), U strictly above (order of discovery)
   std::vector<double> La, Ua, D;            // D holds the inverse pivots
};

// ---- reverse Cuthill-McKee (par_ilu.c:2687-2999), every tie broken as there ----
namespace rcm {
inline void build_level(const int *Gi, const int *Gj, int root, std::vector<int> &marker, std::vector<int> &level_i, std::vector<int> &level_j,
                        int *nlevp)
{
   level_i[0] = 0;
   level_j[0] = root;
   marker[(size_t) root] = 0;
   int nlev = 1, l1 = 0, l2 = 1, l_current = 1;
   while (l2 > l1)
   {
      level_i[(size_t) nlev++] = l2;
      for (int i = l1; i < l2; i++)
      {
         const int rowi = level_j[(size_t) i];
         for (int j = Gi[rowi]; j < Gi[rowi + 1]; j++)
         {
            const int rowj = Gj[j];
            if (marker[(size_t) rowj] < 0) { marker[(size_t) rowj] = 0; level_j[(size_t) l_current++] = rowj; }
         }
      }
      l1 = l2;
      l2 = l_current;
   }
   nlev--;                                    // the last level is an empty one
   for (int i = 0; i < l2; i++) { marker[(size_t) level_j[(size_t) i]] = -1; }
   *nlevp = nlev;
}

// a pseudo-peripheral node of root's component: the node of least degree in the last level, until the depth stops growing
inline int find_pp_node(int n, const int *Gi, const int *Gj, int root, std::vector<int> &marker)
{
   std::vector<int> level_i((size_t) n + 2), level_j((size_t) n + 1);
   int newnlev;
   build_level(Gi, Gj, root, marker, level_i, level_j, &newnlev);
   int nlev = newnlev - 1;
   while (nlev < newnlev)
   {
      nlev = newnlev;
      int min_degree = n;
      for (int i = level_i[(size_t) nlev - 1]; i < level_i[(size_t) nlev]; i++)
      {
         const int row = level_j[(size_t) i], deg = Gi[row + 1] - Gi[row];
         if (min_degree > deg) { min_degree = deg; root = row; }
      }
      build_level(Gi, Gj, root, marker, level_i, level_j, &newnlev);
   }
   return root;
}

// perm[start..end] ascending in degree; the reference's own quicksort, whose order among equal degrees is part of the result
inline void qsort_by_degree(std::vector<int> &perm, int start, int end, const std::vector<int> &degree)
{
   if (start >= end) { return; }
   std::swap(perm[(size_t) start], perm[(size_t) ((start + end) / 2)]);
   int mid = start;
   for (int i = start + 1; i <= end; i++)
   {
      if (degree[(size_t) perm[(size_t) i]] < degree[(size_t) perm[(size_t) start]]) { std::swap(perm[(size_t) ++mid], perm[(size_t) i]); }
   }
   std::swap(perm[(size_t) start], perm[(size_t) mid]);
   qsort_by_degree(perm, mid + 1, end, degree);
   qsort_by_degree(perm, start, mid - 1, degree);
}

// breadth-first numbering of root's component, the new neighbours of every node sorted by degree, then reversed
inline void numbering(const int *Gi, const int *Gj, int root, std::vector<int> &marker, std::vector<int> &perm, int *current_nump)
{
   int current_num = *current_nump;
   marker[(size_t) root] = 0;
   int l1 = current_num;
   perm[(size_t) current_num++] = root;
   int l2 = current_num;
   while (l2 > l1)
   {
      for (int i = l1; i < l2; i++)
      {
         const int rowi = perm[(size_t) i], row_start = current_num;
         for (int j = Gi[rowi]; j < Gi[rowi + 1]; j++)
         {
            const int rowj = Gj[j];
            if (marker[(size_t) rowj] < 0)
            {
               marker[(size_t) rowj] = Gi[rowj + 1] - Gi[rowj];      // the degree, read by the sort
               perm[(size_t) current_num++] = rowj;
            }
         }
         qsort_by_degree(perm, row_start, current_num - 1, marker);
      }
      l1 = l2;
      l2 = current_num;
   }
   std::reverse(perm.begin() + *current_nump, perm.begin() + current_num);
   *current_nump = current_num;
}
}  // namespace rcm

// hypre_ILUGetLocalPerm with reordering 1: RCM on the pattern of the block as it is stored, less its diagonal (the
// reference calls hypre_ILULocalRCM with sym = 1: a non-symmetric pattern is NOT symmetrised); identity when the block
// has no off-diagonal entry
inline void local_rcm(int n, const int *Ai, const int *Aj, std::vector<int> &perm)
{
   perm.resize((size_t) n);
   for (int i = 0; i < n; i++) { perm[(size_t) i] = i; }
   if (n <= 0) { return; }
   std::vector<int> Gi((size_t) n + 1, 0), Gj;
   Gj.reserve((size_t) Ai[n]);
   for (int i = 0; i < n; i++)
   {
      for (int j = Ai[i]; j < Ai[i + 1]; j++)
      {
         if (Aj[j] != i && Aj[j] >= 0 && Aj[j] < n) { Gj.push_back(Aj[j]); }
      }
      Gi[(size_t) i + 1] = (int) Gj.size();
   }
   if (Gj.empty()) { return; }
   std::vector<int> marker((size_t) n, -1), G_perm((size_t) n, 0);
   int current_num = 0;
   while (current_num < n)
   {
      // the unvisited node of least degree, the first of them (hypre_ILULocalRCMMindegree)
      int root = 0, min_degree = n + 1;
      for (int i = 0; i < n; i++)
      {
         if (marker[(size_t) i] < 0 && Gi[(size_t) i + 1] - Gi[(size_t) i] < min_degree) { root = i; min_degree = Gi[(size_t) i + 1] - Gi[(size_t) i]; }
      }
      root = rcm::find_pp_node(n, Gi.data(), Gj.data(), root, marker);
      rcm::numbering(Gi.data(), Gj.data(), root, marker, G_perm, &current_num);
   }
   perm = G_perm;
}

// ---- ILU(k), symbolic: an entry enters with level lev(i,k) + lev(k,j) + 1 if that is at most lfil; L columns ascending,
// U columns in the order they are met (A's entries in stored order first), as the reference stores them ----
inline void symbolic(int n, const int *Ai, const int *Aj, int lfil, const int *perm, const int *rperm, std::vector<int> &Li, std::vector<int> &Lj,
                     std::vector<int> &Ui, std::vector<int> &Uj)
{
   Li.assign((size_t) n + 1, 0); Ui.assign((size_t) n + 1, 0);
   Lj.clear(); Uj.clear();
   std::vector<int> u_levels, lev((size_t) std::max(n, 1), 0), in((size_t) std::max(n, 1), 0), urow;
   for (int ii = 0; ii < n; ii++)
   {
      const int i = perm[ii];
      std::priority_queue<int, std::vector<int>, std::greater<int>> heap;     // columns below ii still to eliminate, smallest first
      urow.clear();
      for (int j = Ai[i]; j < Ai[i + 1]; j++)
      {
         const int col = rperm[Aj[j]];
         if (col == ii || in[(size_t) col]) { continue; }
         in[(size_t) col] = 1; lev[(size_t) col] = 0;
         if (col < ii) { heap.push(col); }
         else { urow.push_back(col); }
      }
      const size_t l0 = Lj.size();
      while (!heap.empty())
      {
         const int k = heap.top();
         heap.pop();
         const int ilev = lev[(size_t) k];
         Lj.push_back(k);
         for (int j = Ui[(size_t) k]; j < Ui[(size_t) k + 1]; j++)
         {
            const int col = Uj[(size_t) j], l = u_levels[(size_t) j] + ilev + 1;
            if (l > lfil) { continue; }
            if (!in[(size_t) col])
            {
               if (col == ii) { continue; }
               in[(size_t) col] = 1; lev[(size_t) col] = l;
               if (col < ii) { heap.push(col); }
               else { urow.push_back(col); }
            }
            else { lev[(size_t) col] = std::min(l, lev[(size_t) col]); }
         }
      }
      for (size_t t = l0; t < Lj.size(); t++) { in[(size_t) Lj[t]] = 0; }
      for (int col : urow) { Uj.push_back(col); u_levels.push_back(lev[(size_t) col]); in[(size_t) col] = 0; }
      Li[(size_t) ii + 1] = (int) Lj.size();
      Ui[(size_t) ii + 1] = (int) Uj.size();
   }
}

// ---- numeric factorisation on the pattern (hypre_ILUSetupILUK; for lfil 0 the values of hypre_ILUSetupILU0) ----
inline void numeric(int n, const int *Ai, const int *Aj, const double *Aa, const int *perm, const int *rperm, Factors &F)
{
   F.La.assign(F.Lj.size(), 0.0); F.Ua.assign(F.Uj.size(), 0.0); F.D.assign((size_t) n, 0.0);
   std::vector<int> iw((size_t) std::max(n, 1), -1);
   const int *Li = F.Li.data(), *Lj = F.Lj.data(), *Ui = F.Ui.data(), *Uj = F.Uj.data();
   double *La = F.La.data(), *Ua = F.Ua.data(), *D = F.D.data();
   for (int ii = 0; ii < n; ii++)
   {
      const int i = perm[ii], kl = Li[ii + 1], ku = Ui[ii + 1];
      for (int j = Li[ii]; j < kl; j++) { iw[(size_t) Lj[j]] = j; }
      D[ii] = 0.0;
      iw[(size_t) ii] = ii;
      for (int j = Ui[ii]; j < ku; j++) { iw[(size_t) Uj[j]] = j; }
      for (int j = Ai[i]; j < Ai[i + 1]; j++)
      {
         const int col = rperm[Aj[j]], icol = iw[(size_t) col];
         if (col < ii) { La[icol] = Aa[j]; }
         else if (col == ii) { D[ii] = Aa[j]; }
         else { Ua[icol] = Aa[j]; }
      }
      for (int j = Li[ii]; j < kl; j++)
      {
         const int jpiv = Lj[j];
         La[j] *= D[jpiv];
         for (int k = Ui[jpiv]; k < Ui[jpiv + 1]; k++)
         {
            const int col = Uj[k], icol = iw[(size_t) col];
            if (icol < 0) { continue; }
            if (col < ii) { La[icol] -= La[j] * Ua[k]; }
            else if (col == ii) { D[ii] -= La[j] * Ua[k]; }
            else { Ua[icol] -= La[j] * Ua[k]; }
         }
      }
      for (int j = Li[ii]; j < kl; j++) { iw[(size_t) Lj[j]] = -1; }
      iw[(size_t) ii] = -1;
      for (int j = Ui[ii]; j < ku; j++) { iw[(size_t) Uj[j]] = -1; }
      if (std::fabs(D[ii]) < MAT_TOL) { D[ii] = PIVOT_SUBSTITUTE; }
      D[ii] = 1. / D[ii];
   }
}

// ordering, pattern and values of the block's factors; reordering: 0 none, 1 reverse Cuthill-McKee
inline void factor(int n, const int *Ai, const int *Aj, const double *Aa, int lfil, int reordering, Factors &F)
{
   F.n = n;
   if (reordering) { local_rcm(n, Ai, Aj, F.perm); }
   else
   {
      F.perm.resize((size_t) n);
      for (int i = 0; i < n; i++) { F.perm[(size_t) i] = i; }
   }
   std::vector<int> rperm((size_t) std::max(n, 1), 0);
   for (int i = 0; i < n; i++) { rperm[(size_t) F.perm[(size_t) i]] = i; }
   symbolic(n, Ai, Aj, lfil, F.perm.data(), rperm.data(), F.Li, F.Lj, F.Ui, F.Uj);
   numeric(n, Ai, Aj, Aa, F.perm.data(), rperm.data(), F);
}

// utemp = (L D^-1 U)^-1 ftemp through the permutation (hypre_ILUSolveLU): a row's sum starts from its right-hand side and
// takes the products away one by one in stored order, every product and every difference rounded.  This is THE association:
// the device kernels run the same chain, one lane per row.
inline void solve(const Factors &F, const double *ftemp, double *utemp)
{
   const int n = F.n;
   const int *perm = F.perm.data();
   for (int i = 0; i < n; i++)
   {
      double s = ftemp[perm[i]];
      for (int j = F.Li[(size_t) i]; j < F.Li[(size_t) i + 1]; j++) { s -= F.La[(size_t) j] * utemp[perm[F.Lj[(size_t) j]]]; }
      utemp[perm[i]] = s;
   }
   for (int i = n - 1; i >= 0; i--)
   {
      double s = utemp[perm[i]];
      for (int j = F.Ui[(size_t) i]; j < F.Ui[(size_t) i + 1]; j++) { s -= F.Ua[(size_t) j] * utemp[perm[F.Uj[(size_t) j]]]; }
      utemp[perm[i]] = s * F.D[(size_t) i];
   }
}

// ---- iterative triangular solves (hypre_ILUSolveLUIter, par_ilu_solve.c:960-1110): each exact solve replaced by a fixed
// number of Jacobi sweeps from a zero iterate.  ztemp = the last upper iterate of
//    y^k_i = ftemp_i - sum_j L_ij y^(k-1)_j   (k = 1 .. lower),    z^k_i = Dinv_i (y_i - sum_j U_ij z^(k-1)_j)   (k = 1 .. upper)
// through the permutation; utemp holds y.  The update is in place, but L's rows run last to first and U's first to last, so a
// row reads values of the sweep before only: Jacobi, not Gauss-Seidel.  THE association of this path, which the device sweep
// runs one lane per row: the sum starts at +0.0, the products are added one by one in stored order, every product and every
// sum rounded, then the difference (and the product with the inverse pivot).  Without a lower or without an upper sweep z is
// zero and the caller leaves u as it is.
inline void solve_iter(const Factors &F, const double *ftemp, double *utemp, double *ztemp, int lower, int upper)
{
   const int n = F.n;
   const int *perm = F.perm.data();
   for (int i = 0; i < n; i++) { utemp[perm[i]] = 0.0; ztemp[perm[i]] = 0.0; }
   if (lower <= 0 || upper <= 0) { return; }
   for (int kk = 0; kk < lower; kk++)
   {
      for (int i = n - 1; i >= 0; i--)
      {
         double sum = 0.0;
         for (int j = F.Li[(size_t) i]; j < F.Li[(size_t) i + 1]; j++) { sum += F.La[(size_t) j] * utemp[perm[F.Lj[(size_t) j]]]; }
         utemp[perm[i]] = ftemp[perm[i]] - sum;
      }
   }
   for (int kk = 0; kk < upper; kk++)
   {
      for (int i = 0; i < n; i++)
      {
         double sum = 0.0;
         for (int j = F.Ui[(size_t) i]; j < F.Ui[(size_t) i + 1]; j++) { sum += F.Ua[(size_t) j] * ztemp[perm[F.Uj[(size_t) j]]]; }
         ztemp[perm[i]] = F.D[(size_t) i] * (utemp[perm[i]] - sum);
      }
   }
}

// ---- dependency levels of a triangular factor and its rows in level order ----
// T is L (forward: a row waits for the rows its columns name, all before it) or U (backward: all after it).
// order[lev_start[l] .. lev_start[l + 1]) are the rows of level l, ascending inside a level.
struct Levels { std::vector<int> lev_start, order; int nlev = 0; };
inline void build_levels(int n, const int *Ti, const int *Tj, bool forward, Levels &V)
{
   std::vector<int> level((size_t) std::max(n, 1), 0);
   int nlev = n > 0 ? 1 : 0;
   for (int t = 0; t < n; t++)
   {
      const int i = forward ? t : n - 1 - t;
      int lev = 0;
      for (int j = Ti[i]; j < Ti[i + 1]; j++) { lev = std::max(lev, level[(size_t) Tj[j]] + 1); }
      level[(size_t) i] = lev;
      nlev = std::max(nlev, lev + 1);
   }
   V.nlev = nlev;
   V.lev_start.assign((size_t) nlev + 1, 0);
   for (int i = 0; i < n; i++) { V.lev_start[(size_t) level[(size_t) i] + 1]++; }
   for (int l = 0; l < nlev; l++) { V.lev_start[(size_t) l + 1] += V.lev_start[(size_t) l]; }
   std::vector<int> pos(V.lev_start.begin(), V.lev_start.end());
   V.order.assign((size_t) n, 0);
   for (int i = 0; i < n; i++) { V.order[(size_t) pos[(size_t) level[(size_t) i]]++] = i; }
}

// ---- a factor in row slices, the form the device sweeps read ----
// 64 consecutive slots of `order` (the level order: neighbouring rows have alike lengths) make a slice, one per wave.  Inside
// a slice the entries lie entry-major: entry k of lane l at base[slice] + 64 k + l, every row in its stored order, the slice
// as long as its longest row.  len[] stops a short row at its own length: the padding behind it (column 0, value 0) is never
// read, let alone multiplied.  The permutation is folded into row[] and col[]; slots past the last row carry row -1.
constexpr int SLICE_ROWS = 64;
struct Slices
{
   int nslices = 0;
   long long padded = 0;                     // entries of all slices, padding included
   std::vector<long long> base;              // [nslices] first entry of the slice
   std::vector<int> len, row;                // [64 nslices]
   std::vector<double> dinv;                 // [64 nslices] inverse pivot of the slot's row
   std::vector<int> col;                     // [padded]
   std::vector<double> val;                  // [padded]
};
inline void build_slices(const Factors &F, const std::vector<int> &order, const std::vector<int> &Ti, const std::vector<int> &Tj,
                         const std::vector<double> &Ta, Slices &M)
{
   const int n = F.n;
   M.nslices = (n + SLICE_ROWS - 1) / SLICE_ROWS;
   const size_t slots = (size_t) M.nslices * SLICE_ROWS;
   M.base.assign((size_t) M.nslices, 0);
   M.len.assign(slots, 0); M.row.assign(slots, -1); M.dinv.assign(slots, 0.0);
   M.padded = 0;
   for (int s = 0; s < M.nslices; s++)
   {
      int longest = 0;
      for (int l = 0; l < SLICE_ROWS && s * SLICE_ROWS + l < n; l++)
      {
         const int r = order[(size_t) s * SLICE_ROWS + (size_t) l];
         longest = std::max(longest, Ti[(size_t) r + 1] - Ti[(size_t) r]);
      }
      M.base[(size_t) s] = M.padded;
      M.padded += (long long) longest * SLICE_ROWS;
   }
   M.col.assign((size_t) M.padded, 0); M.val.assign((size_t) M.padded, 0.0);
   for (int t = 0; t < n; t++)
   {
      const int r = order[(size_t) t], s = t / SLICE_ROWS, l = t % SLICE_ROWS, first = Ti[(size_t) r];
      M.row[(size_t) t] = F.perm[(size_t) r];
      M.len[(size_t) t] = Ti[(size_t) r + 1] - first;
      M.dinv[(size_t) t] = F.D[(size_t) r];
      for (int k = 0; k < M.len[(size_t) t]; k++)
      {
         const size_t at = (size_t) M.base[(size_t) s] + (size_t) k * SLICE_ROWS + (size_t) l;
         M.col[at] = F.perm[(size_t) Tj[(size_t) first + (size_t) k]];
         M.val[at] = Ta[(size_t) first + (size_t) k];
      }
   }
}

}  // namespace ilu
}  // namespace hamd
