// Stand-alone check of the host-only half of hypre_amd/csrc/setup_common.hpp (RowBlocks, the sorted-unique lists and
// their index maps, compact_offd_columns, the P_ext split and the numbering of received product rows) against
// straightforward sequential code, on edge cases: no rows, no ghosts, more threads than rows, one ghost used by every row,
// no ghost used.  Built with -fsanitize=address,undefined by tests/test_setup_common_host.py; needs no device and does not
// link the library.
#include "setup_common.hpp"
#include <cstdio>
#include <cstdlib>

using namespace hamd;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static unsigned rng_state = 12345u;
static unsigned rnd(unsigned m) { rng_state = rng_state * 1664525u + 1013904223u; return m ? (rng_state >> 8) % m : 0; }

struct HostCSR
{
   std::vector<HYPRE_Int> i, j; std::vector<HYPRE_Real> a;
   hypre_CSRMatrix m{};
   HostCSR(HYPRE_Int n, HYPRE_Int nnz) : i((size_t) n + 1, -7), j((size_t) nnz, -7), a((size_t) nnz, -7.0)
   {
      m.i = i.data(); m.j = j.data(); m.data = a.data(); m.num_rows = n; m.num_nonzeros = nnz;
   }
};

// rows of random length (some empty) into two blocks, by T "threads" and in one sequential pass
static void check_row_blocks(HYPRE_Int n, int T, bool two)
{
   std::vector<std::vector<HYPRE_Int>> dj((size_t) n), oj((size_t) n);
   for (HYPRE_Int r = 0; r < n; r++)
   {
      for (unsigned k = rnd(5); k > 0; k--) { dj[(size_t) r].push_back((HYPRE_Int) rnd(1000)); }
      for (unsigned k = two ? rnd(3) : 0; k > 0; k--) { oj[(size_t) r].push_back((HYPRE_Int) rnd(1000)); }
   }
   RowBlocks rows(n, T, two);
   CHECK(rows.T >= 1);
   HYPRE_Int covered = 0;
   for (int t = 0; t < rows.T; t++)
   {
      HYPRE_Int rb, re;
      rows.rows_of(t, &rb, &re);
      CHECK(rb == covered && re >= rb);
      covered = re;
      for (HYPRE_Int r = rb; r < re; r++)
      {
         for (HYPRE_Int c : dj[(size_t) r]) { rows.diag[(size_t) t].j.push_back(c); rows.diag[(size_t) t].a.push_back(0.5 * c); }
         rows.di[(size_t) r + 1] = (HYPRE_Int) dj[(size_t) r].size();
         if (two)
         {
            for (HYPRE_Int c : oj[(size_t) r]) { rows.offd[(size_t) t].j.push_back(c); rows.offd[(size_t) t].a.push_back(0.25 * c); }
            rows.oi[(size_t) r + 1] = (HYPRE_Int) oj[(size_t) r].size();
         }
      }
   }
   CHECK(covered == n);
   rows.offsets();
   HostCSR D(n, rows.nnz_diag()), O(n, rows.nnz_offd());
   rows.stitch(&D.m, two ? &O.m : nullptr);
   HYPRE_Int kd = 0, ko = 0;
   for (HYPRE_Int r = 0; r < n; r++)
   {
      CHECK(D.i[(size_t) r] == kd);
      for (HYPRE_Int c : dj[(size_t) r]) { CHECK(D.j[(size_t) kd] == c && D.a[(size_t) kd] == 0.5 * c); kd++; }
      if (two)
      {
         CHECK(O.i[(size_t) r] == ko);
         for (HYPRE_Int c : oj[(size_t) r]) { CHECK(O.j[(size_t) ko] == c && O.a[(size_t) ko] == 0.25 * c); ko++; }
      }
   }
   CHECK(D.i[(size_t) n] == kd && rows.nnz_diag() == kd && rows.nnz_offd() == ko);
   if (two) { CHECK(O.i[(size_t) n] == ko); }
}

static void check_compaction(HYPRE_Int n_ghost, const std::vector<HYPRE_Int> &cols, const std::vector<HYPRE_BigInt> &gid)
{
   std::vector<HYPRE_Int> j(cols);
   const std::vector<HYPRE_BigInt> cmap = compact_offd_columns(j.data(), j.size(), gid.data(), n_ghost);
   for (size_t k = 1; k < cmap.size(); k++) { CHECK(cmap[k - 1] < cmap[k]); }
   for (size_t k = 0; k < cols.size(); k++)
   {
      CHECK(j[k] >= 0 && (size_t) j[k] < cmap.size());
      if (j[k] >= 0 && (size_t) j[k] < cmap.size()) { CHECK(cmap[(size_t) j[k]] == gid[(size_t) cols[k]]); }
   }
   // nothing in the map that no column uses
   for (HYPRE_BigInt g : cmap)
   {
      bool seen = false;
      for (HYPRE_Int c : cols) { seen = seen || gid[(size_t) c] == g; }
      CHECK(seen);
   }
   if (cols.empty()) { CHECK(cmap.empty()); }
}

static ExtCSR random_rows(HYPRE_Int nrows, HYPRE_BigInt lo, HYPRE_BigInt hi, unsigned max_len)
{
   ExtCSR e;
   e.i.assign((size_t) nrows + 1, 0);
   for (HYPRE_Int r = 0; r < nrows; r++)
   {
      for (unsigned k = rnd(max_len + 1); k > 0; k--) { e.j.push_back(lo + (HYPRE_BigInt) rnd((unsigned) (hi - lo))); e.a.push_back(1.0 + (double) e.j.size()); }
      e.i[(size_t) r + 1] = (HYPRE_Int) e.j.size();
   }
   return e;
}

// P_ext of ncoA ghost rows with global columns in [0, 60), local coarse range [first_c, first_c + ncP), P's own ghost columns
// col_map_P; then the rows received for ncRT coarse rows through a send list
static void check_product_numbering(HYPRE_Int ncoA, HYPRE_BigInt first_c, HYPRE_Int ncP, const std::vector<HYPRE_BigInt> &col_map_P,
                                    HYPRE_Int ncRT, const std::vector<HYPRE_Int> &send_map)
{
   const HYPRE_BigInt last_c = first_c + ncP - 1;
   const ExtCSR Ps = random_rows(ncoA, 0, 60, 6);
   const PExt Pe = split_P_ext(Ps, ncoA, first_c, ncP, col_map_P.data(), (HYPRE_Int) col_map_P.size());
   CHECK((HYPRE_Int) Pe.di.size() == ncoA + 1 && (HYPRE_Int) Pe.oi.size() == ncoA + 1);
   for (size_t k = 1; k < Pe.cmap.size(); k++) { CHECK(Pe.cmap[k - 1] < Pe.cmap[k]); }
   for (HYPRE_BigInt g : Pe.cmap) { CHECK(g < first_c || g > last_c); }
   for (HYPRE_Int i = 0; i < ncoA; i++)
   {
      HYPRE_Int kd = Pe.di[(size_t) i], ko = Pe.oi[(size_t) i];
      for (HYPRE_Int k = Ps.i[(size_t) i]; k < Ps.i[(size_t) i + 1]; k++)
      {
         const HYPRE_BigInt g = Ps.j[(size_t) k];
         if (g < first_c || g > last_c) { CHECK(Pe.cmap[(size_t) Pe.oj[(size_t) ko]] == g && Pe.oa[(size_t) ko] == Ps.a[(size_t) k]); ko++; }
         else { CHECK(Pe.dj[(size_t) kd] == (HYPRE_Int) (g - first_c) && Pe.da[(size_t) kd] == Ps.a[(size_t) k]); kd++; }
      }
      CHECK(kd == Pe.di[(size_t) i + 1] && ko == Pe.oi[(size_t) i + 1]);
   }
   CHECK(Pe.oj.size() == Pe.oa.size() && Pe.dj.size() == Pe.da.size());
   for (size_t k = 0; k < col_map_P.size(); k++) { CHECK(Pe.cmap[(size_t) Pe.mapP2Pext[k]] == col_map_P[k]); }

   const HYPRE_Int nsend = (HYPRE_Int) send_map.size();
   const ExtCSR Rext = random_rows(nsend, 0, 80, 5);
   const RapExt Rx = number_received_rows(Rext, Pe, first_c, ncP, ncRT, send_map.data(), nsend);
   for (size_t k = 1; k < Rx.cmap.size(); k++) { CHECK(Rx.cmap[k - 1] < Rx.cmap[k]); }
   for (size_t k = 0; k < Pe.cmap.size(); k++) { CHECK(Rx.cmap[(size_t) Rx.mapPext2RAP[k]] == Pe.cmap[k]); }
   CHECK(Rx.xj.size() == Rext.j.size());
   for (size_t k = 0; k < Rext.j.size(); k++)
   {
      const HYPRE_BigInt g = Rext.j[k];
      if (g < first_c || g > last_c) { CHECK(Rx.xj[k] >= ncP && Rx.cmap[(size_t) (Rx.xj[k] - ncP)] == g); }
      else { CHECK(Rx.xj[k] == (HYPRE_Int) (g - first_c)); }
   }
   // the feed lists against vectors of lists filled in package order
   std::vector<std::vector<HYPRE_Int>> feeds((size_t) std::max(ncRT, 1));
   for (HYPRE_Int s = 0; s < nsend; s++) { feeds[(size_t) send_map[(size_t) s]].push_back(s); }
   int max_seed = 0;
   CHECK((HYPRE_Int) Rx.Fi.size() == ncRT + 1 && Rx.Fi[0] == 0);
   for (HYPRE_Int ic = 0; ic < ncRT; ic++)
   {
      const std::vector<HYPRE_Int> &f = feeds[(size_t) ic];
      CHECK(Rx.Fi[(size_t) ic + 1] - Rx.Fi[(size_t) ic] == (HYPRE_Int) f.size());
      int seed = 0;
      for (size_t q = 0; q < f.size(); q++)
      {
         CHECK(Rx.Fj[(size_t) Rx.Fi[(size_t) ic] + q] == f[q]);
         seed += Rext.i[(size_t) f[q] + 1] - Rext.i[(size_t) f[q]];
      }
      max_seed = std::max(max_seed, seed);
   }
   CHECK(Rx.max_seed == max_seed);
}

int main()
{
   for (bool two : {false, true})
   {
      check_row_blocks(0, 1, two);             // no rows
      check_row_blocks(0, 4, two);
      check_row_blocks(3, 8, two);             // threads with an empty block
      check_row_blocks(1, 1, two);
      check_row_blocks(37, 1, two);
      check_row_blocks(37, 5, two);
      check_row_blocks(64, 8, two);
      check_row_blocks(5, 0, two);             // a thread-count rule that comes out at zero
   }
   // sorted-unique lists and positions in them
   {
      std::vector<HYPRE_BigInt> v = {9, 3, 9, 3, 100, -4};
      sort_unique(v);
      CHECK((v == std::vector<HYPRE_BigInt>{-4, 3, 9, 100}));
      const HYPRE_BigInt ids[3] = {100, 5, -4};
      const std::vector<HYPRE_Int> pos = positions_in(v, ids, 3);
      CHECK(pos[0] == 3 && pos[1] == -1 && pos[2] == 0);
      std::vector<HYPRE_BigInt> none;
      sort_unique(none);
      CHECK(positions_in(none, ids, 0).size() == 1 && bsearch_big(none.data(), 7, 0) == -1);
   }
   check_compaction(0, {}, {});                                          // no ghosts
   check_compaction(4, {}, {40, 10, 30, 20});                            // no ghost used
   check_compaction(4, {2, 2, 2, 2, 2}, {40, 10, 30, 20});               // one ghost used by every row
   check_compaction(5, {4, 0, 3, 0, 1}, {50, 10, 70, 10, 5});            // ids out of order, two ghosts with one id
   check_compaction(3, {0, 1, 2, 1}, {7, 8, 9});                         // ascending already: order kept
   {
      std::vector<HYPRE_Int> j = {0, 1, 2, 1};
      const HYPRE_BigInt gid[3] = {7, 8, 9};
      compact_offd_columns(j.data(), j.size(), gid, 3);
      CHECK((j == std::vector<HYPRE_Int>{0, 1, 2, 1}));
   }
   check_product_numbering(0, 20, 10, {}, 0, {});                        // nothing at all
   check_product_numbering(0, 20, 10, {3, 45}, 4, {});                   // no ghost rows, nothing received
   check_product_numbering(7, 20, 10, {}, 5, {4, 0, 4, 2});              // P without ghost columns
   check_product_numbering(9, 20, 10, {3, 45, 59}, 6, {5, 5, 5, 0, 1, 5, 3});
   check_product_numbering(6, 0, 60, {}, 3, {2, 1, 0});                  // every column local
   check_product_numbering(6, 70, 5, {1, 2}, 3, {0, 0});                 // every column off rank
   if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
   printf("setup_common host checks passed\n");
   return 0;
}
