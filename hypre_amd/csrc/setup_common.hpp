// hypre_amd — the steps the builders of the BoomerAMG setup share (par_amg_setup.cpp: single rank; par_amg_setup_dist.cpp:
// several ranks; host loops and device kernels in both).  The host and the device builder of one operator go through the
// same bookkeeping here, so that their results stay equal array for array and a change to how P or RAP is assembled is
// made once.  The first half needs nothing but the matrix structs (tests/host/setup_common_check.cpp runs it under the
// address and undefined-behaviour sanitizers); the second half owns communication packages and device memory.
#pragma once
#include "amg_internal.hpp"
#include <algorithm>
#include <cstring>

#pragma GCC visibility push(hidden)
namespace hamd {

// ---------------------------------------------------------------------------
// rows of a matrix built by several threads
// ---------------------------------------------------------------------------
// contiguous row chunk of thread t out of T
inline void chunk(int n, int T, int t, int *b, int *e)
{
   const long long per = n / T, rest = n % T;
   *b = (int) (t * per + std::min<long long>(t, rest));
   *e = (int) (*b + per + (t < rest ? 1 : 0));
}

// One contiguous block of the n rows per thread (chunk()); a thread appends the entries of its rows to its own vectors —
// one pair for a matrix of one block, two for diag + offd — and notes every row's lengths in di / oi [row + 1].  After the
// loop offsets() turns the lengths into row offsets and stitch() copies every thread's entries to where its first row
// starts.  The result does not depend on T.
struct RowBlocks
{
   struct Out { std::vector<HYPRE_Int> j; std::vector<HYPRE_Real> a; };
   const HYPRE_Int  n;
   const int        T;
   std::vector<Out> diag, offd;                 // [T]
   std::vector<HYPRE_Int> di, oi;               // [n + 1] (oi: two blocks only)
   RowBlocks(HYPRE_Int n_, int T_, bool two_blocks)
      : n(n_), T(std::max(T_, 1)), diag((size_t) T), offd(two_blocks ? (size_t) T : 0), di((size_t) n_ + 1, 0),
        oi(two_blocks ? (size_t) n_ + 1 : 0, 0) {}
   void rows_of(int t, HYPRE_Int *b, HYPRE_Int *e) const { chunk(n, T, t, b, e); }
   void offsets()
   {
      for (HYPRE_Int i = 0; i < n; i++) { di[(size_t) i + 1] += di[(size_t) i]; }
      for (HYPRE_Int i = 0; i < n && !oi.empty(); i++) { oi[(size_t) i + 1] += oi[(size_t) i]; }
   }
   HYPRE_Int nnz_diag() const { return di[(size_t) n]; }
   HYPRE_Int nnz_offd() const { return oi.empty() ? 0 : oi[(size_t) n]; }
   // into the allocated blocks of the matrix (O: the second block, when there are two)
   void stitch(hypre_CSRMatrix *D, hypre_CSRMatrix *O = nullptr) const
   {
      memcpy(D->i, di.data(), sizeof(HYPRE_Int) * ((size_t) n + 1));
      if (O) { memcpy(O->i, oi.data(), sizeof(HYPRE_Int) * ((size_t) n + 1)); }
#pragma omp parallel for num_threads(T) schedule(static, 1)
      for (int t = 0; t < T; t++)
      {
         HYPRE_Int rb, re;
         rows_of(t, &rb, &re);
         place(diag[(size_t) t], D, (size_t) di[(size_t) rb]);
         if (O) { place(offd[(size_t) t], O, (size_t) oi[(size_t) rb]); }
      }
   }
private:
   static void place(const Out &o, hypre_CSRMatrix *M, size_t at)
   {
      if (o.j.empty()) { return; }
      memcpy(M->j + at, o.j.data(), sizeof(HYPRE_Int) * o.j.size());
      memcpy(M->data + at, o.a.data(), sizeof(HYPRE_Real) * o.a.size());
   }
};

// ---------------------------------------------------------------------------
// sorted lists of global ids and positions in them
// ---------------------------------------------------------------------------
inline void sort_unique(std::vector<HYPRE_BigInt> &v)
{
   std::sort(v.begin(), v.end());
   v.erase(std::unique(v.begin(), v.end()), v.end());
}
// position of v in the ascending list, or -1
inline HYPRE_Int bsearch_big(const HYPRE_BigInt *list, HYPRE_BigInt v, HYPRE_Int n)
{
   const HYPRE_BigInt *p = std::lower_bound(list, list + n, v);
   return (p != list + n && *p == v) ? (HYPRE_Int) (p - list) : -1;
}
// positions of ids[0 .. n) in the ascending list (at least one slot, so that .data() can be handed on)
inline std::vector<HYPRE_Int> positions_in(const std::vector<HYPRE_BigInt> &list, const HYPRE_BigInt *ids, size_t n)
{
   std::vector<HYPRE_Int> pos(std::max<size_t>(n, 1));
   for (size_t k = 0; k < n; k++) { pos[k] = bsearch_big(list.data(), ids[k], (HYPRE_Int) list.size()); }
   return pos;
}

// Column map of an off-rank block that uses some of n_ghost ghost columns (aux_interp.c:777-900, par_interp.c:2370-2440,
// par_csr_filter.c): the global ids of the ghosts in use, ascending, and for every ghost in use its position among them.
struct GhostCompaction
{
   std::vector<HYPRE_BigInt> cmap;
   std::vector<HYPRE_Int>    renum;             // [n_ghost], -1: not in use
};
template <class Flag>
GhostCompaction compact_ghosts(const Flag *used, const HYPRE_BigInt *global_id, HYPRE_Int n_ghost)
{
   GhostCompaction c;
   for (HYPRE_Int g = 0; g < n_ghost; g++) { if (used[g]) { c.cmap.push_back(global_id[g]); } }
   sort_unique(c.cmap);
   c.renum.assign((size_t) std::max(n_ghost, 1), -1);
   for (HYPRE_Int g = 0; g < n_ghost; g++)
   {
      if (used[g]) { c.renum[(size_t) g] = bsearch_big(c.cmap.data(), global_id[g], (HYPRE_Int) c.cmap.size()); }
   }
   return c;
}
// the same for columns on the host: j[0 .. nnz) is renumbered in place, the column map comes back
inline std::vector<HYPRE_BigInt> compact_offd_columns(HYPRE_Int *j, size_t nnz, const HYPRE_BigInt *global_id, HYPRE_Int n_ghost)
{
   std::vector<char> used((size_t) std::max(n_ghost, 1), 0);
   for (size_t k = 0; k < nnz; k++) { used[(size_t) j[k]] = 1; }
   GhostCompaction c = compact_ghosts(used.data(), global_id, n_ghost);
   for (size_t k = 0; k < nnz; k++) { j[k] = c.renum[(size_t) j[k]]; }
   return std::move(c.cmap);
}

// ---------------------------------------------------------------------------
// Galerkin product over several ranks: what arrives from the neighbours (par_rap.c:300-700)
// ---------------------------------------------------------------------------
// rows of variable length as they travel through a comm package
struct ExtCSR
{
   std::vector<HYPRE_Int>    i;       // [nrows+1]
   std::vector<HYPRE_BigInt> j;       // global column ids (or encoded local/ghost ids later)
   std::vector<HYPRE_Real>   a;       // may stay empty
   HYPRE_Int nrows() const { return (HYPRE_Int) i.size() - 1; }
};

// P_ext: the rows of P for A's ghost columns, split into the part with local coarse columns (dj: local numbers) and the
// part with off-rank ones (oj: positions in cmap).  cmap holds the off-rank coarse columns of P_ext and of P itself,
// ascending; mapP2Pext takes a ghost column of P there.
struct PExt
{
   std::vector<HYPRE_Int>    di, dj, oi, oj;
   std::vector<HYPRE_Real>   da, oa;
   std::vector<HYPRE_BigInt> cmap;
   std::vector<HYPRE_Int>    mapP2Pext;
   HYPRE_Int ncols_offd() const { return (HYPRE_Int) cmap.size(); }
};
inline PExt split_P_ext(const ExtCSR &Ps, HYPRE_Int ncoA, HYPRE_BigInt first_c, HYPRE_Int ncP, const HYPRE_BigInt *col_map_P, HYPRE_Int ncoP)
{
   PExt e;
   const HYPRE_BigInt last_c = first_c + ncP - 1;
   e.di.assign((size_t) ncoA + 1, 0); e.oi.assign((size_t) ncoA + 1, 0);
   std::vector<HYPRE_BigInt> big;
   for (HYPRE_Int i = 0; i < ncoA; i++)
   {
      for (HYPRE_Int k = Ps.i[(size_t) i]; k < Ps.i[(size_t) i + 1]; k++)
      {
         const HYPRE_BigInt g = Ps.j[(size_t) k];
         if (g < first_c || g > last_c) { big.push_back(g); e.oa.push_back(Ps.a[(size_t) k]); }
         else { e.dj.push_back((HYPRE_Int) (g - first_c)); e.da.push_back(Ps.a[(size_t) k]); }
      }
      e.di[(size_t) i + 1] = (HYPRE_Int) e.dj.size();
      e.oi[(size_t) i + 1] = (HYPRE_Int) big.size();
   }
   for (HYPRE_BigInt g : big) { e.cmap.push_back(g); }
   for (HYPRE_Int k = 0; k < ncoP; k++) { e.cmap.push_back(col_map_P[k]); }
   sort_unique(e.cmap);
   e.oj = positions_in(e.cmap, big.data(), big.size());
   if (big.empty()) { e.oj.clear(); }
   e.mapP2Pext = positions_in(e.cmap, col_map_P, (size_t) ncoP);
   return e;
}

// The rows of the product the neighbours computed for this rank (Rext: one per entry of RT's send list, global columns).
// cmap: the off-rank columns of the product (those of the received rows and of P_ext), ascending; xj: the received rows'
// columns as local coarse number, or ncP + position in cmap; Fi / Fj: per local coarse row the received rows that feed it,
// in package order; max_seed: the most received entries any coarse row starts from.
struct RapExt
{
   std::vector<HYPRE_BigInt> cmap;
   std::vector<HYPRE_Int>    mapPext2RAP, xj, Fi, Fj;
   int                       max_seed = 0;
   HYPRE_Int ncols_offd() const { return (HYPRE_Int) cmap.size(); }
};
inline RapExt number_received_rows(const ExtCSR &Rext, const PExt &Pe, HYPRE_BigInt first_c, HYPRE_Int ncP, HYPRE_Int ncRT,
                                   const HYPRE_Int *send_map_elmts, HYPRE_Int nsend)
{
   RapExt r;
   const HYPRE_BigInt last_c = first_c + ncP - 1;
   for (HYPRE_BigInt g : Rext.j) { if (g < first_c || g > last_c) { r.cmap.push_back(g); } }
   for (HYPRE_BigInt g : Pe.cmap) { r.cmap.push_back(g); }
   sort_unique(r.cmap);
   r.mapPext2RAP = positions_in(r.cmap, Pe.cmap.data(), Pe.cmap.size());
   r.xj.assign(Rext.j.size(), 0);
   for (size_t k = 0; k < Rext.j.size(); k++)
   {
      const HYPRE_BigInt g = Rext.j[k];
      r.xj[k] = (g < first_c || g > last_c) ? ncP + bsearch_big(r.cmap.data(), g, r.ncols_offd()) : (HYPRE_Int) (g - first_c);
   }
   r.Fi.assign((size_t) ncRT + 1, 0); r.Fj.assign((size_t) std::max(nsend, 1), 0);
   for (HYPRE_Int s = 0; s < nsend; s++) { r.Fi[(size_t) send_map_elmts[s] + 1]++; }
   for (HYPRE_Int ic = 0; ic < ncRT; ic++) { r.Fi[(size_t) ic + 1] += r.Fi[(size_t) ic]; }
   std::vector<HYPRE_Int> pos(r.Fi.begin(), r.Fi.end() - 1), seed((size_t) std::max(ncRT, 1), 0);
   for (HYPRE_Int s = 0; s < nsend; s++)
   {
      const HYPRE_Int ic = send_map_elmts[s];
      r.Fj[(size_t) pos[(size_t) ic]++] = s;
      seed[(size_t) ic] += Rext.i[(size_t) s + 1] - Rext.i[(size_t) s];
      r.max_seed = std::max(r.max_seed, (int) seed[(size_t) ic]);
   }
   return r;
}

// ===========================================================================
// from here on: communication packages and device memory
// ===========================================================================
inline int comm_size(MPI_Comm c) { HYPRE_Int n; hypre_MPI_Comm_size(c, &n); return n; }
inline int comm_rank(MPI_Comm c) { HYPRE_Int r; hypre_MPI_Comm_rank(c, &r); return r; }

template <class T> struct HaloJob;
template <> struct HaloJob<double>       { static constexpr int fwd = 1,  rev = 2; };
template <> struct HaloJob<HYPRE_Int>    { static constexpr int fwd = 11, rev = 12; };
template <> struct HaloJob<HYPRE_BigInt> { static constexpr int fwd = 21; };      // ghost -> owner is never needed for indices

// owner values -> ghost array (offd column order)
template <class T>
void halo_forward(hypre_ParCSRCommPkg *pkg, const T *local, T *ghost)
{
   if (!pkg) { return; }
   const HYPRE_Int tot = pkg->send_map_starts[pkg->num_sends];
   std::vector<T> buf((size_t) std::max(tot, 1));
   for (HYPRE_Int k = 0; k < tot; k++) { buf[(size_t) k] = local[pkg->send_map_elmts[k]]; }
   hypre_ParCSRCommHandle *h = hypre_ParCSRCommHandleCreate(HaloJob<T>::fwd, pkg, buf.data(), ghost);
   hypre_ParCSRCommHandleDestroy(h);
}
// ghost values -> owners' buffer laid out like send_map_elmts
template <class T>
void halo_reverse(hypre_ParCSRCommPkg *pkg, const T *ghost, T *buf)
{
   if (!pkg) { return; }
   hypre_ParCSRCommHandle *h = hypre_ParCSRCommHandleCreate(HaloJob<T>::rev, pkg, (void *) ghost, buf);
   hypre_ParCSRCommHandleDestroy(h);
}

// A comm package of A's layout for ghost points A itself does not have (the new off-rank nodes of extended+i
// interpolation, aux_interp.c:560-640), alive as long as this object.  Collective: every rank builds one, possibly empty.
struct ExtPkg
{
   hypre_ParCSRCommPkg pkg;
   ExtPkg(hypre_ParCSRMatrix *A, const std::vector<HYPRE_BigInt> &ghost_ids)
   {
      memset(&pkg, 0, sizeof(pkg));
      pkg.comm = A->comm;
      hypre_ParCSRCommPkgCreate_core(A->comm, ghost_ids.empty() ? nullptr : const_cast<HYPRE_BigInt *>(ghost_ids.data()),
                                     A->first_col_diag, A->col_starts, A->diag->num_cols, (HYPRE_Int) ghost_ids.size(),
                                     &pkg.num_recvs, &pkg.recv_procs, &pkg.recv_vec_starts, &pkg.num_sends, &pkg.send_procs,
                                     &pkg.send_map_starts, &pkg.send_map_elmts);
   }
   ExtPkg(const ExtPkg &) = delete;
   ExtPkg &operator=(const ExtPkg &) = delete;
   ~ExtPkg()
   {
      hypre_Free(pkg.recv_procs, HYPRE_MEMORY_HOST); hypre_Free(pkg.recv_vec_starts, HYPRE_MEMORY_HOST);
      hypre_Free(pkg.send_procs, HYPRE_MEMORY_HOST); hypre_Free(pkg.send_map_starts, HYPRE_MEMORY_HOST);
      hypre_Free(pkg.send_map_elmts, HYPRE_MEMORY_HOST);
   }
};

// the column map of M's off-rank block becomes cmap
inline void set_col_map_offd(hypre_ParCSRMatrix *M, const std::vector<HYPRE_BigInt> &cmap)
{
   M->offd->num_cols = (HYPRE_Int) cmap.size();
   if (M->col_map_offd) { hypre_Free(M->col_map_offd, HYPRE_MEMORY_HOST); M->col_map_offd = nullptr; }
   if (cmap.empty()) { return; }
   M->col_map_offd = hypre_TAlloc(HYPRE_BigInt, cmap.size(), HYPRE_MEMORY_HOST);
   memcpy(M->col_map_offd, cmap.data(), sizeof(HYPRE_BigInt) * cmap.size());
}

// An owning pointer to device memory.  What a kernel launcher hands back through an out-parameter (&buf.p) belongs to the
// buffer from then on: it is freed on every way out of the scope unless release() gave it to a matrix.
template <class T>
struct DevBuf
{
   T *p = nullptr;
   DevBuf() = default;
   explicit DevBuf(T *q) : p(q) {}
   DevBuf(DevBuf &&o) noexcept : p(o.release()) {}
   DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
   DevBuf(const DevBuf &) = delete;
   DevBuf &operator=(const DevBuf &) = delete;
   ~DevBuf() { reset(); }
   operator T *() const { return p; }
   T   *release() { T *q = p; p = nullptr; return q; }
   void reset() { if (p) { HIP_CHECK(hipFree(p)); p = nullptr; } }
};
// n items (at least one) of device memory
template <class T>
DevBuf<T> dev_alloc(size_t n)
{
   DevBuf<T> d;
   HIP_CHECK(hipMalloc((void **) &d.p, sizeof(T) * std::max<size_t>(n, 1)));
   return d;
}
template <class T>
DevBuf<T> upload(const T *h, size_t n)
{
   DevBuf<T> d = dev_alloc<T>(n);
   if (n) { hypre_Memcpy(d.p, h, sizeof(T) * n, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST); }
   return d;
}
// device -> host, n items.  The pages of a large destination are touched by all threads first (a copy into untouched
// memory faults them in one by one on one thread: 1.8 GB took 0.4 s that way)
template <class T>
void fetch(T *h, const T *d, size_t n)
{
   const size_t bytes = sizeof(T) * n;
   if (bytes > (size_t) 1 << 24)
   {
      char *p = (char *) h;
#pragma omp parallel for schedule(static)
      for (long long o = 0; o < (long long) bytes; o += 4096) { p[o] = 0; }
   }
   hypre_Memcpy(h, d, bytes, HYPRE_MEMORY_HOST, HYPRE_MEMORY_DEVICE);
}

// the three arrays of a CSR block as the kernel launchers return them (&b.i.p, &b.j.p, &b.a.p, &b.nnz)
struct DevCSRBlock
{
   DevBuf<int>    i, j;
   DevBuf<double> a;
   int            nnz = 0;
};
// M, as hypre_ParCSRMatrixCreate left it, takes the device arrays for its diag block (and its offd block; without one the
// offd block stays an empty host block).  The blocks give their arrays away.
inline void adopt_device_blocks(hypre_ParCSRMatrix *M, DevCSRBlock &diag, DevCSRBlock *offd = nullptr)
{
   auto adopt = [](hypre_CSRMatrix *&blk, DevCSRBlock &b)
   {
      const HYPRE_Int nr = blk->num_rows, nc = blk->num_cols;
      hypre_CSRMatrixDestroy(blk);
      blk = setup_wrap_device_csr(nr, nc, b.nnz, b.i.release(), b.j.release(), b.a.release());
   };
   adopt(M->diag, diag);
   if (offd) { adopt(M->offd, *offd); }
   else { hypre_CSRMatrixInitialize_v2(M->offd, 0, HYPRE_MEMORY_HOST); }
}

}  // namespace hamd
#pragma GCC visibility pop
