"""Hybrid Gauss-Seidel / SOR kernels (gs_kernels.hip, par_relax_gs.cpp; relax 3, 4, 6, 8, 13, 14, 88, 89) against the
oracle's in-order row loop (oracle.c hybrid_gs_core), bit for bit: every comparison in this file is np.array_equal on the
int64 views of the two vectors, there is no tolerance.

What the matrices are built to reach, and how a case knows that it did: every case works out the dependency levels of its
matrix (per emulated thread block), the lane width (cuts at 4.5, 9 and 18 entries a row) and, by the rule documented in
par_relax_gs.cpp (a level of at most 1024 / lanes rows joins a run of at most 12288 levels, a larger level gets a grid of
its own), the launches of gs_run_kernel and gs_level_kernel it expects, and asserts all four against
hypre_amd_GsSweepStats.

* stripe matrices, one per lane width G (small = 1024 / G): rows of stripe s couple to stripes s-1 and s+1 only, so with
  one block the levels are the stripes.  Widths [1, small-1, small, small+1, 3, 2 small+5, 1, 1, small+1, small, 7]: a run,
  the run / grid boundary from both sides, a grid that is no multiple of the workgroup, a run between two grids, a one-row
  level right after a large one, a trailing run.  Off-diagonal counts cycle through 0 (row 0 only), 1, G-1, G, G+1, 2G-1,
  2G, 2G+1 (and 3G+1 at 32 lanes: past the two chunks the 32-lane groups fetch ahead), capped by what the two neighbouring
  stripes can supply.  Departures from those widths: the 8-lane matrix ends with a stripe of 8 rows so that 3 and 7 do not
  divide its row count (the thread-block cases want an uneven split); the 32-lane matrix gets four more stripes
  [100, 45, 100, 3], because none of the large levels above has 97 neighbours to draw from: the 45-row level (a grid at 32
  lanes) has 200; and its stripe of 7 rows has 9, so that this level, which stays in a run, cycles through all the counts.
* the 16^3 7-point grid (8 lanes, 46 levels, up to 192 rows), an 8x8 5-point grid (4.5 entries a row exactly: 4 lanes) and
  a tridiagonal chain of 2 * 12288 + 3 rows (one row per level: three runs a direction, the 49 KB of level offsets in LDS).
* a 700-row matrix with columns anywhere and a pattern that is not symmetric: the one shape in which a row reads a row that
  comes after it in the sweep but is already final in u (it sits in an earlier level), so the copy of u from the start of
  the directional sweep is not just another name for u.
* a 100-row chain whose rows at the cut of the uneven split (p = 3, 7, 8) also read one column past the far end of the
  neighbouring block: on the other matrices no row holds exactly that column, so an edge of the block that is off by one
  row there (`i <= cut` for `i < cut` in gs_block_of) would go unseen.
* emulated threads p in {2, 3, 7, n} (5 as well on the chain, whose row count 3 divides), and n + 5 on the 8x8 grid for the
  clamp to the row count; with p = n every row is its own block and the sweep is a Jacobi-like update from Vtemp.
* rows with a zero diagonal (relax 3) and a zero l1 value (relax 13): left untouched, as the oracle leaves them.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from util import rand_vector

pytestmark = pytest.mark.gpu

MAX_RUN = 12288
L1_TYPES = (8, 13, 14, 88, 89)
RELAX_TYPES = [3, 4, 6, 8, 13, 14, 88, 89]
WEIGHTS = [(1.0, 1.0), (0.8, 1.2)]


# ---------------------------------------------------------------------------------------------------------------------
# matrices (numpy only: diagonal first in every row, no empty rows)
# ---------------------------------------------------------------------------------------------------------------------
def stripe_widths(G, last=7, extra=()):
    small = 1024 // G
    return [1, small - 1, small, small + 1, 3, 2 * small + 5, 1, 1, small + 1, small, last] + list(extra)


def stripe_matrix(widths, counts, seed):
    """Rows of stripe s are contiguous; a row holds its diagonal, then, shuffled, columns drawn without repetition from
    stripes s-1 and s+1 only, at least one from each where that stripe exists.  counts: off-diagonal counts to cycle
    through, capped by the pool; counts[0] must be 0 and goes to row 0 only (every other row needs its links), every later
    stripe starts the cycle at counts[1], so a stripe of len(counts) - 1 rows or more sees all of them."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate(([0], np.cumsum(widths)))
    indptr, indices, data = [0], [], []
    assert counts[0] == 0 and widths[0] == 1
    for s, wd in enumerate(widths):
        k = 0 if s == 0 else 1
        prev = np.arange(starts[s - 1], starts[s]) if s > 0 else np.zeros(0, dtype=np.int64)
        nxt = np.arange(starts[s + 1], starts[s + 2]) if s + 1 < len(widths) else np.zeros(0, dtype=np.int64)
        for r in range(starts[s], starts[s + 1]):
            c = counts[k % len(counts)]
            k += 1
            cols = []
            if not (r == 0 and c == 0):
                forced = [int(rng.choice(side)) for side in (prev, nxt) if side.size]
                c = min(max(c, len(forced)), prev.size + nxt.size)
                rest = np.setdiff1d(np.concatenate((prev, nxt)), forced)
                cols = forced + [int(v) for v in rng.choice(rest, c - len(forced), replace=False)]
                rng.shuffle(cols)
            indices += [r] + cols
            data += [rng.uniform(2.0, 3.0)] + list(rng.uniform(-1.0, 1.0, len(cols)))
            indptr.append(len(indices))
    return np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), np.array(data)


def grid_matrix(dims, seed):
    """5- or 7-point pattern of a lexicographic grid, diagonal first then the neighbours in a shuffled order; random values
    (the kernels must not depend on the stencil's -1s cancelling anything)."""
    rng = np.random.default_rng(seed)
    idx = np.arange(int(np.prod(dims))).reshape(dims[::-1])
    indptr, indices, data = [0], [], []
    for r in range(idx.size):
        pos = np.unravel_index(r, idx.shape)
        cols = []
        for ax in range(len(dims)):
            for d in (-1, 1):
                q = list(pos)
                q[ax] += d
                if 0 <= q[ax] < idx.shape[ax]:
                    cols.append(int(idx[tuple(q)]))
        rng.shuffle(cols)
        indices += [r] + cols
        data += [rng.uniform(2.0, 3.0)] + list(rng.uniform(-1.0, 1.0, len(cols)))
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), np.array(data)


def chain_matrix(n, seed):
    rng = np.random.default_rng(seed)
    rows = np.arange(n)
    cnt = np.full(n, 3)
    cnt[0] = cnt[-1] = 2
    indptr = np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)
    indices = np.empty(indptr[-1], dtype=np.int32)
    indices[indptr[:-1]] = rows
    indices[indptr[1:-1] + 1] = rows[1:] - 1               # rows 1 .. n-1: the left neighbour
    indices[indptr[1:] - 1] = np.where(rows < n - 1, rows + 1, rows - 1)   # the last entry: the right neighbour (last row: left)
    data = rng.uniform(-1.0, 1.0, indptr[-1])
    data[indptr[:-1]] = rng.uniform(2.0, 3.0, n)
    return indptr, indices, data


def oneway_matrix(n, max_off, seed):
    """Columns anywhere, pattern not symmetric: a row may read a row that the sweep reaches after it but that sits in an
    EARLIER level (it does not read back), so that row is already final in u when this one must still see the value from
    the start of the directional sweep."""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for r in range(n):
        cols = rng.choice(np.setdiff1d(np.arange(n), [r]), int(rng.integers(1, max_off + 1)), replace=False)
        indices += [r] + [int(v) for v in cols]
        data += [rng.uniform(2.0, 3.0)] + list(rng.uniform(-1.0, 1.0, len(cols)))
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), np.array(data)


EDGE_N, EDGE_P = 100, (3, 7, 8)


def edge_cut(n, p):
    """first row of the blocks that hold n // p rows (the blocks before it hold one more), and that block's length"""
    size, rest = divmod(n, p)
    return rest * (size + 1), size


def blockedge_matrix(n, ps, seed):
    """A chain in which, for every p of ps (none divides n), the first row of the first SHORT block also reads the first row
    of the block after it, and the last row of the last LONG block the last row of the block before that one (where there
    is one): one column past each end of the blocks on either side of the cut row of the uneven split.  A block edge that
    is off by one there changes which of u, its copy and Vtemp such an entry reads, and nothing else does."""
    indptr, indices, data = chain_matrix(n, seed)
    rng = np.random.default_rng(seed + 1)
    rows = [list(indices[indptr[r]:indptr[r + 1]]) for r in range(n)]
    vals = [list(data[indptr[r]:indptr[r + 1]]) for r in range(n)]
    for p in ps:
        cut, size = edge_cut(n, p)
        for r, c in ((cut, cut + size), (cut - 1, cut - size - 2)):
            if c < 0:                  # one long block only: nothing lies before it
                continue
            assert c < n and 0 < cut < n and c not in rows[r], (p, r, c)
            rows[r].append(c)
            vals[r].append(rng.uniform(-1.0, 1.0))
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    return indptr, np.array(sum(rows, []), dtype=np.int32), np.array(sum(vals, []))


def _build(name):
    if name == "blockedge":
        return blockedge_matrix(EDGE_N, EDGE_P, seed=9), None
    if name == "oneway":
        return oneway_matrix(700, 3, seed=8), None
    if name.startswith("stripe"):
        G = int(name[6:])
        filler = {4: [2] * 10, 8: [4] * 4, 16: [], 32: [3 * G + 1]}[G]
        counts = [0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1] + filler
        widths = stripe_widths(G, last={8: 8, 32: 9}.get(G, 7), extra=(100, 45, 100, 3) if G == 32 else ())
        return stripe_matrix(widths, counts, seed=G), widths
    if name == "grid3d":
        return grid_matrix((16, 16, 16), seed=5), None
    if name == "grid2d":
        return grid_matrix((8, 8), seed=6), None
    assert name == "chain"
    return chain_matrix(2 * MAX_RUN + 3, seed=7), None


# ---------------------------------------------------------------------------------------------------------------------
# the test's own level schedule (a second implementation of build_direction / run_direction)
# ---------------------------------------------------------------------------------------------------------------------
def block_of(n, p, t):
    """rows [s, e) of block t when n rows are dealt to p threads: the first n % p blocks hold one row more"""
    size, rest = divmod(n, p)
    s = t * size + min(t, rest)
    return s, s + size + (1 if t < rest else 0)


def row_levels(indptr, indices, p, forward):
    """dependency level of every row: one more than the deepest row of its own block that it reads and that the sweep has
    reached before it"""
    n = len(indptr) - 1
    ip, ix = indptr.tolist(), indices.tolist()
    level = [0] * n
    for t in range(p):
        s, e = block_of(n, p, t)
        for i in (range(s, e) if forward else range(e - 1, s - 1, -1)):
            lev = 0
            for j in ix[ip[i]:ip[i + 1]]:
                if (s <= j < i) if forward else (i < j < e):
                    lev = max(lev, level[j] + 1)
            level[i] = lev
    return level


def level_sizes(indptr, indices, p, forward):
    """rows per dependency level, all blocks together"""
    return np.bincount(row_levels(indptr, indices, p, forward)).tolist()


def lanes_of(indptr):
    avg = float(indptr[-1]) / (len(indptr) - 1)
    return 4 if avg <= 4.5 else 8 if avg <= 9.0 else 16 if avg <= 18.0 else 32


def launches(sizes, lanes):
    """(run launches, level launches): a level of at most 1024 / lanes rows joins a run of at most MAX_RUN levels, a larger
    one gets a grid"""
    small = 1024 // lanes
    runs = grids = in_run = 0
    for c in sizes:
        if c > small:
            grids += 1
            in_run = 0
        else:
            if in_run == 0 or in_run == MAX_RUN:
                runs += 1
                in_run = 0
            in_run += 1
    return runs, grids


class Case:
    def __init__(self, name, lib, oracle):
        from hypre_amd import binding as B
        (self.indptr, self.indices, self.data), self.widths = _build(name)
        self.name, self.lib, self.oracle = name, lib, oracle
        self.n = n = len(self.indptr) - 1
        assert np.all(self.indices[self.indptr[:-1]] == np.arange(n)) and np.all(np.diff(self.indptr) >= 1)
        self.lanes = lanes_of(self.indptr)
        self.f, self.u0 = rand_vector(n, 3), rand_vector(n, 4)
        rng = np.random.default_rng(11)
        self.l1 = rng.uniform(1.0, 2.0, n)
        self.cf = rng.choice(np.array([-1, 1], dtype=np.int32), n)
        self.d_cf = self._device_ints(self.cf)
        self.d_l1 = B.parvec_from_numpy(self.l1)
        self._mats, self._sizes = {}, {}
        self.par, self.A = self.matrix(self.data)

    def _device_ints(self, a):
        from hypre_amd import binding as B
        a = np.ascontiguousarray(a, dtype=np.int32)
        p = self.lib.hypre_MAlloc(a.nbytes, B.HYPRE_MEMORY_DEVICE)
        self.lib.hypre_Memcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes, B.HYPRE_MEMORY_DEVICE, B.HYPRE_MEMORY_HOST)
        return C.cast(C.c_void_p(p), C.POINTER(C.c_int))

    def matrix(self, data):
        """(oracle matrix, device matrix) of this pattern with the given values"""
        from hypre_amd import binding as B
        n = self.n
        data = np.ascontiguousarray(data, dtype=np.float64)
        par = self.oracle.Par.from_scipy_single(sp.csr_matrix((data, self.indices, self.indptr), shape=(n, n)))
        part, z = np.array([0, n], dtype=np.int64), np.zeros(n + 1, dtype=np.int32)
        A = self.lib.hypre_amd_ParCSRMatrixFromArrays(0, n, n, B._bp(part), B._bp(part), 0, None, B._ip(self.indptr), B._ip(self.indices),
                                                      B._rp(data), B._ip(z), None, None, B.HYPRE_MEMORY_DEVICE)
        B.check()
        self._mats[id(A)] = (par, A, data, part, z)
        return par, A

    def sizes(self, p, forward):
        key = (p, forward)
        if key not in self._sizes:
            self._sizes[key] = level_sizes(self.indptr, self.indices, p, forward)
        return self._sizes[key]

    def expected(self, relax_type, p):
        """(lanes, blocks, run launches, level launches) of the LAST device call that relax_type makes (89: its backward half)"""
        p = min(p, self.n)
        dirs = {3: (True,), 13: (True,), 4: (False,), 14: (False,), 89: (False,)}.get(relax_type, (True, False))
        runs = grids = 0
        for fwd in dirs:
            r, g = launches(self.sizes(p, fwd), self.lanes)
            runs, grids = runs + r, grids + g
        return self.lanes, p, runs, grids

    def stats(self):
        v = [C.c_int(-1) for _ in range(4)]
        self.lib.hypre_amd_GsSweepStats(*[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def check(self, relax_type, relax_points, w, omega, p=1, mat=None, l1=None):
        """one sweep on the device and in the oracle from the same state; returns the stats of the device call"""
        from hypre_amd import binding as B
        lib = self.lib
        par, A = mat if mat is not None else (self.par, self.A)
        uses_l1 = relax_type in L1_TYPES
        d_l1v = self.d_l1 if l1 is None else B.parvec_from_numpy(l1)
        h_l1 = self.l1 if l1 is None else l1
        vecs = [B.parvec_from_numpy(v) for v in (self.u0, self.f, np.zeros(self.n), np.zeros(self.n))]
        du, df, dv, dz = vecs
        try:
            lib.hypre_amd_RelaxSetNumThreads(p)
            err = lib.hypre_BoomerAMGRelax(A, df, self.d_cf if relax_points else None, relax_type, relax_points, w, omega,
                                           d_l1v.contents.local_vector.contents.data if uses_l1 else None, du, dv, dz)
            B.check()
            assert err == 0
            u = B.parvec_to_numpy(du)
            stats = self.stats()
        finally:
            lib.hypre_amd_RelaxSetNumThreads(1)
            for v in vecs + ([d_l1v] if l1 is not None else []):
                lib.hypre_ParVectorDestroy(v)
        ur = self.u0.copy()
        assert self.oracle.relax(par, self.f, self.cf if relax_points else None, relax_type, relax_points, w, omega,
                                 h_l1 if uses_l1 else None, ur, num_threads=p) == 0
        if not np.array_equal(u.view(np.int64), ur.view(np.int64)):
            i = int(np.nonzero(u.view(np.int64) != ur.view(np.int64))[0][0])
            raise AssertionError("%s relax %d points %d w %g omega %g p %d: first differing row %d (%d entries, block %s, level "
                                 "%d forward / %d backward): device %r oracle %r; %d rows differ"
                                 % (self.name, relax_type, relax_points, w, omega, p, i, self.indptr[i + 1] - self.indptr[i],
                                    [t for t in range(min(p, self.n)) if block_of(self.n, min(p, self.n), t)[0] <= i][-1],
                                    row_levels(self.indptr, self.indices, min(p, self.n), True)[i],
                                    row_levels(self.indptr, self.indices, min(p, self.n), False)[i],
                                    u[i], ur[i], int(np.sum(u != ur))))
        assert stats == self.expected(relax_type, p), (stats, self.expected(relax_type, p))
        return stats, u


@pytest.fixture(scope="module")
def cases(gpu_lib, oracle):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(name, gpu_lib, oracle)
        return built[name]

    yield get
    for c in built.values():
        for par, A, *_ in c._mats.values():
            gpu_lib.hypre_ParCSRMatrixDestroy(A)
        gpu_lib.hypre_ParVectorDestroy(c.d_l1)
        from hypre_amd import binding as B
        gpu_lib.hypre_Free(C.cast(c.d_cf, C.c_void_p), B.HYPRE_MEMORY_DEVICE)


# ---------------------------------------------------------------------------------------------------------------------
# the shapes are what the docstring says (no GPU work: the generators and the test's own schedule)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [4, 8, 16, 32])
def test_stripe_matrix_has_the_levels_and_rows_it_was_built_for(cases, G):
    c = cases("stripe%d" % G)
    small = 1024 // G
    assert c.lanes == G
    fwd, bwd = c.sizes(1, True), c.sizes(1, False)
    assert fwd == c.widths
    # row 0 has no entry but its diagonal: it reads nothing, so in the backward sweep it sits in level 0 with the last stripe
    assert bwd == [c.widths[-1] + 1] + c.widths[-2:0:-1]
    for sizes in (fwd, bwd):
        assert {small - 1, small, small + 1, 2 * small + 5, 1, 3} <= set(sizes)
        runs, grids = launches(sizes, G)
        assert grids >= 3 and runs >= 4
    # entries after the diagonal, in the levels that get a grid of their own and in those that stay in a run
    off = np.diff(c.indptr) - 1
    starts = np.concatenate(([0], np.cumsum(c.widths)))
    want = {1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1} | ({3 * G + 1} if G == 32 else set())
    in_grid = set().union(*[set(off[starts[s]:starts[s + 1]].tolist()) for s, wd in enumerate(c.widths) if wd > small])
    in_run = set().union(*[set(off[starts[s]:starts[s + 1]].tolist()) for s, wd in enumerate(c.widths) if wd <= small])
    # (one entry after the diagonal is for the last stripe alone, which is small: a row between two stripes needs two links)
    assert want - {1} <= in_grid and want <= in_run, (sorted(want - in_grid), sorted(want - in_run))
    assert off[0] == 0 and np.all(off[1:] >= 1)


def test_the_other_matrices_have_the_levels_they_were_built_for(cases):
    g3, g2, ch = cases("grid3d"), cases("grid2d"), cases("chain")
    assert (g3.n, g3.lanes, len(g3.sizes(1, True)), max(g3.sizes(1, True))) == (4096, 8, 46, 192)
    assert (g2.n, g2.lanes, float(g2.indptr[-1]) / g2.n) == (64, 4, 4.5)
    assert (ch.n, ch.lanes) == (2 * MAX_RUN + 3, 4)
    for fwd in (True, False):
        assert ch.sizes(1, fwd) == [1] * ch.n and launches(ch.sizes(1, fwd), 4) == (3, 0)
    # uneven splits for the thread-block cases
    for c, ps in ((cases("stripe8"), (3, 7)), (g3, (3, 7)), (g2, (3, 7)), (ch, (2, 5, 7))):
        assert all(c.n % p for p in ps), (c.name, c.n)


# ---------------------------------------------------------------------------------------------------------------------
# one block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax_points", [0, 1, -1])
@pytest.mark.parametrize("w,omega", WEIGHTS)
@pytest.mark.parametrize("relax_type", RELAX_TYPES)
@pytest.mark.parametrize("name", ["stripe4", "stripe8", "stripe16", "stripe32", "grid2d", "oneway"])
def test_sweep_is_the_sequential_sweep(cases, name, relax_type, w, omega, relax_points):
    c = cases(name)
    (lanes, threads, runs, grids), _ = c.check(relax_type, relax_points, w, omega)
    assert threads == 1
    if name.startswith("stripe"):
        assert lanes == int(name[6:])
    if name != "grid2d":
        assert grids > 0 and runs > 0


@pytest.mark.parametrize("w,omega", WEIGHTS)
@pytest.mark.parametrize("relax_type", RELAX_TYPES)
def test_sweep_on_the_16_cubed_grid(cases, relax_type, w, omega):
    (lanes, threads, runs, grids), _ = cases("grid3d").check(relax_type, 0, w, omega)
    assert lanes == 8 and grids > 0


@pytest.mark.parametrize("w,omega", WEIGHTS)
@pytest.mark.parametrize("relax_type", RELAX_TYPES)
def test_sweep_on_a_chain_of_three_runs(cases, relax_type, w, omega):
    """one row per level: runs of 12288, 12288 and 3 levels a direction; the second and third must start at the right level"""
    (lanes, threads, runs, grids), _ = cases("chain").check(relax_type, 0, w, omega)
    assert lanes == 4 and grids == 0 and runs == (6 if relax_type in (6, 8, 88) else 3)


# ---------------------------------------------------------------------------------------------------------------------
# emulated threads
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,omega", WEIGHTS)
@pytest.mark.parametrize("relax_type", RELAX_TYPES)
@pytest.mark.parametrize("name,p", [(m, p) for m in ("stripe8", "grid3d", "chain", "grid2d") for p in (2, 3, 7, "n")]
                         + [("chain", 5), ("grid2d", "n+5")] + [("blockedge", p) for p in EDGE_P])
def test_sweep_in_thread_blocks(cases, name, p, relax_type, w, omega):
    c = cases(name)
    threads = {"n": c.n, "n+5": c.n + 5}.get(p, p)
    (lanes, blocks, runs, grids), _ = c.check(relax_type, 0, w, omega, p=threads)
    assert blocks == min(threads, c.n)
    if p == "n" or p == "n+5":
        # every row its own block: one level of n rows a direction
        both = 2 if relax_type in (6, 8, 88) else 1
        assert (runs, grids) == ((0, both) if c.n > 1024 // lanes else (both, 0))


@pytest.mark.parametrize("relax_points", [1, -1])
@pytest.mark.parametrize("relax_type", [6, 89])
@pytest.mark.parametrize("name,p", [("stripe8", 3), ("stripe8", 7), ("grid2d", 3), ("oneway", 3)])
def test_sweep_in_thread_blocks_on_cf_points(cases, name, p, relax_type, relax_points):
    cases(name).check(relax_type, relax_points, 0.8, 1.2, p=p)


def test_the_cut_row_of_an_uneven_split_reads_across_both_of_its_edges(cases):
    """no GPU work: the block-edge matrix holds the entries it was built for, one past each end of the blocks around the cut"""
    c = cases("blockedge")
    for p in EDGE_P:
        assert c.n % p
        cut, size = edge_cut(c.n, p)
        assert block_of(c.n, p, c.n % p) == (cut, cut + size) and block_of(c.n, p, c.n % p - 1) == (cut - size - 1, cut)
        assert cut + size in c.indices[c.indptr[cut]:c.indptr[cut + 1]]
        assert c.n % p == 1 or cut - size - 2 in c.indices[c.indptr[cut - 1]:c.indptr[cut]]


def test_thread_block_cases_reach_the_level_kernel(cases):
    """the in-block / off-block split must be seen by gs_level_kernel too, not by the run kernel alone"""
    for name, ps in (("stripe8", (2, 3, 7)), ("grid3d", (2, 3, 7))):
        c = cases(name)
        for p in ps:
            for fwd in (True, False):
                assert launches(c.sizes(p, fwd), c.lanes)[1] > 0, (name, p, fwd)


# ---------------------------------------------------------------------------------------------------------------------
# rows the sweep must leave alone
# ---------------------------------------------------------------------------------------------------------------------
def _some_rows(c):
    """a handful of rows in small and in large levels"""
    starts = np.concatenate(([0], np.cumsum(c.widths)))
    return np.array(sorted({0, int(starts[3]) + 5, int(starts[5]) + 1, int(starts[5]) + 2 * (1024 // c.lanes), int(starts[8]), c.n - 1}))


@pytest.mark.parametrize("w,omega", WEIGHTS)
@pytest.mark.parametrize("G", [4, 8, 16, 32])
def test_rows_with_a_zero_diagonal_are_left_untouched(cases, G, w, omega):
    c = cases("stripe%d" % G)
    rows = _some_rows(c)
    key = "_zero_diag"
    if not hasattr(c, key):
        data = c.data.copy()
        data[c.indptr[rows]] = 0.0
        setattr(c, key, c.matrix(data))
    _, u = c.check(3, 0, w, omega, mat=getattr(c, key))
    assert np.array_equal(u[rows], c.u0[rows])
    assert np.sum(u != c.u0) == c.n - len(rows)


@pytest.mark.parametrize("w,omega", WEIGHTS)
@pytest.mark.parametrize("G", [4, 8, 16, 32])
def test_rows_with_a_zero_l1_value_are_left_untouched(cases, G, w, omega):
    c = cases("stripe%d" % G)
    rows = _some_rows(c)
    l1 = c.l1.copy()
    l1[rows] = 0.0
    _, u = c.check(13, 0, w, omega, l1=l1)
    assert np.array_equal(u[rows], c.u0[rows])
    assert np.sum(u != c.u0) == c.n - len(rows)
