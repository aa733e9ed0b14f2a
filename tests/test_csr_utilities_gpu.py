"""The three setup-time CSR utilities of kernels.hip at their size boundaries: the exclusive scan (launch_scan_exclusive,
driven through the transpose, whose row pointer IS the scan of the column counts over num_cols elements), the device
transpose (hypre_CSRMatrixTranspose of a device matrix) and the in-place row sort (hypre_amd_CSRMatrixSortRows).

Reference: plain numpy — a stable argsort by column for the transpose (util.transpose_reference), a lexsort for the row
sort — never the oracle or the library's host routines.  Every comparison is exact: integer arrays with np.array_equal,
values byte for byte; every entry carries its own value (its position + 0.25), so a value that travels with the wrong
index shows.  Matrices are built with binding.csr_from_arrays: the stored order is what the test wrote.

Outside the contract and not tested: duplicate columns within one row (order_rows_kernel ranks the entries of a row of
A^T by source row and needs them distinct).  Not covered: the second grid-stride trip of count_columns_kernel, which needs
more than 16.7 million entries (65536 workgroups of 256)."""
import ctypes as C
import time

import numpy as np
import pytest

from util import transpose_reference

pytestmark = pytest.mark.gpu

SORT_CAP = 2048          # sort_rows_kernel: the widest bitonic network; longer rows are left as stored


def _csr(rows):
    """(indptr, indices, data) of a list of per-row column arrays, stored as given; entry k holds k + 0.25"""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = (np.concatenate(rows) if len(rows) and lens.sum() else np.zeros(0)).astype(np.int32)
    for r in rows:
        assert len(np.unique(r)) == len(r)          # distinct columns within a row: the contract
    return indptr, indices, np.arange(len(indices)) + 0.25


def _check_transpose(lib, nr, nc, indptr, indices, data, modes=(1, 0)):
    """device transpose with values (1) and pattern only (0) against the numpy reference; returns the reference ti"""
    from hypre_amd import binding as B
    assert len(indptr) == nr + 1 and indptr[nr] == len(indices)
    assert len(indices) == 0 or (0 <= indices.min() and indices.max() < nc)        # nothing the kernels would write astray
    ri, rj, ra = transpose_reference(indptr, indices, data, nr, nc)
    dA = B.csr_from_arrays(nr, nc, indptr, indices, data)
    for with_data in modes:
        dT = C.POINTER(B.CSRMatrix)()
        lib.hypre_CSRMatrixTranspose(dA, C.byref(dT), with_data)
        B.check()
        t = dT.contents
        assert (t.num_rows, t.num_cols, t.num_nonzeros, t.memory_location) == (nc, nr, len(indices), B.HYPRE_MEMORY_DEVICE)
        ti, tj, ta = B.csr_to_arrays(dT)
        assert len(ti) == nc + 1 and ti[nc] == len(indices)
        assert np.array_equal(ti, ri), "row pointer (the scan) differs first at %d" % np.flatnonzero(ti != ri)[0]
        assert np.array_equal(tj, rj), "source rows differ first at entry %d" % np.flatnonzero(tj != rj)[0]
        if with_data:
            assert len(indices) == 0 or bool(t.data)
            assert ta.tobytes() == ra.tobytes()
        else:
            assert not bool(t.data)
        lib.hypre_CSRMatrixDestroy(dT)
    lib.hypre_CSRMatrixDestroy(dA)
    return ri


# ---------------------------------------------------------------------------
# 1. the scan's regimes and boundaries
# ---------------------------------------------------------------------------
def _scan_matrix(nc, nr=2000):
    """about min(1.5 nc, 200000) entries in nr rows at random distinct columns; column 0 and nc - 1 present, one column in
    every third row, and runs of 3000 empty columns around 4096, 16384 and 819200 wherever nc reaches past them"""
    rng = np.random.default_rng(nc)
    free = np.ones(nc, dtype=bool)
    gaps = [(m - 1500, m + 1500) for m in (4096, 16384, 4096 * 200) if m + 1500 < nc - 1]
    for lo, hi in gaps:
        free[lo:hi] = False
    allowed = np.flatnonzero(free)
    hot = allowed[len(allowed) // 3]
    mean = min(1.5 * nc, 200000) / nr
    rows = []
    for r in range(nr):
        k = min(int(rng.integers(0, int(2 * mean) + 2)), len(allowed))
        forced = ([hot] if r % 3 == 0 else []) + ([0, nc - 1] if r in (5, nr - 1) else [])
        cols = np.union1d(allowed[rng.integers(0, len(allowed), k)], np.array(forced, dtype=np.int64))
        rows.append(rng.permutation(cols))
    return rows, gaps


@pytest.mark.parametrize("nc", [1, 2, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 20479, 20480, 20481, 65537, 1000003])
def test_scan_regimes_through_the_transpose(gpu_lib, nc):
    """launch_scan_exclusive over nc column counts: one workgroup walking 4096-element steps with a carry up to 16384
    (one step, exactly one, one and an element, two, exactly four), block sums + their scan + per-block scans above
    (16385 = four blocks and one element; 20480 = exactly five blocks; 65537 and 1000003: the block sums themselves still
    scanned by one workgroup).  Counts are 0, 1 and a few hundred, with runs of zeros across block boundaries."""
    rows, gaps = _scan_matrix(nc)
    indptr, indices, data = _csr(rows)
    ri = _check_transpose(gpu_lib, len(rows), nc, indptr, indices, data)
    cnt = np.diff(ri)
    assert cnt[0] > 0 and cnt[nc - 1] > 0 and cnt.max() > 600
    for lo, hi in gaps:
        assert not cnt[lo:hi].any()


def test_scan_of_more_than_16384_blocks(gpu_lib):
    """nc = 4096 * 16384 + 1: 16385 block sums, so the scan of the block sums takes the two-level path itself (second
    static buffer).  Entries sit in column 0, the last column and on both sides of the first and the last block boundaries.
    This case found order_rows_kernel launched with a wave per row of A^T: 64 nc threads are more than the 2^32 a launch
    may hold, the runtime refused the launch unnoticed, and A^T came back in the scatter's arbitrary order.  The waves
    now stride over the rows and launch_transpose reports a refused launch.
    About 270 MB per device array of nc ints.  Measured on an MI355X: 0.33 s for the whole test, 0.23 s of it the numpy
    reference, the device transpose, the copy back and the comparison (the line printed below), the rest building the input."""
    nc, nr = 4096 * 16384 + 1, 2000
    rng = np.random.default_rng(7)
    forced = np.array([0, nc - 1] + [4096 * k + d for k in (1, 16383, 16384) for d in (-1, 0, 1)], dtype=np.int64)
    forced = np.unique(forced[forced < nc])          # 4096 * 16384 is the last column; there is none behind it
    rows = []
    for r in range(nr):
        cols = np.unique(rng.integers(0, nc, 100))
        if r in (1, 700, 1300, nr - 1):
            cols = np.union1d(cols, forced)
        rows.append(rng.permutation(cols))
    indptr, indices, data = _csr(rows)
    t0 = time.perf_counter()
    ri = _check_transpose(gpu_lib, nr, nc, indptr, indices, data, modes=(1,))
    print("third scan regime: %d entries, reference + device transpose + comparison %.2f s" % (len(indices), time.perf_counter() - t0))
    assert np.all(np.diff(ri)[forced] >= 4)


# ---------------------------------------------------------------------------
# 2. long rows of A^T, the 8-lanes-per-row scatter, degenerate shapes
# ---------------------------------------------------------------------------
def test_rows_of_the_transpose_around_one_and_two_trips_of_a_wave(gpu_lib):
    """order_rows_kernel: one wave per row of A^T, lanes striding by 64.  Column c of A sits in rows 0 .. L_c - 1, so the
    rows of A^T hold exactly 1, 63, 64, 65, 127, 128, 129 and 130 entries."""
    L = (1, 63, 64, 65, 127, 128, 129, 130)
    rng = np.random.default_rng(130)
    rows = [rng.permutation([c for c in range(8) if r < L[c]]) for r in range(130)]
    indptr, indices, data = _csr(rows)
    ri = _check_transpose(gpu_lib, 130, 8, indptr, indices, data)
    assert tuple(np.diff(ri)) == L


def test_dense_columns(gpu_lib):
    """6000 full rows of 7 shuffled columns: every row of A^T has 6000 entries, 94 trips of its wave"""
    rng = np.random.default_rng(6000)
    indptr, indices, data = _csr([rng.permutation(7) for _ in range(6000)])
    _check_transpose(gpu_lib, 6000, 7, indptr, indices, data)


def test_scatter_row_lengths(gpu_lib):
    """scatter_transpose_kernel gives a row 8 lanes: rows of 0, 1, 7, 8, 9, 16, 17 and 3000 entries (no trip, part of one,
    exactly one and two, one over, 375 trips), 40 times over, between two blocks of empty rows"""
    rng = np.random.default_rng(17)
    lens = [0] * 25 + [0, 1, 7, 8, 9, 16, 17, 3000] * 40 + [0] * 25
    indptr, indices, data = _csr([rng.permutation(5000)[:l] for l in lens])
    _check_transpose(gpu_lib, len(lens), 5000, indptr, indices, data)


@pytest.mark.parametrize("nr,nc,rows", [(50, 70, [[]] * 50), (0, 33, []), (1, 1, [[0]])], ids=["no-entries", "no-rows", "one-entry"])
def test_degenerate_shapes(gpu_lib, nr, nc, rows):
    indptr, indices, data = _csr([np.array(r, dtype=np.int64) for r in rows])
    ri = _check_transpose(gpu_lib, nr, nc, indptr, indices, data)
    assert len(ri) == nc + 1 and (len(indices) > 0 or not ri.any())


# ---------------------------------------------------------------------------
# 3. the row sort, every row
# ---------------------------------------------------------------------------
SPECIAL_LENGTHS = (2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 130, 257, 1024, 1025, 2047, 2048, 2049, 2050, 3000)
SPECIAL_ROWS = (3, 40, 41, 97, 1007, 2007, 3007, 4007, 5007, 6007, 7007, 8007, 9007, 16383, 16384, 18007, 20001, 22222, 23998, 23999)


def _sort_matrix():
    """24000 x 5000 (more rows than the 64 x CUs workgroups of launch_sort_rows): rows of 0-12 entries in random order, and
    among them rows of the SPECIAL_LENGTHS, a descending and an ascending row of 1500, and a row that ascends behind a
    first entry which is its largest column"""
    nr, nc = 24000, 5000
    rng = np.random.default_rng(24000)
    rows = [rng.permutation(nc)[:l] for l in rng.integers(0, 13, nr)]
    for r, l in zip(SPECIAL_ROWS, SPECIAL_LENGTHS):
        rows[r] = rng.permutation(nc)[:l]
    asc = np.sort(rng.permutation(nc)[:1500])
    rows[50] = asc[::-1].copy()
    rows[21000] = asc.copy()
    rows[12345] = np.concatenate([asc[-1:], asc[:-1]])
    return nr, nc, rows


def _sort_reference(indptr, indices, data, keep_first):
    """each row's entries by ascending column, values alongside; the first entry excluded with keep_first; rows whose
    sorted part is longer than SORT_CAP as stored"""
    lens = np.diff(indptr).astype(np.int64)
    rows = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(len(indices))
    first = (pos == indptr[:-1].astype(np.int64)[rows]) & bool(keep_first)
    as_stored = (lens - (1 if keep_first else 0) > SORT_CAP)[rows]
    order = np.lexsort((np.where(as_stored, pos, indices), np.where(first, 0, 1), rows))
    return indices[order], data[order]


def test_sort_rows_every_row(gpu_lib):
    """sort_rows_kernel: bitonic networks of 2 to 2048 keys (t striding over the 64 lanes from 256 keys on), rows on both
    sides of the cap (2049 entries: sorted behind a kept first entry, as stored without; 2050 and 3000: as stored), the
    already-ascending exit (with and without the kept entry), workgroups that take a second row — all 24000 rows compared,
    with keep_first 1 and 0, and a second call on the sorted matrix changing nothing."""
    from hypre_amd import binding as B
    lib = gpu_lib
    nr, nc, rows = _sort_matrix()
    indptr, indices, data = _csr(rows)
    for keep_first in (1, 0):
        rj, ra = _sort_reference(indptr, indices, data, keep_first)
        # the reference did something and left something: row 23998 (2050) as stored, row 50 (descending) reversed
        b, e = indptr[23998], indptr[23999]
        assert np.array_equal(rj[b:e], indices[b:e]) and not np.array_equal(rj, indices)
        b, e = indptr[50] + keep_first, indptr[51]
        assert np.array_equal(rj[b:e], indices[b:e][::-1])
        dA = B.csr_from_arrays(nr, nc, indptr, indices, data)
        for call in (1, 2):
            lib.hypre_amd_CSRMatrixSortRows(dA, keep_first)
            B.check()
            ii, jj, aa = B.csr_to_arrays(dA)
            assert np.array_equal(ii, indptr)
            bad = np.flatnonzero((jj != rj) | (aa.view(np.int64) != ra.view(np.int64)))
            assert len(bad) == 0, "keep_first %d, call %d: %d entries differ, the first in row %d" % (
                keep_first, call, len(bad), np.searchsorted(indptr, bad[0], side="right") - 1)
        lib.hypre_CSRMatrixDestroy(dA)
