"""The device Galerkin product (rap_kernels.hip: device_rap) on every path it can take, against the host loop and against
scipy.

hypre_BoomerAMGBuildCoarseOperatorKT(P, A, P) is called on synthetic operands, once by the host loop and once with
hypre_amd_SetSetupDeviceRAP(2, 0), which sends a standalone call to the device product.  The operands are shaped (and
hypre_amd_SetDeviceRapTables forces table sizes and the scratch budget) so that each case reaches one path of the
product: with or without the pilot walk, first attempt or the retry ladder, one walk or two walks, or the host fallback.
hypre_amd_GetDeviceRapPath reports which path ran.  Every case checks:
  * device == host, array for array: row pointers, column order (diagonal first), values bit for bit, and the stored
    transpose of P;
  * device == scipy's P^T A P, which owes nothing to this project: exactly for operands whose products and sums are
    exact in fp64, within the forward-error bound of the sums for random real operands;
  * the path the case is about, and the product counter (one product on the device, none for the fallback).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from util import parcsr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# |C_dev - C_ref| <= C_BOUND * k_ij * eps * (|P|^T |A| |P|)_ij.  An entry is a nested sum (RA over the rows of R, the row
# over RA) of k_ij triple products; the depth of both sums together is at most 2 k_ij + 2 roundings of unit eps / 2, so
# each of the two computations is off by at most (k_ij + 1) eps (|P|^T |A| |P|)_ij and the two together by 4 k_ij eps.
C_BOUND = 4.0
PILOT_STEP = 61           # the pilot walks the coarse rows 0, 61, 122, ...
EXACT_A = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 3.0, -3.0])
EXACT_P = np.array([1.0, -1.0, 0.5, -0.5, 2.0])


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def make_operands(nc, ratio=2.5, a_len=(3, 8), band=6, exact=True, seed=0, long_rows=(), long_len=0, long_spread=False,
                  quiet_rows=(), empty_a_frac=0.0, no_interp_frac=0.1):
    """A (nf x nf) and P (nf x nc) as scipy CSR with stored (unsorted) column order.

    P is the identity on the C-points (spread evenly over the fine points) plus 1 - 6 entries on an F-row, taken from the
    coarse columns near the row; a fraction no_interp_frac of the F-rows has none.  Coarse columns ic % 97 == 5 and the `quiet_rows` are
    touched by no F-row (their only P entry is their own C-row).  A has a_len entries per row within `band` of the row,
    diagonal first; `empty_a_frac` of its rows are empty.  The C-rows of A of the coarse points `long_rows` get long_len
    columns: a contiguous block (few coarse neighbours) or, with long_spread, spread over all fine points."""
    rng = np.random.default_rng(seed)
    nf = int(round(nc * ratio))
    cpts = np.round(np.arange(nc) * (nf - 1) / max(nc - 1, 1)).astype(np.int64) if nc > 1 else np.zeros(1, dtype=np.int64)
    is_c = np.zeros(nf, dtype=bool)
    is_c[cpts] = True
    below = np.cumsum(is_c) - is_c                  # C-points before every fine point: its position on the coarse grid
    quiet = np.zeros(nc, dtype=bool)
    quiet[np.arange(nc) % 97 == 5] = True
    quiet[list(quiet_rows)] = True
    pval = (lambda n: rng.choice(EXACT_P, n)) if exact else (lambda n: rng.uniform(-1.0, 1.0, n))
    aval = (lambda n: rng.choice(EXACT_A, n)) if exact else (lambda n: rng.uniform(-1.0, 1.0, n))

    p_ptr, p_col, p_val = [0], [], []
    coarse_of = np.full(nf, -1, dtype=np.int64)
    coarse_of[cpts] = np.arange(nc)
    for i in range(nf):
        if is_c[i]:
            p_col.append(np.array([coarse_of[i]])); p_val.append(np.ones(1))
        elif rng.random() >= no_interp_frac:
            lo, hi = max(0, below[i] - 4), min(nc, below[i] + 4)
            cand = np.arange(lo, hi)
            cand = cand[~quiet[cand]]
            k = min(int(rng.integers(1, 7)), cand.size)
            cols = rng.choice(cand, k, replace=False) if k else np.zeros(0, dtype=np.int64)
            p_col.append(cols); p_val.append(pval(cols.size))
        else:
            p_col.append(np.zeros(0, dtype=np.int64)); p_val.append(np.zeros(0))
        p_ptr.append(p_ptr[-1] + p_col[-1].size)
    P = sp.csr_matrix((np.concatenate(p_val), np.concatenate(p_col).astype(np.int32), np.array(p_ptr, dtype=np.int32)),
                      shape=(nf, nc))

    long_fine = {int(cpts[ic]) for ic in long_rows}
    a_ptr, a_col, a_val = [0], [], []
    for i in range(nf):
        if i in long_fine:
            if long_spread:
                others = rng.choice(np.delete(np.arange(nf), i), min(long_len, nf) - 1, replace=False)
            else:
                lo = min(max(0, i - long_len // 2), max(nf - long_len, 0))
                others = rng.permutation(np.setdiff1d(np.arange(lo, min(nf, lo + long_len)), [i]))[:long_len - 1]
            cols = np.concatenate([[i], others])
        elif empty_a_frac and rng.random() < empty_a_frac:
            cols = np.zeros(0, dtype=np.int64)
        else:
            lo, hi = max(0, i - band), min(nf, i + band + 1)
            k = min(int(rng.integers(a_len[0], a_len[1] + 1)), hi - lo)
            cols = np.concatenate([[i], rng.permutation(np.setdiff1d(np.arange(lo, hi), [i]))[:k - 1]])
        a_col.append(cols); a_val.append(aval(cols.size))
        a_ptr.append(a_ptr[-1] + cols.size)
    A = sp.csr_matrix((np.concatenate(a_val), np.concatenate(a_col).astype(np.int32), np.array(a_ptr, dtype=np.int32)),
                      shape=(nf, nf))
    return A, P


def row_lengths(A, P):
    """Lengths of every coarse row's RA (distinct fine columns) and of its output row (diagonal slot included): what the
    kernel's tables must hold."""
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    RA = (ones(P).T.tocsr() @ ones(A)).tocsr()
    O = (RA @ ones(P)).tocsr() + sp.identity(P.shape[1], format="csr")
    return np.diff(RA.indptr), np.diff(O.tocsr().indptr)


# ---------------------------------------------------------------------------------------------------------------------
# the library's side
# ---------------------------------------------------------------------------------------------------------------------
def galerkin(L, B, A, P, device, keepT=1, on_device=False):
    """hypre_BoomerAMGBuildCoarseOperatorKT(P, A, P) -> (arrays of the product, arrays of P's stored transpose or None,
    products the device formed, path report)"""
    loc = B.HYPRE_MEMORY_DEVICE if on_device else B.HYPRE_MEMORY_HOST
    Ap, Pp = parcsr(L, B, A, loc), parcsr(L, B, P, loc)
    L.hypre_amd_SetSetupDeviceRAP(2 if device else 1, 0)
    try:
        out = C.c_void_p()
        L.hypre_BoomerAMGBuildCoarseOperatorKT(Pp, Ap, Pp, keepT, C.byref(out))
        B.check()
    finally:
        formed = L.hypre_amd_SetSetupDeviceRAP(1, 20000)
    assert out.value, "no product came back"
    Cp = C.cast(out, C.POINTER(B.ParCSRMatrix))
    prod = B.csr_to_arrays(Cp.contents.diag)
    T = B.csr_to_arrays(Pp.contents.diagT) if keepT else None
    if not keepT:
        assert not Pp.contents.diagT
    path = [C.c_int(-1) for _ in range(4)]
    L.hypre_amd_GetDeviceRapPath(*[C.byref(v) for v in path])
    for m in (Cp, Ap, Pp):
        L.hypre_ParCSRMatrixDestroy(m)
    B.check()
    return prod, T, formed, dict(zip(("pilot", "attempts", "two_walks", "fell_back"), [v.value for v in path]))


@pytest.fixture
def rap(gpu_lib):
    """the library with every switch of the product restored afterwards"""
    from hypre_amd import binding as B
    L = gpu_lib
    L.hypre_amd_SetSetupDeviceRAP(-1, -1)
    try:
        yield L, B
    finally:
        L.hypre_amd_SetDeviceRapTables(-1, -1, -1)
        L.hypre_amd_SetSetupDeviceRAP(1, 20000)


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def assert_same_arrays(x, y, what):
    for name, a, b in zip(("row pointers", "columns", "values"), x, y):
        assert a.shape == b.shape, "%s: %s of shapes %s and %s" % (what, name, a.shape, b.shape)
        if not np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                              b.view(np.int64) if b.dtype == np.float64 else b):
            k = int(np.flatnonzero(a != b)[0]) if np.any(a != b) else -1
            raise AssertionError("%s: %s differ (first at %d)" % (what, name, k))


def _keys(M, nc):
    M = M.tocoo()
    k = M.row.astype(np.int64) * nc + M.col
    o = np.argsort(k, kind="stable")
    return k[o], M.data[o]


def _at(keys, ref_keys, ref_vals):
    """ref values at `keys` (0 where the reference has no entry)"""
    if ref_keys.size == 0:
        return np.zeros(keys.size)
    idx = np.minimum(np.searchsorted(ref_keys, keys), ref_keys.size - 1)
    return np.where(ref_keys[idx] == keys, ref_vals[idx], 0.0)


def assert_is_scipy_product(prod, A, P, exact):
    """the device's product against scipy's P^T A P: the pattern is the symbolic product's plus the diagonal slot,
    every row starts with its diagonal, and the values are scipy's (exact operands) or within the bound (real ones)"""
    nc = P.shape[1]
    ii, jj, aa = prod
    assert ii.shape == (nc + 1,) and ii[0] == 0 and np.all(np.diff(ii) >= 1)
    rows = np.repeat(np.arange(nc), np.diff(ii))
    assert np.array_equal(jj[ii[:-1]], np.arange(nc)), "a row does not start with its diagonal"
    keys = rows * nc + jj
    assert np.unique(keys).size == keys.size, "a row holds a column twice"
    order = np.argsort(keys)
    keys, vals = keys[order], aa[order]
    As, Ps = A.sorted_indices(), P.sorted_indices()
    ref = (Ps.T.tocsr() @ As @ Ps).tocsr()
    absP = abs(Ps)
    mag = (absP.T.tocsr() @ abs(As) @ absP).tocsr()
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    terms = (ones(Ps).T.tocsr() @ ones(As) @ ones(Ps)).tocsr()
    sym_keys, _ = _keys(terms + sp.identity(nc, format="csr"), nc)
    assert np.array_equal(keys, sym_keys), "the pattern is not the symbolic product's (%d and %d entries)" % (keys.size, sym_keys.size)
    ref_keys, ref_vals = _keys(ref, nc)
    ref_keys, ref_vals = ref_keys[ref_vals != 0], ref_vals[ref_vals != 0]
    assert np.isin(ref_keys, keys).all(), "a nonzero of scipy's product is missing"
    want = _at(keys, ref_keys, ref_vals)
    if exact:
        bad = np.flatnonzero(vals != want)
        assert bad.size == 0, "%d values differ from the exact product, e.g. (%d, %d): %r vs %r" % (
            bad.size, keys[bad[0]] // nc, keys[bad[0]] % nc, vals[bad[0]], want[bad[0]])
    else:
        k = _at(keys, *_keys(terms, nc))
        m = _at(keys, *_keys(mag, nc))
        err = np.abs(vals - want)
        lim = C_BOUND * k * EPS * m
        bad = np.flatnonzero(err > lim)
        assert bad.size == 0, "%d values outside the bound, worst %.3e x the bound" % (
            bad.size, float(np.max(err[bad] / np.maximum(lim[bad], 1e-300))))


def check_case(L, B, A, P, exact, keepT=1, on_device=False):
    """host and device product of the same operands, checked against each other and against scipy; the device's path"""
    host, hT, formed_h, _ = galerkin(L, B, A, P, device=False, keepT=keepT)
    assert formed_h == 0
    dev, dT, formed, path = galerkin(L, B, A, P, device=True, keepT=keepT, on_device=on_device)
    assert_same_arrays(host, dev, "device and host product")
    if keepT:
        assert_same_arrays(hT, dT, "stored transposes of P")
    assert_is_scipy_product(dev, A, P, exact)
    return formed, path


# ---------------------------------------------------------------------------------------------------------------------
# the paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_pilot_first_attempt_one_walk(rap, exact):
    """nc >= 4096 uniform rows: the pilot's sample (every 61st row) sizes the tables, its margin covers the rows it did
    not see, the first attempt fits, one walk"""
    L, B = rap
    A, P = make_operands(6000, exact=exact, seed=1)
    ra, o = row_lengths(A, P)
    s_ra, s_o = ra[::PILOT_STEP].max(), o[::PILOT_STEP].max()
    # the case is about the margin: some row the pilot did not see is longer than every row it saw
    assert ra.max() > s_ra or o.max() > s_o
    assert ra.max() <= s_ra + s_ra // 4 + 16 and o.max() <= s_o + s_o // 4 + 8
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 1
    assert path == dict(pilot=1, attempts=1, two_walks=0, fell_back=0), path


@pytest.mark.parametrize("exact", [True, False])
def test_no_pilot_first_attempt(rap, exact):
    """nc < 4096: no pilot, the fixed first guesses (384 / 192 entries) hold every row"""
    L, B = rap
    A, P = make_operands(2500, exact=exact, seed=2)
    ra, o = row_lengths(A, P)
    assert ra.max() <= 384 and o.max() <= 192
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 1
    assert path == dict(pilot=0, attempts=1, two_walks=0, fell_back=0), path


@pytest.mark.parametrize("exact", [True, False])
def test_no_pilot_overflow_retries(rap, exact):
    """nc < 4096 and a few RA rows longer than 384: the first attempt overflows, a later one with larger tables fits"""
    L, B = rap
    A, P = make_operands(2500, exact=exact, seed=3, long_rows=(7, 1200, 2301), long_len=450)
    ra, o = row_lengths(A, P)
    assert ra.max() > 384 and np.sum(ra > 384) == 3
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 1
    assert path["pilot"] == 0 and path["attempts"] >= 2 and path["two_walks"] == 0 and path["fell_back"] == 0, path


@pytest.mark.parametrize("exact", [True, False])
def test_pilot_underestimates(rap, exact):
    """nc >= 4096, the rows the pilot samples are short (no F-row touches them) and a few rows it does not see are many
    times longer: the pilot's tables overflow, the ladder climbs to a fit"""
    L, B = rap
    nc = 6000
    sampled = np.arange(0, nc, PILOT_STEP)
    A, P = make_operands(nc, exact=exact, seed=4, quiet_rows=sampled, long_rows=(30, 2000, 4321, 5999), long_len=120)
    ra, o = row_lengths(A, P)
    s_ra, s_o = ra[sampled].max(), o[sampled].max()
    assert ra.max() >= 5 * s_ra and ra.max() > s_ra + s_ra // 4 + 16 and o.max() > s_o + s_o // 4 + 8
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 1
    assert path["pilot"] == 1 and path["attempts"] >= 2 and path["two_walks"] == 0 and path["fell_back"] == 0, path


@pytest.mark.parametrize("exact", [True, False])
def test_forced_tiny_tables_climb_the_ladder(rap, exact):
    """first tables forced to 8 entries (no pilot, although nc >= 4096): at least three attempts, growing tables, the
    same product"""
    L, B = rap
    A, P = make_operands(4500, exact=exact, seed=5)
    L.hypre_amd_SetDeviceRapTables(8, 8, -1)
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 1
    assert path["pilot"] == 0 and path["attempts"] >= 3 and path["two_walks"] == 0 and path["fell_back"] == 0, path


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("overflow_first", [False, True])
def test_two_walks(rap, exact, overflow_first):
    """scratch budget 0: lengths first, then a second walk with output tables sized to the longest row; after an
    overflow too (the second walk's tables must come from the longest row, not from the first attempt)"""
    L, B = rap
    A, P = make_operands(2500, exact=exact, seed=6)
    ra, o = row_lengths(A, P)
    if overflow_first:
        assert o.max() > 8
        L.hypre_amd_SetDeviceRapTables(8, 8, 0)
    else:
        L.hypre_amd_SetDeviceRapTables(-1, -1, 0)
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 1
    assert path["pilot"] == 0 and path["two_walks"] == 1 and path["fell_back"] == 0, path
    assert path["attempts"] >= 3 if overflow_first else path["attempts"] == 1, path


@pytest.mark.parametrize("exact", [True, False])
def test_row_over_the_lds_budget_goes_to_the_host(rap, exact):
    """one coarse row whose RA has more than 4096 distinct fine columns: its tables pass the 150 KB LDS budget, the
    product is left to the host loop, and what comes back is the host's"""
    L, B = rap
    A, P = make_operands(2400, exact=exact, seed=7, long_rows=(1000,), long_len=4500, long_spread=True)
    ra, o = row_lengths(A, P)
    assert ra.max() > 4096
    formed, path = check_case(L, B, A, P, exact)
    assert formed == 0
    assert path["fell_back"] == 1, path


@pytest.mark.parametrize("shape", ["one_entry", "empty_A_rows", "lonely_coarse_points", "F_rows_without_P"])
def test_degenerate_shapes(rap, shape):
    """a 1 x 1 A; A with empty rows (C-rows and F-rows); coarse points whose only P entry is their own C-row; F-rows that
    interpolate from nothing"""
    L, B = rap
    if shape == "one_entry":
        A = sp.csr_matrix(([2.0], [0], [0, 1]), shape=(1, 1))
        P = sp.csr_matrix(([1.0], [0], [0, 1]), shape=(1, 1))
    elif shape == "empty_A_rows":
        A, P = make_operands(600, exact=True, seed=8, empty_a_frac=0.3)
        assert np.sum(np.diff(A.indptr) == 0) > 100
    elif shape == "lonely_coarse_points":
        A, P = make_operands(600, exact=True, seed=9, quiet_rows=np.arange(0, 600, 3))
    else:
        A, P = make_operands(300, ratio=4.0, exact=True, seed=10, no_interp_frac=0.6)
        assert np.sum(np.diff(P.indptr) == 0) > 300
    formed, path = check_case(L, B, A, P, exact=True)
    assert formed == 1
    assert path["attempts"] == 1 and path["fell_back"] == 0, path


@pytest.mark.parametrize("keepT", [0, 1])
def test_operands_already_on_the_device(rap, keepT):
    """A and P migrated to device memory first: the device product takes them as they are (no twin), same result"""
    L, B = rap
    A, P = make_operands(2500, exact=False, seed=11)
    formed, path = check_case(L, B, A, P, exact=False, keepT=keepT, on_device=True)
    assert formed == 1
    assert path == dict(pilot=0, attempts=1, two_walks=0, fell_back=0), path
