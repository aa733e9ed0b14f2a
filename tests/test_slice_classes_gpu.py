"""Class storage of the slice form (spmv_sl_kernel_cls): a lane streams one class byte instead of its packed words and
rebuilds the very words from the block's table, so every product the slice kernel serves has the SAME BITS with
hypre_amd_SpmvSetSliceClasses on and off — products, residuals, sweeps, multivector products, whole cycles and solves.
Matrices whose blocks do not repeat (or whose class tables are not to be had) keep the packed stream."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from util import rand_vector

pytestmark = pytest.mark.gpu

CLASS_CAP = 255          # a class is named by a byte
XS_DESC = 96             # ints of a block's piece descriptors (2 * SPMV_XS_SEGS)

# Grids whose lines do not divide a block and whose rows do not fill the last one, and one with lines of exactly 256.  The
# 27-point operator gets the slice form only where its rows, padded to 32 entries, hold at most 1.3 x its entries (a rule of
# the form itself, older than the classes): thin or tiny grids have too many boundary rows, so its grids are thicker.
GRIDS_7 = [(13, 7, 5), (33, 33, 33), (64, 64, 3), (100, 40, 9), (256, 5, 4)]
GRIDS_27 = [(33, 33, 33), (45, 37, 29), (50, 30, 27), (256, 20, 18)]
CASES = ([(n, "laplacian") for n in GRIDS_7] + [(n, "27pt") for n in GRIDS_27] + [(n, "difconv") for n in GRIDS_7])
SWEEP_CASES = [((33, 33, 33), "laplacian"), ((100, 40, 9), "laplacian"), ((33, 33, 33), "27pt"), ((45, 37, 29), "27pt"),
               ((33, 33, 33), "difconv"), ((100, 40, 9), "difconv")]


@pytest.fixture
def classes(gpu_lib):
    yield gpu_lib
    gpu_lib.hypre_amd_SpmvSetSliceClasses(1)
    gpu_lib.hypre_amd_PlanTestFailAlloc(0, 0)
    gpu_lib.hypre_amd_SetMixedPrecisionValues(0)
    gpu_lib.HYPRE_ClearAllErrors()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _operator(n, problem):
    """the stencil of the ij driver on grid n as a scipy matrix"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(n=n, problem=problem)
    if problem == "difconv":
        opt.c = (1.0, 0.1, 0.01)                       # anisotropic diffusion
    P = ij.build_matrix(opt)
    A = B.csr_to_scipy(P.contents.diag).tocsr()
    B.load_library().hypre_ParCSRMatrixDestroy(P)
    return A


def _multivector(B, X):
    """column-major device multivector; the columns lie an EVEN number of doubles apart (n + 1 where n is odd), because the
    fused kernel stages x in 16-byte pieces and takes only columns that are so aligned: grids with an odd row count — the
    most ragged last blocks — then reach it too"""
    n, nv = X.shape
    stride = n + (n & 1)
    flat = np.zeros(nv * stride)
    for k in range(nv):
        flat[k * stride:k * stride + n] = X[:, k]
    v = B.vec_from_numpy(flat)
    v.contents.size, v.contents.num_vectors, v.contents.vecstride, v.contents.idxstride = n, nv, stride, 1
    return v


def _columns(B, v):
    s = v.contents
    flat = B.fetch(s.data, s.vecstride * s.num_vectors, np.float64, s.memory_location)
    return flat.reshape(s.num_vectors, s.vecstride)[:, :s.size].T


def _products(lib, A, mixed, expect_classes):
    """y = alpha A x + beta b for three (alpha, beta), in and out of place, and the multivector entry for NV = 2, 3, 4"""
    from hypre_amd import binding as B
    n = A.shape[0]
    x, b = rand_vector(n, 1), rand_vector(n, 2)
    lib.hypre_amd_SetMixedPrecisionValues(1 if mixed else 0)
    dA = B.csr_from_scipy(A)
    dx, db, dy = B.vec_from_numpy(x), B.vec_from_numpy(b), B.vec_from_numpy(np.zeros(n))
    res = []
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.7, -0.3)):
        lib.hypre_CSRMatrixMatvecOutOfPlace(alpha, dA, dx, beta, db, dy, 0)
        B.check()
        res.append(B.vec_to_numpy(dy))
    lib.hypre_CSRMatrixMatvec(-1.0, dA, dx, 1.0, db)                     # the residual, in place
    B.check()
    res.append(B.vec_to_numpy(db))
    assert lib.hypre_amd_CSRMatrixPlanForm(dA) == 4
    ncls = lib.hypre_amd_CSRMatrixPlanSliceClasses(dA)
    if expect_classes:
        assert 0 < ncls <= CLASS_CAP, ncls
    else:
        assert ncls == 0
    if not mixed:                                     # (the fused multivector kernel does not serve mixed precision)
        for nv in (2, 3, 4):
            X = np.stack([rand_vector(n, 10 + k) for k in range(nv)], axis=1)
            Bm = np.stack([rand_vector(n, 20 + k) for k in range(nv)], axis=1)
            vx, vb, vy = _multivector(B, X), _multivector(B, Bm), _multivector(B, np.full((n, nv), 7.0))
            before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
            lib.hypre_CSRMatrixMatvecOutOfPlace(0.7, dA, vx, -1.3, vb, vy, 0)
            B.check()
            assert lib.hypre_amd_SpmvFusedMultivectorLaunches() > before
            res.append(_columns(B, vy))
            for o in (vx, vb, vy):
                lib.hypre_SeqVectorDestroy(o)
    for o in (dx, db, dy):
        lib.hypre_SeqVectorDestroy(o)
    lib.hypre_CSRMatrixDestroy(dA)
    lib.hypre_amd_SetMixedPrecisionValues(0)
    return res


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n,problem", CASES)
def test_products_have_the_bits_of_the_packed_stream(classes, n, problem, mixed):
    """y = alpha A x + beta b, the residual and the multivector products (NV = 2, 3, 4), classes on against off: the same
    bits; the query reports classes within the cap and the slice form's lanes per row are what they were."""
    lib = classes
    A = _operator(n, problem)
    out = {}
    for on in (1, 0):
        lib.hypre_amd_SpmvSetSliceClasses(on)
        out[on] = _products(lib, A, mixed, expect_classes=bool(on))
    assert len(out[1]) == len(out[0]) >= 4
    for y1, y0 in zip(out[1], out[0]):
        assert np.array_equal(_bits(y1), _bits(y0))
    ref = A @ rand_vector(A.shape[0], 1)
    assert np.all(np.abs(out[1][0] - ref) <= (1e-6 if mixed else 1e-13) * (abs(A) @ np.abs(rand_vector(A.shape[0], 1))) + 1e-300)


def _setup(lib, aniso=True, **kw):
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(**kw)
    if opt.problem == "difconv" and aniso:
        opt.c = (1.0, 0.1, 0.01)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    return opt, A, s


SWEEPS = [(18, 0, False), (18, 1, False), (18, -1, False), (7, 0, False), (0, 0, False), (11, 0, False), (12, 0, False),
          (11, 0, True), (12, 0, True)]


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n,problem", SWEEP_CASES)
def test_sweeps_have_the_bits_of_the_packed_stream(classes, n, problem, mixed):
    """One sweep of every smoother the slice kernel serves on the fine level (Jacobi, CF-masked Jacobi, l1-Jacobi, the
    residual and the inner steps of the two-stage Gauss-Seidel sweeps, from a zero and a nonzero guess), classes on
    against off: the same bits."""
    from hypre_amd import binding as B
    lib = classes
    out = {}
    for on in (1, 0):
        lib.hypre_amd_SpmvSetSliceClasses(on)
        opt, A0, s = _setup(lib, n=n, problem=problem, relax_type=18, coarsen_type=8, relax_order=1)
        if mixed:
            lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
            lib.hypre_amd_SetMixedPrecisionValues(1)
        Ap = C.cast(lib.hypre_amd_BoomerAMGGetA(s, 0), C.POINTER(B.ParCSRMatrix))
        cfp = lib.hypre_amd_BoomerAMGGetCFMarker(s, 0)
        l1p = lib.hypre_amd_BoomerAMGGetL1Norms(s, 0)
        cf = C.cast(cfp, C.POINTER(B.IntArray)).contents.data if cfp else None
        l1 = C.cast(l1p, C.POINTER(B.Vector)).contents.data if l1p else None
        nrows = int(np.prod(n))
        f = rand_vector(nrows, 3)
        res = []
        for relax_type, points, zero in SWEEPS:
            u0 = np.zeros(nrows) if zero else rand_vector(nrows, 4)
            du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
            dv, dz = B.parvec_from_numpy(np.zeros(nrows)), B.parvec_from_numpy(np.zeros(nrows))
            if zero:
                lib.hypre_ParVectorSetZeros(du)
            uses_l1 = relax_type in (7, 18, 11, 12)
            err = lib.hypre_BoomerAMGRelax(Ap, df, cf, relax_type, points, 0.9, 1.0, l1 if uses_l1 else None, du, dv, dz)
            B.check()
            assert err == 0
            res.append(B.parvec_to_numpy(du))
        assert lib.hypre_amd_CSRMatrixPlanForm(Ap.contents.diag) == 4
        ncls = lib.hypre_amd_CSRMatrixPlanSliceClasses(Ap.contents.diag)
        assert (0 < ncls <= CLASS_CAP) if on else ncls == 0
        out[on] = res
        lib.hypre_amd_SetMixedPrecisionValues(0)
        lib.HYPRE_BoomerAMGDestroy(s)
    for (sweep, u1, u0) in zip(SWEEPS, out[1], out[0]):
        assert np.array_equal(_bits(u1), _bits(u0)), sweep


def _nonrepeating(n=6000, seed=5):
    """coded (two distinct values), seven random columns per row inside a band: no two lane-rows of a block alike"""
    rng = np.random.default_rng(seed)
    indptr = 7 * np.arange(n + 1, dtype=np.int32)
    indices = np.empty(7 * n, dtype=np.int32)
    for r in range(n):
        lo = min(max(r - 150, 0), n - 300)
        indices[7 * r:7 * r + 7] = np.sort(rng.choice(np.arange(lo, lo + 300), 7, replace=False))
    data = np.array([6.0, -1.0])[rng.integers(0, 2, 7 * n)]
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


@pytest.mark.parametrize("how", ["no repetition", "allocation failure"])
def test_matrices_without_classes_keep_the_packed_stream(classes, how):
    """A coded short-row matrix that does not repeat — and a stencil whose class tables are not to be had (each allocation
    of the new site failed in turn) — keeps the packed stream: the query says 0, the form is still 4, the bits are those of
    the switch turned off."""
    lib = classes
    A = _nonrepeating() if how == "no repetition" else _operator((33, 33, 33), "laplacian")
    lib.hypre_amd_SpmvSetSliceClasses(0)
    off = _products(lib, A, False, expect_classes=False)
    lib.hypre_amd_SpmvSetSliceClasses(1)
    if how == "no repetition":
        on = _products(lib, A, False, expect_classes=False)
        for y1, y0 in zip(on, off):
            assert np.array_equal(_bits(y1), _bits(y0))
        return
    for nth in range(1, 5):                   # class bytes, counts, offsets, tables
        lib.hypre_amd_PlanTestFailAlloc(6, nth)
        on = _products(lib, A, False, expect_classes=False)
        assert lib.hypre_amd_PlanTestFailAlloc(0, 0) == 0          # the failure happened
        for y1, y0 in zip(on, off):
            assert np.array_equal(_bits(y1), _bits(y0))
    on = _products(lib, A, False, expect_classes=True)             # and nothing is left armed
    for y1, y0 in zip(on, off):
        assert np.array_equal(_bits(y1), _bits(y0))


def test_the_class_kernel_notices_an_edited_coefficient(classes):
    """The staleness watch is what it was (it reads the caller's arrays, not the stream): one coefficient changed in place
    behind a plan with classes is found within the slice kernel's 128 products, the error raised, the plan rebuilt and the
    product repeated with the new matrix."""
    from hypre_amd import binding as B
    from util import laplace_3d
    lib = classes
    A = laplace_3d(24, 22, 20).tocsr()
    A.sort_indices()
    n = A.shape[0]
    x = rand_vector(n, 9)
    k, new = 2048 * 7 + 1001, 0.375
    A2 = A.copy()
    A2.data[k] = new
    dA = B.csr_from_scipy(A)
    dx, dy = B.vec_from_numpy(x), B.vec_from_numpy(np.zeros(n))
    lib.hypre_CSRMatrixMatvec(1.0, dA, dx, 0.0, dy)
    B.check()
    assert lib.hypre_amd_CSRMatrixPlanForm(dA) == 4 and lib.hypre_amd_CSRMatrixPlanSliceClasses(dA) > 0
    base = C.cast(dA.contents.data, C.c_void_p).value
    src = np.array([new], dtype=np.float64)
    lib.hypre_Memcpy(C.c_void_p(base + 8 * k), src.ctypes.data_as(C.c_void_p), 8, B.HYPRE_MEMORY_DEVICE, B.HYPRE_MEMORY_HOST)
    found = None
    for launch in range(1, 129):
        lib.hypre_CSRMatrixMatvec(1.0, dA, dx, 0.0, dy)
        if lib.HYPRE_GetError():
            found = launch
            break
    assert found is not None, "an edited coefficient went unnoticed for 128 products"
    lib.HYPRE_ClearAllErrors()
    assert np.all(np.abs(B.vec_to_numpy(dy) - A2 @ x) <= 1e-13 * (abs(A2) @ np.abs(x)))
    lib.hypre_CSRMatrixMatvec(1.0, dA, dx, 0.0, dy)
    B.check()
    for o in (dx, dy):
        lib.hypre_SeqVectorDestroy(o)
    lib.hypre_CSRMatrixDestroy(dA)


@pytest.mark.parametrize("problem,n,relax", [("laplacian", (64, 64, 64), 18), ("27pt", (48, 48, 48), 11), ("difconv", (56, 56, 56), 18)])
def test_cycle_and_pcg_have_the_bits_of_the_packed_stream(classes, problem, n, relax):
    """One V(1,1) cycle and a PCG solve preconditioned by it, classes on against off: every iterate bit for bit, the same
    iteration count."""
    from hypre_amd import binding as B
    lib = classes
    nrows = int(np.prod(n))
    out = {}
    for on in (1, 0):
        lib.hypre_amd_SpmvSetSliceClasses(on)
        opt, A, s = _setup(lib, aniso=False, n=n, problem=problem, relax_type=relax, coarsen_type=8)      # (difconv as the benchmark solves it)
        du, df = B.parvec_from_numpy(np.zeros(nrows)), B.parvec_from_numpy(np.ones(nrows))
        lib.hypre_ParVectorSetZeros(du)
        lib.HYPRE_BoomerAMGSetTol(s, 0.0)
        lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
        lib.HYPRE_BoomerAMGSolve(s, A, df, du)
        B.check()
        cycle = B.parvec_to_numpy(du)
        Ap = C.cast(lib.hypre_amd_BoomerAMGGetA(s, 0), C.POINTER(B.ParCSRMatrix))
        ncls = lib.hypre_amd_CSRMatrixPlanSliceClasses(Ap.contents.diag)
        assert (0 < ncls <= CLASS_CAP) if on else ncls == 0
        pcg, its, rel = C.c_void_p(), C.c_int(), C.c_double()
        dx = B.parvec_from_numpy(np.zeros(nrows))
        lib.HYPRE_ParCSRPCGCreate(0, C.byref(pcg))
        lib.HYPRE_PCGSetTol(pcg, 1e-8)
        lib.HYPRE_PCGSetMaxIter(pcg, 200)
        lib.HYPRE_PCGSetTwoNorm(pcg, 1)
        lib.HYPRE_PCGSetPrecond(pcg, C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s)
        lib.HYPRE_ParCSRPCGSetup(pcg, A, df, dx)
        lib.HYPRE_ParCSRPCGSolve(pcg, A, df, dx)
        B.check()
        lib.HYPRE_PCGGetNumIterations(pcg, C.byref(its))
        lib.HYPRE_PCGGetFinalRelativeResidualNorm(pcg, C.byref(rel))
        lib.HYPRE_ParCSRPCGDestroy(pcg)
        out[on] = (cycle, B.parvec_to_numpy(dx), its.value, rel.value)
        lib.HYPRE_BoomerAMGDestroy(s)
    assert np.array_equal(_bits(out[1][0]), _bits(out[0][0]))
    assert np.array_equal(_bits(out[1][1]), _bits(out[0][1]))
    assert out[1][2] == out[0][2] and 0 < out[1][2] < 200
    assert out[1][3] == out[0][3]


def test_streamed_bytes_of_a_launch_are_the_layout(classes):
    """hypre_amd_ByteCounters, streamed count of one fine-level product.  On a 7-point grid with lines of 256 every block is
    one line: a left end, an interior and a right end — three classes of 8 words.  With classes the launch reads per block
    256 class bytes, its table, the descriptors (96 + 4 words), two table offsets and one row pointer, the value table and
    the 72 words of the rotating check; the packed stream reads 24 bytes per lane and a row pointer per row instead."""
    from hypre_amd import binding as B
    lib = classes
    n = (256, 6, 5)
    A = _operator(n, "laplacian")
    nr, blocks = A.shape[0], 6 * 5
    x = rand_vector(nr, 1)
    counts = {}
    for on in (1, 0):
        lib.hypre_amd_SpmvSetSliceClasses(on)
        dA = B.csr_from_scipy(A)
        dx, dy = B.vec_from_numpy(x), B.vec_from_numpy(np.zeros(nr))
        lib.hypre_CSRMatrixMatvec(1.0, dA, dx, 0.0, dy)                    # builds the plan
        B.check()
        ncls, ndict = lib.hypre_amd_CSRMatrixPlanSliceClasses(dA), lib.hypre_amd_CSRMatrixPlanValueCodes(dA)
        csr, streamed = C.c_double(), C.c_double()
        lib.hypre_amd_ByteCounters(None, None, 1)
        lib.hypre_CSRMatrixMatvec(1.0, dA, dx, 0.0, dy)
        lib.hypre_amd_ByteCounters(C.byref(csr), C.byref(streamed), 1)
        B.check()
        counts[on] = (csr.value, streamed.value, ncls, ndict)
        for o in (dx, dy):
            lib.hypre_SeqVectorDestroy(o)
        lib.hypre_CSRMatrixDestroy(dA)
    assert counts[1][2] == 3 and counts[0][2] == 0
    ndict = counts[1][3]
    vectors = 8.0 * nr + 8.0 * nr                                          # y written, x read
    per_block = 4.0 * (XS_DESC + 4) + 8.0 * ndict + 4.0 * 72
    assert counts[1][1] == blocks * (per_block + 256 + 4.0 * 3 + 4.0 * 3 * 8) + vectors
    assert counts[0][1] == blocks * (per_block + 256 * 24.0) + 4.0 * (nr + 1) + vectors
    assert counts[1][1] < counts[0][1]
    assert counts[1][0] == counts[0][0]                                    # the CSR count does not depend on the form
