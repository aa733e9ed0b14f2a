"""Row-slice form with a multivector (spmv_rs_mv_kernel): a matrix that cannot change behind its plan is multiplied from its
jagged row slices for groups of 2 - 4 columns in one pass, every column bit for bit the single-vector row-slice product of
that column (a lane's entries in stored order, then the W partial sums of a row in lane order)."""
import ctypes as C

import numpy as np
import pytest

from util import banded_csr, rand_vector

pytestmark = pytest.mark.gpu


def _bound(A, x, alpha, beta, b):
    return 1e-13 * (abs(alpha) * (abs(A) @ np.abs(x)) + abs(beta) * np.abs(b)) + 1e-300


def _multivector(B, X):
    n, nv = X.shape
    v = B.vec_from_numpy(np.ascontiguousarray(X.T).ravel())
    v.contents.size, v.contents.num_vectors, v.contents.vecstride, v.contents.idxstride = n, nv, n, 1
    return v


def _columns(B, v):
    s = v.contents
    return B.fetch(s.data, s.size * s.num_vectors, np.float64, s.memory_location).reshape(s.num_vectors, s.size).T


# the widths of test_seq_matvec_gpu.py::test_row_slice_form that take the form: W = 1, 2, 4, 8, 32, every KP, an empty row,
# a last block that is not full; the numbers of rows and columns are even (columns of x and y 16-byte aligned)
MATRICES = [(13, 48, 5000, 2), (20, 40, 9000, 2), (49, 160, 3000, 8), (60, 90, 2500, 4), (200, 900, 1500, 32), (0, 30, 4000, 1),
            (33, 64, 2000, 4), (10, 20, 300, 1)]


@pytest.fixture(scope="module")
def matrices():
    return {(lo, hi, n): banded_csr(n, n - 100, lo, hi, max(hi + 100, 500), seed=hi + n, empty_frac=0.02 if lo == 0 else 0.0)
            for lo, hi, n, _ in MATRICES}


@pytest.mark.parametrize("lo,hi,n,lanes", MATRICES)
@pytest.mark.parametrize("nv,alpha,beta", [(2, 1.0, 0.0), (3, 0.7, -1.3), (4, -1.0, 1.0), (7, 2.5, 0.5)])
def test_row_slice_multivector_has_the_bits_of_the_column_loop(gpu_lib, matrices, lo, hi, n, lanes, nv, alpha, beta):
    from hypre_amd import binding as B
    lib = gpu_lib
    A = matrices[lo, hi, n]
    m = A.shape[1]
    X = np.stack([rand_vector(m, 10 + k) for k in range(nv)], axis=1)
    Bm = np.stack([rand_vector(n, 20 + k) for k in range(nv)], axis=1)
    dA = B.csr_from_scipy(A)
    lib.hypre_amd_CSRMatrixSetImmutable(dA, 1)
    out = {}
    try:
        for on in (1, 0):
            lib.hypre_amd_SpmvSetFusedMultivectors(on)
            vx, vb, vy = _multivector(B, X), _multivector(B, Bm), _multivector(B, np.full((n, nv), 7.0))
            before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
            lib.hypre_CSRMatrixMatvecOutOfPlace(alpha, dA, vx, beta, vb, vy, 0)
            B.check()
            launches = lib.hypre_amd_SpmvFusedMultivectorLaunches() - before
            rows, per = C.c_int(), C.c_int()
            assert lib.hypre_amd_CSRMatrixPlanForm(dA) == 5 and lib.hypre_amd_CSRMatrixPlanRowSlices(dA, C.byref(rows), C.byref(per)) == lanes
            assert (launches >= 1) if on else (launches == 0), (on, launches)
            out[on] = _columns(B, vy)
            lib.hypre_CSRMatrixMatvec(alpha, dA, vx, beta, vb)          # in place: B = alpha A X + beta B
            B.check()
            out[on, "inplace"] = _columns(B, vb)
            for o in (vx, vb, vy):
                lib.hypre_SeqVectorDestroy(o)
        # the loop over the columns written out: one single-vector call per column
        single = np.zeros((n, nv))
        for k in range(nv):
            dx, db, dy = B.vec_from_numpy(X[:, k].copy()), B.vec_from_numpy(Bm[:, k].copy()), B.vec_from_numpy(np.zeros(n))
            lib.hypre_CSRMatrixMatvecOutOfPlace(alpha, dA, dx, beta, db, dy, 0)
            B.check()
            single[:, k] = B.vec_to_numpy(dy)
            for o in (dx, db, dy):
                lib.hypre_SeqVectorDestroy(o)
    finally:
        lib.hypre_amd_SpmvSetFusedMultivectors(1)
    lib.hypre_CSRMatrixDestroy(dA)
    assert out[1].tobytes() == out[0].tobytes(), float(np.max(np.abs(out[1] - out[0])))
    assert out[1].tobytes() == single.tobytes()
    assert out[1, "inplace"].tobytes() == out[0, "inplace"].tobytes()
    assert out[1].tobytes() == out[1, "inplace"].tobytes()
    ref = alpha * (A @ X) + beta * Bm
    bound = np.stack([_bound(A, X[:, k], alpha, beta, Bm[:, k]) for k in range(nv)], axis=1)
    assert np.all(np.abs(out[1] - ref) <= bound)
