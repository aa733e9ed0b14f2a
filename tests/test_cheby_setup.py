"""Setup of the Chebyshev smoother (relax 16, par_cheby.cpp) against references that share nothing with it: the two
spectrum estimates, the tridiagonal eigenvalue routine behind the second one, the polynomial coefficients, the scaling
vector, and which of these numbers a hierarchy hands to which level.  Host only.

References
* Gershgorin estimate: the discs of every row in exact rational arithmetic (fractions.Fraction), then the sign rule.
* CG / Lanczos estimate: textbook conjugate gradients from a zero guess in numpy.longdouble, the Lanczos matrix
  of its step lengths, numpy.linalg.eigvalsh.  The start vector and the stopping rule are part of what the routine is
  (Park-Miller values; stop once r.r < 2^-52) and are restated here, everything else is the textbook's.
* coefficients: the Chebyshev polynomial the smoother is defined by, expanded in exact rational arithmetic from the double
  inputs:  with upper = 1.1 * (the dominant estimate), lower = fraction * (upper - other) + other,
  theta = (upper + lower) / 2, delta = (upper - lower) / 2, x = (theta - t) / delta, x0 = theta / delta, k the order,
      variant 0:          1 - t p(t) = T_k(x) / T_k(x0)
      variant 1, k >= 2:  1 - t p(t) = (x + 1) T_{k-1}(x) / ((x0 + 1) T_{k-1}(x0))      (k = 1: p = 1 / theta in both)
  The variant-1 form is not taken from anywhere: test_coefficients passes for variant 1 at orders 2, 3 and 4 only if the
  closed formulas of par_cheby.cpp expand to exactly this polynomial, which they do (roots at x = -1 and at the roots
  of T_{k-1}).

Measured bounds (each against the stated reference, never against the routine under test; test_recorded_measurements_hold
repeats both measurements and fails if they no longer support the recorded figures):
* CG_BOUND:   the same textbook reference run in float64 deviates from its longdouble run by at most 2.11e-15 of the spectral
  scale max(|ritz_min|, |ritz_max|) over all (matrix, scale, steps) cases below; 16 x that = 3.4e-14, below the floor, so the
  floor of 1e-13 is the bound.  (The routine's own largest deviation from the longdouble run was 4.6e-15 when this was written.)
* COEF_BOUND: the closed form evaluated in float64 with numpy.polynomial.chebyshev deviates from the exact expansion by at
  most 1.58e-15 relative, coefficient by coefficient, over the whole parameter grid; 8 x that = 1.264e-14.  (The routine's own
  largest deviation was 1.2e-15.)
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.polynomial import chebyshev as npcheb
from numpy.polynomial import polynomial as nppoly

from util import laplace_3d

EPS = 2.0 ** -52
CG_MEASURED, CG_BOUND = 2.11e-15, 1e-13         # 16 x 2.11e-15 = 3.4e-14 < the floor of 1e-13
COEF_MEASURED, COEF_BOUND = 1.58e-15, 1.264e-14  # 8 x 1.58e-15


# ---------------------------------------------------------------------------------------------------------------------
# matrices: (indptr, indices, data), n <= 400
# ---------------------------------------------------------------------------------------------------------------------
def _csr(rows):
    """rows: per row a list of (column, value) in the order they are to be stored"""
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    indices = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    data = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return indptr, indices, data


def laplacian():
    A = laplace_3d(6, 5, 4)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def neg_laplacian():
    ip, ix, a = laplacian()
    return ip, ix, -a


def random_sdd(n=300, seed=21):
    """Symmetric, strictly diagonally dominant with a positive diagonal (so positive definite); rows of 1 to 25 entries stored in
    a shuffled order (the diagonal anywhere in its row), 12 rows holding the diagonal alone, row 0 holding 25 entries."""
    rng = np.random.default_rng(seed)
    alone = set(rng.choice(np.arange(1, n), 12, replace=False).tolist())
    nb = [dict() for _ in range(n)]
    free = [i for i in range(1, n) if i not in alone]
    for j in rng.choice(free, 24, replace=False):
        v = rng.uniform(-1.0, 1.0)
        nb[0][int(j)] = v
        nb[int(j)][0] = v
    for _ in range(6 * n):
        i, j = (int(v) for v in rng.choice(free, 2, replace=False))
        if j in nb[i] or len(nb[i]) >= 24 or len(nb[j]) >= 24:
            continue
        v = rng.uniform(-1.0, 1.0)
        nb[i][j] = v
        nb[j][i] = v
    rows = []
    for i in range(n):
        row = [(i, sum(abs(v) for v in nb[i].values()) + rng.uniform(0.1, 1.0))] + list(nb[i].items())
        rows.append([row[k] for k in rng.permutation(len(row))])
    return _csr(rows)


def gershgorin_negative(n=200, seed=22):
    """Symmetric chain with a dominant negative diagonal (about -10, couplings in (-1, 1)) except for five rows whose
    diagonal is +2: the discs reach from about -12 to about +4, so |e_min| > |e_max| while e_max > 0."""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-1.0, 1.0, n - 1)
    diag = -rng.uniform(9.0, 10.0, n)
    diag[rng.choice(n, 5, replace=False)] = 2.0
    rows = []
    for i in range(n):
        row = [(i, diag[i])]
        if i > 0:
            row.append((i - 1, off[i - 1]))
        if i < n - 1:
            row.append((i + 1, off[i]))
        rows.append(row)
    return _csr(rows)


def diagonal(entries):
    return _csr([[(i, float(v))] for i, v in enumerate(entries)])


DIAG8 = [0.75, 2.5, -1.25, 4.0, 6.5, -3.0, 9.0, 5.25]                      # both signs, well separated
MATRICES = {
    "laplacian": laplacian, "neg_laplacian": neg_laplacian, "random_sdd": random_sdd, "gershgorin_negative": gershgorin_negative,
    "diag8": lambda: diagonal(DIAG8), "diag8_positive": lambda: diagonal([abs(v) for v in DIAG8]),
    "diag_negative": lambda: diagonal([-3.0, -0.5, -7.25, -2.0]),
    # the awkward inputs of the tridiagonal eigenvalue routine
    "diag_repeated": lambda: diagonal([1.0, 2.0, 2.0, 3.5, 5.0]), "diag_spread": lambda: diagonal([1e-6, 1e-3, 0.5, 7.0, 1e3, 1e6]),
    "diag_1": lambda: diagonal([3.25]), "diag_2": lambda: diagonal([2.0, -5.0]),
}
# compared with the conjugate-gradient reference: definite matrices of either sign and two indefinite ones (the Gershgorin
# matrix and the mixed-sign diagonal one; the tridiagonal matrix of the step lengths is the Lanczos matrix there as well)
CG_MATRICES = ["laplacian", "neg_laplacian", "random_sdd", "gershgorin_negative", "diag8", "diag8_positive"]
QL_MATRICES = ["diag_repeated", "diag_spread", "diag_1", "diag_2"]


class Mat:
    def __init__(self, lib, name, arrays=None):
        from hypre_amd import binding as B
        self.name = name
        self.indptr, self.indices, self.data = arrays if arrays is not None else MATRICES[name]()
        self.n = n = len(self.indptr) - 1
        self._part, self._z = np.array([0, n], dtype=np.int64), np.zeros(n + 1, dtype=np.int32)
        self.h = lib.hypre_amd_ParCSRMatrixFromArrays(0, n, n, B._bp(self._part), B._bp(self._part), 0, None, B._ip(self.indptr),
                                                      B._ip(self.indices), B._rp(self.data), B._ip(self._z), None, None, B.HYPRE_MEMORY_HOST)
        B.check()
        self.csr = sp.csr_matrix((self.data, self.indices, self.indptr), shape=(n, n))
        self.diag = self.csr.diagonal()
        self._dense = {}

    def dense(self, scale, dtype):
        """A, or D^-1/2 A D^-1/2 with D = |diag(A)|, in the given precision"""
        key = (scale, dtype)
        if key not in self._dense:
            M = self.csr.toarray().astype(dtype)
            if scale:
                ds = dtype(1) / np.sqrt(np.abs(self.diag).astype(dtype))
                M = ds[:, None] * M * ds[None, :]
            self._dense[key] = M
        return self._dense[key]


@pytest.fixture(scope="module")
def mats(lib):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Mat(lib, name)
        return built[name]

    yield get
    for m in built.values():
        lib.hypre_ParCSRMatrixDestroy(m.h)


# ---------------------------------------------------------------------------------------------------------------------
# a. Gershgorin discs
# ---------------------------------------------------------------------------------------------------------------------
def gershgorin_reference(indptr, indices, data, scale):
    """(max_eig, min_eig, tolerance).  Discs in exact arithmetic; a row of k entries is summed in stored order by the routine, so
    each edge of its disc carries at most (k + 2) roundings (k - 1 additions, the edge itself, the division by |a_ii|) of
    2^-53 relative to the disc's outer edge |a_ii| + r_i; max and min over the rows move by no more than the largest of these."""
    e_max = e_min = None
    tol = 0.0
    for i in range(len(indptr) - 1):
        cols, vals = indices[indptr[i]:indptr[i + 1]], data[indptr[i]:indptr[i + 1]]
        a_ii = sum((Fraction(float(v)) for c, v in zip(cols, vals) if c == i), Fraction(0))
        r_i = sum((abs(Fraction(float(v))) for c, v in zip(cols, vals) if c != i), Fraction(0))
        lo, hi, edge = a_ii - r_i, a_ii + r_i, abs(a_ii) + r_i
        if scale:
            lo, hi, edge = lo / abs(a_ii), hi / abs(a_ii), edge / abs(a_ii)
        e_max = hi if e_max is None else max(e_max, hi)
        e_min = lo if e_min is None else min(e_min, lo)
        tol = max(tol, (len(cols) + 2) * 2.0 ** -53 * float(edge))
    if abs(e_min) > abs(e_max):
        return float(min(Fraction(0), e_max)), float(e_min), tol
    return float(e_max), float(max(e_min, Fraction(0))), tol


def lib_gershgorin(lib, h, scale):
    from hypre_amd import binding as B
    mx, mn = C.c_double(-77.0), C.c_double(-77.0)
    lib.hypre_ParCSRMaxEigEstimate(h, scale, C.byref(mx), C.byref(mn))
    B.check()
    return mx.value, mn.value


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("name", ["laplacian", "neg_laplacian", "random_sdd", "gershgorin_negative", "diag8", "diag8_positive",
                                  "diag_negative", "diag_1"])
def test_gershgorin_estimate(lib, mats, name, scale):
    m = mats(name)
    mx, mn = lib_gershgorin(lib, m.h, scale)
    rmx, rmn, tol = gershgorin_reference(m.indptr, m.indices, m.data, scale)
    print("%s scale %d: max %r (ref %r) min %r (ref %r) tol %.3e" % (name, scale, mx, rmx, mn, rmn, tol))
    assert abs(mx - rmx) <= tol and abs(mn - rmn) <= tol


def test_gershgorin_matrices_reach_both_sign_branches(mats):
    """no library call: the matrices are what the cases above need"""
    for name, branch in (("gershgorin_negative", "neg"), ("neg_laplacian", "neg"), ("laplacian", "pos"), ("diag_negative", "neg")):
        m = mats(name)
        r = np.abs(m.csr).sum(axis=1).A1 - np.abs(m.diag)
        e_min, e_max = np.min(m.diag - r), np.max(m.diag + r)
        assert (abs(e_min) > 1.5 * abs(e_max)) if branch == "neg" else (abs(e_max) > 1.5 * abs(e_min)), name
    g = mats("gershgorin_negative")
    r = np.abs(g.csr).sum(axis=1).A1 - np.abs(g.diag)
    assert np.max(g.diag + r) > 1.0                      # min(0, e_max) has something to cut
    assert np.max(mats("diag_negative").diag) < 0.0      # ... and here it has not: max_eig stays negative
    s = mats("random_sdd")
    lens = np.diff(s.indptr)
    assert lens.min() == 1 and lens.max() == 25 and np.sum(lens == 1) == 12 and abs(s.csr - s.csr.T).max() == 0.0
    assert not np.all(s.indices[s.indptr[:-1]] == np.arange(s.n))      # the diagonal is not always stored first


# ---------------------------------------------------------------------------------------------------------------------
# b. conjugate gradients / Lanczos
# ---------------------------------------------------------------------------------------------------------------------
def park_miller(n, dtype):
    """minimal-standard generator (a = 16807, m = 2^31 - 1) from seed 1, the first value after one step, mapped to (-1, 1)"""
    s, out = 1, []
    for _ in range(n):
        s = (16807 * s) % 2147483647
        out.append(s)
    return dtype(2) * np.array(out, dtype=dtype) / dtype(2147483647) - dtype(1)


def cg_lanczos(M, steps, dtype):
    """Extreme Ritz values (max, min) after `steps` steps of conjugate gradients on M x = b from x = 0, b the Park-Miller vector.
    Hestenes-Stiefel as in any textbook; the Lanczos matrix of the step lengths (Golub & Van Loan, 4th ed., section 11.3.3;
    Saad, Iterative Methods, section 6.7.3) has
    diagonal 1/alpha_i + beta_i/alpha_{i-1} and off-diagonal sqrt(beta_i)/alpha_{i-1}."""
    n = M.shape[0]
    r = park_miller(n, dtype)
    p = r.copy()
    rho = r @ r
    alpha, beta = [], []
    for _ in range(min(steps, n)):
        if rho < EPS:
            break
        q = M @ p
        a = rho / (p @ q)
        r = r - a * q
        rho_new = r @ r
        b = rho_new / rho
        p = r + b * p
        rho = rho_new
        alpha.append(a)
        beta.append(b)
    k = len(alpha)
    if k == 0:
        return 0.0, 0.0, 0
    T = np.zeros((k, k))
    for i in range(k):
        T[i, i] = float(dtype(1) / alpha[i] + (beta[i - 1] / alpha[i - 1] if i else dtype(0)))
        if i:
            T[i, i - 1] = T[i - 1, i] = float(np.sqrt(beta[i - 1]) / alpha[i - 1])
    ev = np.linalg.eigvalsh(T)
    return float(ev[-1]), float(ev[0]), k


_cg_cache = {}


def cg_reference(m, scale, steps, dtype=np.longdouble):
    key = (m.name, scale, min(steps, m.n), dtype)
    if key not in _cg_cache:
        _cg_cache[key] = cg_lanczos(m.dense(scale, dtype), steps, dtype)
    return _cg_cache[key]


def lib_cg(lib, h, scale, max_iter):
    from hypre_amd import binding as B
    mx, mn = C.c_double(-77.0), C.c_double(-77.0)
    lib.hypre_ParCSRMaxEigEstimateCG(h, scale, max_iter, C.byref(mx), C.byref(mn))
    B.check()
    return mx.value, mn.value


def iters_of(m):
    return [1, 2, 10, m.n, m.n + 5]


def spectrum(m, scale):
    if not hasattr(m, "_spec"):
        m._spec = {}
    if scale not in m._spec:
        M = m.dense(scale, np.float64)
        ev = np.linalg.eigvalsh((M + M.T) / 2)
        m._spec[scale] = (ev[0], ev[-1], np.max(np.sum(np.abs(M), axis=1)))
    return m._spec[scale]


def assert_interlaced(m, scale, steps, mx, mn):
    """Ritz values of a symmetric matrix lie in its spectrum; k steps in floating point widen that by k 2^-52 |M|_inf"""
    lo, hi, norm = spectrum(m, scale)
    w = min(steps, m.n) * EPS * norm
    assert np.isfinite(mx) and np.isfinite(mn)
    assert lo - w <= mn <= mx <= hi + w, (m.name, scale, steps, (lo, hi), (mn, mx), w)


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4], ids=["1", "2", "10", "n", "n+5"])
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("name", CG_MATRICES)
def test_cg_estimate(lib, mats, name, scale, which):
    m = mats(name)
    steps = iters_of(m)[which]
    mx, mn = lib_cg(lib, m.h, scale, steps)
    rmx, rmn, k = cg_reference(m, scale, steps)
    size = max(abs(rmx), abs(rmn))
    dev = max(abs(mx - rmx), abs(mn - rmn)) / size
    print("%s scale %d steps %d (%d taken): max %r (ref %r) min %r (ref %r) deviation %.3e" % (name, scale, steps, k, mx, rmx, mn, rmn, dev))
    # measured: float64 reference against longdouble reference 2.11e-15 at most; 16 x that (3.4e-14) is below the floor of 1e-13
    assert dev <= CG_BOUND
    assert_interlaced(m, scale, steps, mx, mn)


@pytest.mark.parametrize("name", ["diag8", "diag8_positive", "diag_negative", "diag_1", "diag_2"])
def test_cg_estimate_finds_the_ends_of_a_small_diagonal_matrix(lib, mats, name):
    """as many steps as rows: the Krylov space is everything, the tridiagonal matrix has the matrix's own eigenvalues and the
    eigenvalue routine runs at full size"""
    m = mats(name)
    assert m.n <= 8
    for steps in (m.n, m.n + 5):
        mx, mn = lib_cg(lib, m.h, 0, steps)
        size = np.max(np.abs(m.diag))
        print("%s steps %d: max %r min %r of %r" % (name, steps, mx, mn, sorted(m.diag)))
        assert abs(mx - np.max(m.diag)) <= CG_BOUND * size and abs(mn - np.min(m.diag)) <= CG_BOUND * size


@pytest.mark.parametrize("max_iter", [0, -1, -10])
def test_cg_estimate_without_steps_is_zero(lib, mats, max_iter):
    assert lib_cg(lib, mats("laplacian").h, 0, max_iter) == (0.0, 0.0)
    assert lib_cg(lib, mats("laplacian").h, 1, max_iter) == (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# c. the tridiagonal eigenvalue routine on awkward input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("name", QL_MATRICES)
def test_cg_estimate_on_awkward_tridiagonals(lib, mats, name, scale):
    """a repeated eigenvalue (the residual vanishes one step early: the guard on r.r ends the loop), entries over twelve orders
    of magnitude, one and two rows"""
    m = mats(name)
    for steps in iters_of(m):
        mx, mn = lib_cg(lib, m.h, scale, steps)
        print("%s scale %d steps %d: max %r min %r" % (name, scale, steps, mx, mn))
        assert_interlaced(m, scale, steps, mx, mn)
    if name in ("diag_repeated", "diag_1", "diag_2") and scale == 0:
        # small and well separated but for the pair: after n steps the ends are the matrix's
        mx, mn = lib_cg(lib, m.h, 0, m.n)
        size = np.max(np.abs(m.diag))
        assert abs(mx - np.max(m.diag)) <= CG_BOUND * size and abs(mn - np.min(m.diag)) <= CG_BOUND * size


# ---------------------------------------------------------------------------------------------------------------------
# d. coefficients and scaling vector
# ---------------------------------------------------------------------------------------------------------------------
ORDERS, VARIANTS, FRACTIONS = [0, 1, 2, 3, 4, 7], [0, 1], [0.1, 0.3, 0.9]
EIGS = [(3.7, 0.02), (1.0, 0.0), (-0.0, -5.5), (-0.3, -6.0)]


def _pmul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = out[i + j] + x * y
    return out


def _cheb_T(k, x):
    """T_0 .. T_k of the polynomial (or number) x by the three-term recurrence; polynomials as ascending coefficient lists"""
    poly = isinstance(x, list)
    T = [[Fraction(1)] if poly else Fraction(1), x]
    for _ in range(2, k + 1):
        if poly:
            two_x_t = [2 * c for c in _pmul(x, T[-1])]
            prev = T[-2] + [Fraction(0)] * (len(two_x_t) - len(T[-2]))
            T.append([a - b for a, b in zip(two_x_t, prev)])
        else:
            T.append(2 * x * T[-1] - T[-2])
    return T


def interval(max_eig, min_eig, fraction, one_point_one):
    """(theta, delta) in the arithmetic of the arguments"""
    if max_eig <= 0:
        upper, other = min_eig * one_point_one, max_eig
    else:
        upper, other = max_eig * one_point_one, min_eig
    lower = fraction * (upper - other) + other
    return (upper + lower) / 2, (upper - lower) / 2


def exact_coefs(max_eig, min_eig, fraction, order, variant):
    """coefficients of p, ascending, as Fractions: the double inputs taken exactly, 1.1 as 11/10"""
    k = min(max(order, 1), 4)
    theta, delta = interval(Fraction(max_eig), Fraction(min_eig), Fraction(fraction), Fraction(11, 10))
    x, x0 = [theta / delta, -1 / delta], theta / delta
    if variant == 0 or k == 1:
        num, den = _cheb_T(k, x)[k], _cheb_T(k, x0)[k]
    else:
        num, den = _pmul([x[0] + 1, x[1]], _cheb_T(k - 1, x)[k - 1]), (x0 + 1) * _cheb_T(k - 1, x0)[k - 1]
    q = [c / den for c in num]
    assert q[0] == 1 and len(q) == k + 1
    return [-c for c in q[1:]]


def float64_coefs(max_eig, min_eig, fraction, order, variant):
    """the same closed form in float64 with numpy.polynomial (what the bound is measured with)"""
    k = min(max(order, 1), 4)
    theta, delta = interval(float(max_eig), float(min_eig), float(fraction), 1.1)
    x, x0 = nppoly.Polynomial([theta / delta, -1.0 / delta]), theta / delta
    unit = lambda j: [0.0] * j + [1.0]
    if variant == 0 or k == 1:
        num, den = nppoly.Polynomial(npcheb.cheb2poly(unit(k)))(x), npcheb.chebval(x0, unit(k))
    else:
        num = (x + 1.0) * nppoly.Polynomial(npcheb.cheb2poly(unit(k - 1)))(x)
        den = (x0 + 1.0) * npcheb.chebval(x0, unit(k - 1))
    return [-c / den for c in num.coef[1:]]


def coef_deviation(got, exact):
    return max(abs(Fraction(float(g)) - e) / abs(e) for g, e in zip(got, exact))


def lib_setup(lib, h, max_eig, min_eig, fraction, order, scale, variant, n):
    """(coefficients [clamped order + 1], ds or None)"""
    from hypre_amd import binding as B
    cp, dp = B.RealP(), B.RealP()
    lib.hypre_ParCSRRelax_Cheby_Setup(h, max_eig, min_eig, fraction, order, scale, variant, C.byref(cp), C.byref(dp))
    flag = lib.HYPRE_GetError()
    lib.HYPRE_ClearAllErrors()
    k = min(max(order, 1), 4)
    coefs = np.array([cp[i] for i in range(k + 1)])
    ds = np.array([dp[i] for i in range(n)]) if dp else None
    lib.hypre_Free(C.cast(cp, C.c_void_p), B.HYPRE_MEMORY_HOST)
    if dp:
        lib.hypre_Free(C.cast(dp, C.c_void_p), B.HYPRE_MEMORY_HOST)
    return coefs, ds, flag


@pytest.mark.parametrize("max_eig,min_eig", EIGS)
@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", ORDERS)
def test_coefficients(lib, mats, order, variant, fraction, max_eig, min_eig):
    m = mats("diag8")
    coefs, ds, flag = lib_setup(lib, m.h, max_eig, min_eig, fraction, order, 0, variant, m.n)
    assert flag == 0 and ds is None
    k = min(max(order, 1), 4)
    exact = exact_coefs(max_eig, min_eig, fraction, order, variant)
    dev = coef_deviation(coefs[:k], exact)
    print("order %d variant %d fraction %g eig (%r, %r): %r deviation %.3e" % (order, variant, fraction, max_eig, min_eig, list(coefs), float(dev)))
    # measured: the float64 closed form deviates from the exact expansion by 1.58e-15 at most over this grid; 8 x that = 1.264e-14
    assert dev <= COEF_BOUND
    assert coefs[k] == 0.0                               # the array holds one entry more than the polynomial has


def test_variant_1_of_order_1_is_variant_0():
    for mx, mn in EIGS:
        assert exact_coefs(mx, mn, 0.3, 1, 1) == exact_coefs(mx, mn, 0.3, 1, 0)
        theta, _ = interval(Fraction(mx), Fraction(mn), Fraction(0.3), Fraction(11, 10))
        assert exact_coefs(mx, mn, 0.3, 1, 1) == [1 / theta]


def test_recorded_measurements_hold(mats):
    """the two measurements behind CG_BOUND and COEF_BOUND, repeated: reference against reference, no library call"""
    worst = 0.0
    for name in CG_MATRICES:
        m = mats(name)
        for scale in (0, 1):
            for steps in iters_of(m):
                hi, lo, _ = cg_reference(m, scale, steps)
                hi64, lo64, _ = cg_reference(m, scale, steps, np.float64)
                worst = max(worst, max(abs(hi - hi64), abs(lo - lo64)) / max(abs(hi), abs(lo)))
    print("float64 against longdouble conjugate gradients: %.3e" % worst)
    assert worst <= CG_MEASURED and max(16 * CG_MEASURED, 1e-13) == CG_BOUND
    worst = Fraction(0)
    for order in ORDERS:
        for variant in VARIANTS:
            for fraction in FRACTIONS:
                for mx, mn in EIGS:
                    worst = max(worst, coef_deviation(float64_coefs(mx, mn, fraction, order, variant),
                                                      exact_coefs(mx, mn, fraction, order, variant)))
    print("float64 closed form against the exact expansion: %.3e" % float(worst))
    assert worst <= COEF_MEASURED and abs(8 * COEF_MEASURED - COEF_BOUND) < 1e-20


def test_scaling_vector(lib, mats):
    """1 / sqrt(|a_ii|) bit for bit (both operations are correctly rounded), 0 where the diagonal is stored as 0 or not stored
    at all, nothing without scaling"""
    for name in ("laplacian", "neg_laplacian", "random_sdd", "gershgorin_negative", "diag8"):
        m = mats(name)
        _, ds, flag = lib_setup(lib, m.h, 2.0, 0.1, 0.3, 2, 1, 0, m.n)
        assert flag == 0 and np.array_equal(ds.view(np.int64), (1.0 / np.sqrt(np.abs(m.diag))).view(np.int64)), name
        _, ds, flag = lib_setup(lib, m.h, 2.0, 0.1, 0.3, 2, 0, 0, m.n)
        assert flag == 0 and ds is None
    # row 1 stores its diagonal as 0 (after another entry), row 3 stores none
    z = Mat(lib, "zeros", _csr([[(0, 4.0), (1, 1.0)], [(0, 1.0), (1, 0.0)], [(2, -0.25)], [(2, 1.0)], [(3, 1.0), (4, 16.0)]]))
    _, ds, flag = lib_setup(lib, z.h, 2.0, 0.1, 0.3, 2, 1, 0, z.n)
    assert flag != 0                                     # "Zero diagonal found!"
    assert np.array_equal(ds, [0.5, 0.0, 2.0, 0.0, 0.25])
    lib.hypre_ParCSRMatrixDestroy(z.h)


# ---------------------------------------------------------------------------------------------------------------------
# e. a hierarchy uses its own levels' numbers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eig_est,scale,order,variant", [(10, 1, 2, 0), (10, 0, 3, 1), (0, 1, 4, 0), (0, 0, 2, 1)])
def test_hierarchy_levels_get_their_own_numbers(lib, oracle, eig_est, scale, order, variant):
    """Every level's coefficients are those of ITS operator: the estimate of that operator (checked against the references of
    a / b) put through the exact expansion of d.  A wrong level, min and max swapped, or scaling not handed on all show."""
    from hypre_amd import binding as B, ij
    fraction = 0.3
    opt = ij.IJOptions(n=(12, 11, 10), relax_type=16, coarsen_type=8, cheby_eig_est=eig_est, cheby_scale=scale, cheby_order=order,
                       cheby_variant=variant, cheby_fraction=fraction)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_HOST)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    amg = oracle.amg_from_solvers([s])
    nl = len(amg.A_levels)
    assert nl >= 3 and amg.c.cheby_order == order and amg.c.cheby_scale == scale
    smoothed = [l for l in range(nl) if amg.cheby_coefs[l] is not None]
    assert smoothed[:2] == [0, 1] and len(smoothed) >= nl - 1
    seen = []
    for l in smoothed:
        blk = amg.A_levels[l].blocks[0][0]
        m = Mat(lib, "level%d" % l, (blk.indptr, blk.indices, blk.data))
        # the estimate of this level's operator, by the routine and by the reference
        if eig_est:
            mx, mn = lib_cg(lib, m.h, scale, eig_est)
            rmx, rmn, _ = cg_lanczos(m.dense(scale, np.longdouble), eig_est, np.longdouble)
            assert max(abs(mx - rmx), abs(mn - rmn)) <= CG_BOUND * max(abs(rmx), abs(rmn)), l
        else:
            mx, mn = lib_gershgorin(lib, m.h, scale)
            rmx, rmn, tol = gershgorin_reference(m.indptr, m.indices, m.data, scale)
            assert abs(mx - rmx) <= tol and abs(mn - rmn) <= tol, l
        assert mx > 0.0 and 0.0 <= mn < mx
        # the level's coefficients are the polynomial of exactly that estimate
        k = min(max(order, 1), 4)
        dev = coef_deviation(amg.cheby_coefs[l][:k], exact_coefs(mx, mn, fraction, order, variant))
        print("level %d (%d rows): estimate (%r, %r) reference (%r, %r) coefficients %r deviation %.3e"
              % (l, m.n, mx, mn, rmx, rmn, list(amg.cheby_coefs[l]), float(dev)))
        assert dev <= COEF_BOUND, l
        if scale:
            assert np.array_equal(amg.cheby_ds[l].view(np.int64), (1.0 / np.sqrt(np.abs(m.diag))).view(np.int64)), l
        else:
            assert amg.cheby_ds[l] is None, l
        seen.append((mx, mn))
        lib.hypre_ParCSRMatrixDestroy(m.h)
    # the levels differ, so one level's numbers on another would have been seen
    assert len(set(seen)) == len(seen)
    lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)
