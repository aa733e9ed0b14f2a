"""BoomerAMG cycles with ILU as a level smoother (smooth_type 5 | 15), restated in numpy on the hierarchy a solver built.

The hierarchy is the oracle's export of the solver (pyoracle.amg_from_solvers: A_levels, P_levels, smoother diagonals and
weights).  The smoother of a level is a stand-alone HOST HYPRE_ILU set up on that level's matrix with the solver's parameters
and applied with hypre_amd_ILUApplyFactors on host vectors (tests/test_ilu_host.py pins that host solve on its own).  Levels the
smoother does not cover are relaxed with l1-Jacobi (relax 7 | 18), the coarsest of them solved with numpy.linalg.solve.

Every cycle is written twice: in numpy.float64, with the products by the oracle's par_matvec / par_matvecT, and in
numpy.longdouble, with the products summed in long double; the ILU application and the dense solve take and give float64 in
both.  What the two differ by is the rounding of a float64 cycle, the yardstick of the GPU tests.

fma() is a fused multiply-add in exact arithmetic on float64 arrays (python has none before 3.13): the rounding the device
kernels of the accelerated smoother spell out."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

LD = np.longdouble


# ---- an exactly rounded fused multiply-add -------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    c = 134217729.0                      # 2^27 + 1 (Veltkamp split)
    ah = c * a; ah = ah - (ah - a); al = a - ah
    bh = c * b; bh = bh - (bh - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c) with one rounding, elementwise on float64 (Boldo and Melquiond: the exact product and two exact sums,
    the low parts added with rounding to odd, one last rounding to nearest); no overflow or underflow in the operands' range"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    z, err = _two_sum(tl, vl)
    # round to odd: an inexact sum whose last mantissa bit is even moves one unit towards the part that was lost
    even = (z.view(np.int64) & 1) == 0
    fix = (err != 0.0) & even
    z = np.where(fix, np.nextafter(z, np.where(err > 0, np.inf, -np.inf)), z)
    return vh + z


# ---- sparse products in a chosen precision --------------------------------------------------------------------------
class _Csr:
    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.float64), shape
        self.data_ld = self.data.astype(LD)
        self.empty = np.diff(self.indptr) == 0

    def dot_ld(self, x):
        if self.data.size == 0:
            return np.zeros(self.shape[0], LD)
        prod = self.data_ld * x[self.indices]
        out = np.add.reduceat(prod, np.minimum(self.indptr[:-1], prod.size - 1))
        out[self.empty] = 0
        return out

    def transpose(self):
        T = sp.csr_matrix((self.data, self.indices, self.indptr), shape=self.shape).T.tocsr()
        return _Csr(T.indptr, T.indices, T.data, T.shape)


def _eliminate(M, b):
    """Gaussian elimination with partial pivoting in the arrays' own precision (numpy.linalg has no long double)"""
    M, b = M.copy(), np.array(b, dtype=M.dtype)
    n = b.size
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]], b[[k, p]] = M[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            m = M[i, k] / M[k, k]
            M[i, k:] -= m * M[k, k:]
            b[i] -= m * b[k]
    x = np.zeros(n, M.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - np.dot(M[k, k + 1:], x[k + 1:])) / M[k, k]
    return x


def _csr_of(par):
    d = par.blocks[0][0]
    return _Csr(d.indptr, d.indices, d.data, (par.nrows, par.ncols))


class Restatement:
    """One solver's hierarchy and smoothers on the CPU.  Parameters of the smoother as the solver got them."""

    def __init__(self, lib, B, O, solver, smooth_type, smooth_num_levels, smooth_num_sweeps=1, lfil=0, reordering=1, max_iter=1,
                 iterative=0, lower=5, upper=5):
        from util import parcsr
        self.lib, self.B, self.O = lib, B, O
        self.amg = O.amg_from_solvers([solver])
        self.nl = len(self.amg.A_levels)
        self.A = [_csr_of(a) for a in self.amg.A_levels]
        self.P = [_csr_of(p) for p in self.amg.P_levels]
        self.PT = [p.transpose() for p in self.P]
        self.smooth_type, self.sweeps, self.max_iter = smooth_type, smooth_num_sweeps, max_iter
        self.snl = min(smooth_num_levels, self.nl) if smooth_type in (5, 15) else 0
        self.mu = int(self.amg.c.cycle_type)
        self.grid_sweeps = [int(self.amg.c.num_grid_sweeps[k]) for k in range(4)]
        self.types = [int(self.amg.c.grid_relax_type[k]) for k in range(4)]
        self.ilu, self.host_A = [], []
        for l in range(self.snl):
            a = self.A[l]
            M = sp.csr_matrix((a.data, a.indices.astype(np.int32), a.indptr.astype(np.int32)), shape=a.shape)
            hA = parcsr(lib, B, M, B.HYPRE_MEMORY_HOST)
            s = C.c_void_p()
            assert lib.HYPRE_ILUCreate(C.byref(s)) == 0
            lib.HYPRE_ILUSetLevelOfFill(s, lfil)
            lib.HYPRE_ILUSetLocalReordering(s, reordering)
            lib.hypre_amd_ILUSetIterativeTriSolve(s, iterative)
            lib.HYPRE_ILUSetLowerJacobiIters(s, lower)
            lib.HYPRE_ILUSetUpperJacobiIters(s, upper)
            assert lib.HYPRE_ILUSetup(s, hA, None, None) == 0
            B.check()
            self.ilu.append(s); self.host_A.append(hA)
        last = self.nl - 1
        self.dense_coarse = None
        if last >= self.snl:
            a = self.A[last]
            self.dense_coarse = sp.csr_matrix((a.data, a.indices, a.indptr), shape=a.shape).toarray()

    def close(self):
        for s in self.ilu:
            self.lib.HYPRE_ILUDestroy(s)
        for a in self.host_A:
            self.lib.hypre_ParCSRMatrixDestroy(a)
        self.ilu, self.host_A = [], []

    # products: float64 by the oracle, long double by numpy
    def _Ax(self, l, x, dt):
        if dt is LD:
            return self.A[l].dot_ld(x)
        y = np.zeros(self.A[l].shape[0])
        self.O.par_matvec(1.0, self.amg.A_levels[l], np.ascontiguousarray(x), 0.0, y, y)
        return y

    def _Px(self, l, x, dt):
        if dt is LD:
            return self.P[l].dot_ld(x)
        y = np.zeros(self.P[l].shape[0])
        self.O.par_matvec(1.0, self.amg.P_levels[l], np.ascontiguousarray(x), 0.0, y, y)
        return y

    def _PTx(self, l, x, dt):
        if dt is LD:
            return self.PT[l].dot_ld(x)
        y = np.zeros(self.P[l].shape[1])
        self.O.par_matvecT(1.0, self.amg.P_levels[l], np.ascontiguousarray(x), 0.0, y)
        return y

    def apply_factors(self, l, r):
        """(L D^-1 U)^-1 r by the library's host solve; float64 in and out"""
        B, lib = self.B, self.lib
        r64 = np.ascontiguousarray(np.asarray(r, dtype=np.float64))
        fv = B.parvec_from_numpy(r64, location=B.HYPRE_MEMORY_HOST)
        uv = B.parvec_from_numpy(np.zeros(r64.size), location=B.HYPRE_MEMORY_HOST)
        assert lib.hypre_amd_ILUApplyFactors(self.ilu[l], fv, uv) == 0
        z = B.parvec_to_numpy(uv)
        for v in (fv, uv):
            lib.hypre_ParVectorDestroy(v)
        return z

    def ilu_solve(self, l, f, u, zero, dt):
        """HYPRE_ILUSolve(smoother[l], A[l], f, u): max_iter applications u += M^-1 (f - A u); the product is skipped from zero"""
        for _ in range(self.max_iter):
            r = f if zero else f - self._Ax(l, u, dt)
            u = u + self.apply_factors(l, r).astype(dt)
            zero = False
        return u

    def smooth(self, l, cycle_param, f, u, zero, dt):
        if l >= self.snl:
            if l == self.nl - 1:
                assert self.types[3] in (9, 19, 98, 99)
                if dt is LD:
                    return _eliminate(self.dense_coarse.astype(LD), f)
                return np.linalg.solve(self.dense_coarse, f)
            assert self.types[cycle_param] in (7, 18), "the restatement relaxes uncovered levels with l1-Jacobi"
            w, d = dt(self.amg.rw[l]), self.amg.l1[l].astype(dt)
            for _ in range(self.grid_sweeps[cycle_param]):
                u = (w * f) / d if zero else u + w * (f - self._Ax(l, u, dt)) / d
                zero = False
            return u
        if self.smooth_type == 5:
            for _ in range(self.sweeps):
                u = self.ilu_solve(l, f, u, zero, dt)
                zero = False
            return u
        r = f.copy() if zero else f - self._Ax(l, u, dt)
        gamma, p = dt(0), None
        for jj in range(self.sweeps):
            z = np.zeros(r.size, dt)
            for j in range(self.grid_sweeps[cycle_param]):
                z = self.ilu_solve(l, r, z, j == 0, dt)
            gammaold, gamma = gamma, np.dot(r, z)
            if gamma == 0:
                break                         # (the deviation from the reference: U stays)
            p = z if jj == 0 else z + (gamma / gammaold) * p
            v = self._Ax(l, p, dt)
            alfa = gamma / np.dot(p, v)
            u = u + alfa * p
            r = r - alfa * v
        return u

    def _level(self, l, f, u, zero, dt):
        last = l == self.nl - 1
        u = self.smooth(l, 3 if last else 1, f, u, zero, dt)
        if last:
            return u
        for _ in range(1 if l == 0 else self.mu):
            fc = self._PTx(l, f - self._Ax(l, u, dt), dt)
            uc = self._level(l + 1, fc, np.zeros(fc.size, dt), True, dt)
            u = u + self._Px(l, uc, dt)
            u = self.smooth(l, 2, f, u, False, dt)
        return u

    def cycle(self, f, u, zero=False, dt=np.float64):
        dt = LD if dt is LD else np.float64
        return self._level(0, np.asarray(f, dtype=dt), np.asarray(u, dtype=dt), zero, dt)

    def solve(self, f, tol=1e-8, max_iter=100):
        """HYPRE_BoomerAMGSolve from zero: (cycles, relative residual norms after every cycle)"""
        u, hist, zero = np.zeros(f.size), [], True
        nf = np.sqrt(np.dot(f, f))
        while len(hist) < max_iter:
            u = self.cycle(f, u, zero)
            zero = False
            hist.append(np.sqrt(np.sum((self._Ax(0, u, np.float64) - f) ** 2)) / nf)
            if hist[-1] < tol:
                break
        return len(hist), hist

    def pcg(self, b, tol=1e-8, max_iter=200):
        """krylov/pcg.c with two_norm 1 behind one cycle from zero: (iterations, relative residual norms of the recurrence)"""
        x, r = np.zeros(b.size), b.copy()
        bb, hist = np.dot(b, b), []
        s = self.cycle(r, np.zeros(b.size), True)
        p, gamma = s.copy(), np.dot(r, s)
        while len(hist) < max_iter:
            ap = self._Ax(0, p, np.float64)
            alpha = gamma / np.dot(ap, p)
            x, r = x + alpha * p, r - alpha * ap
            hist.append(np.sqrt(np.dot(r, r) / bb))
            if hist[-1] < tol:
                break
            s = self.cycle(r, np.zeros(b.size), True)
            gamma, gamma_old = np.dot(r, s), gamma
            p = s + (gamma / gamma_old) * p
        return len(hist), hist


def clear_of_tolerance(hist, tol):
    """the last two residuals are not within a factor of 2 of the tolerance: a count cannot flip on rounding"""
    return all(not (tol / 2 <= h <= 2 * tol) for h in hist[-2:])
