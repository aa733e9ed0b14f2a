"""Restarted GMRES and BiCGSTAB in numpy, for the ILU tests: the iterations of krylov/gmres.c (right preconditioning, modified
Gram-Schmidt, Givens rotations, convergence tested on the recurrence and confirmed on the residual of x) and
krylov/bicgstab.c, with the operator, the preconditioner and the inner product handed in, so that the same loop runs on one
rank or on the local pieces of several.  A fixed preconditioner makes FlexGMRES the same iteration as GMRES.  Used on the
CPU with the library's host ILU application (hypre_amd_ILUApplyFactors on host vectors) and with Jacobi: what the counts of
the device solvers are compared with."""
import numpy as np


def gmres(matvec, precond, dot, b, k_dim=5, tol=1e-8, max_iter=500):
    """returns (iterations, final relative residual norm, x)"""
    x = np.zeros_like(b)
    b_norm = np.sqrt(dot(b, b))
    r = b - matvec(x)
    r_norm = np.sqrt(dot(r, r))
    eps = tol * (b_norm if b_norm > 0 else r_norm)
    it = 0
    while it < max_iter:
        if r_norm == 0.0 or r_norm <= eps:
            break
        p = [r / r_norm]
        rs = np.zeros(k_dim + 1)
        rs[0] = r_norm
        hh = np.zeros((k_dim + 1, k_dim))
        c, s = np.zeros(k_dim), np.zeros(k_dim)
        i = 0
        while i < k_dim and it < max_iter:
            i += 1
            it += 1
            w = matvec(precond(p[i - 1]))
            for j in range(i):
                hh[j, i - 1] = dot(p[j], w)
                w = w - hh[j, i - 1] * p[j]
            t = np.sqrt(dot(w, w))
            hh[i, i - 1] = t
            p.append(w / t if t != 0.0 else w)
            for j in range(1, i):
                t = hh[j - 1, i - 1]
                hh[j - 1, i - 1] = s[j - 1] * hh[j, i - 1] + c[j - 1] * t
                hh[j, i - 1] = -s[j - 1] * t + c[j - 1] * hh[j, i - 1]
            t = hh[i, i - 1] * hh[i, i - 1] + hh[i - 1, i - 1] * hh[i - 1, i - 1]
            gamma = np.sqrt(t)
            if gamma == 0.0:
                gamma = 1.0e-16
            c[i - 1], s[i - 1] = hh[i - 1, i - 1] / gamma, hh[i, i - 1] / gamma
            rs[i] = -s[i - 1] * rs[i - 1]
            rs[i - 1] = c[i - 1] * rs[i - 1]
            hh[i - 1, i - 1] = s[i - 1] * hh[i, i - 1] + c[i - 1] * hh[i - 1, i - 1]
            r_norm = abs(rs[i])
            if r_norm <= eps:
                break
        y = np.linalg.solve(np.triu(hh[:i, :i]), rs[:i]) if i else np.zeros(0)
        w = np.zeros_like(b)
        for j in range(i):
            w = w + y[j] * p[j]
        x = x + precond(w)
        r = b - matvec(x)
        r_norm = np.sqrt(dot(r, r))                   # the residual of x itself: a count ends only when it is below eps
    return it, (r_norm / b_norm if b_norm > 0 else r_norm), x


def bicgstab(matvec, precond, dot, b, tol=1e-8, max_iter=500):
    """returns (iterations, final relative residual norm, x)"""
    x = np.zeros_like(b)
    r0 = b - matvec(x)
    r, p = r0.copy(), r0.copy()
    b_norm = np.sqrt(dot(b, b))
    res = dot(r0, r0)
    r_norm = np.sqrt(res)
    eps = tol * (b_norm if b_norm > 0 else r_norm)
    it = 0
    if r_norm == 0.0 or r_norm <= eps:
        return it, r_norm / b_norm, x
    while it < max_iter:
        it += 1
        v = precond(p)
        q = matvec(v)
        alpha = res / dot(r0, q)
        x = x + alpha * v
        r = r - alpha * q
        v = precond(r)
        s = matvec(v)
        gamma = dot(r, s) / dot(s, s)
        x = x + gamma * v
        r = r - gamma * s
        r_norm = np.sqrt(dot(r, r))
        if r_norm <= eps:
            r = b - matvec(x)
            r_norm = np.sqrt(dot(r, r))
            if r_norm <= eps:
                break
        beta = 1.0 / res
        res = dot(r0, r)
        beta *= res
        p = p - gamma * q
        p = p * (beta * alpha / gamma)
        p = p + r
    return it, r_norm / b_norm, x


def host_ilu_preconditioner(lib, B, solver, n):
    """z = (L D^-1 U)^-1 r by the library's host solve: hypre_amd_ILUApplyFactors on host vectors from a zero iterate"""
    def apply(r):
        fv = B.parvec_from_numpy(np.ascontiguousarray(r), location=B.HYPRE_MEMORY_HOST)
        uv = B.parvec_from_numpy(np.zeros(n), location=B.HYPRE_MEMORY_HOST)
        assert lib.hypre_amd_ILUApplyFactors(solver, fv, uv) == 0
        z = B.parvec_to_numpy(uv)
        for v in (fv, uv):
            lib.hypre_ParVectorDestroy(v)
        return z
    return apply
