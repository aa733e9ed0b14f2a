"""Host-side mirror of the reference's `ij` driver for the in-scope options
(test/ij.c:521-2245 flags, :4440-4780 solver 0, :5007-5200 solver 1).

Everything numerical happens in libhypre_amd.so; this module only translates
driver options into HYPRE_* calls, the way test/ij.c does.

A new Krylov solver is added in two places: a row of SOLVERS, and a `solve_<method>(opt, A, b, x, comm=0, amg=None)`
wrapper of _solve_krylov that lists its setters.  The command line, check_options, run and the closing lines read the row.
"""
import collections
import ctypes as C

import numpy as np

from . import binding as B

HOST, DEVICE = B.HYPRE_MEMORY_HOST, B.HYPRE_MEMORY_DEVICE

# method: None (BoomerAMG alone), "ILU" (ILU alone) or the Krylov solver, which run() reaches as solve_<method in lower case>;
# precond: "amg" (BoomerAMG), "ds" (diagonal scaling) or "ilu"; tag: what the closing lines call the solver; cli: whether
# the command line takes the id (60 / 61 are served for options built in code only: tests/test_cogmres_cli.py pins the refusal).
# LGMRES is no row: lgmres = 1 runs it in place of GMRES on 3 and 4.  The hybrid solver is chosen by hybrid = 1.
Solver = collections.namedtuple("Solver", "method precond tag cli")
SOLVERS = {
    0: Solver(None, "amg", "BoomerAMG ", True),
    1: Solver("PCG", "amg", "", True),
    2: Solver("PCG", "ds", "", True),
    3: Solver("GMRES", "amg", "GMRES ", True),
    4: Solver("GMRES", "ds", "GMRES ", True),
    9: Solver("BiCGSTAB", "amg", "BiCGSTAB ", True),
    10: Solver("BiCGSTAB", "ds", "BiCGSTAB ", True),
    16: Solver("COGMRES", "amg", "COGMRES ", True),
    17: Solver("COGMRES", "ds", "COGMRES ", True),
    60: Solver("FlexGMRES", "ds", "FlexGMRES ", False),
    61: Solver("FlexGMRES", "amg", "FlexGMRES ", False),
    80: Solver("ILU", "ilu", "hypre_ILU ", True),
    81: Solver("GMRES", "ilu", "GMRES ", True),
    82: Solver("FlexGMRES", "ilu", "FlexGMRES ", True),
}


class IJOptions:
    """Defaults of test/ij.c (:140-420, :1697-1712)."""

    def __init__(self, **kw):
        self.n = (10, 10, 10)
        self.P = None                 # (P, Q, R); default (1, nprocs, 1)
        self.problem = "laplacian"    # laplacian | 27pt | difconv | rotate
        self.alpha = 1.0              # -alpha (rotate: angle in degrees; test/ij.c:11147)
        self.eps = None               # -eps   (rotate: anisotropy, default 0; vardifconv: diffusion scale, default 1)
        self.sys_num_fun = 1          # -sysL <num functions>: systems version of the 7-point operator
        self.c = (1.0, 1.0, 1.0)      # -c cx cy cz
        self.a = (1.0, 1.0, 1.0)      # -a ax ay az (difconv)
        self.solver = 0               # -solver: a key of SOLVERS
        self.lgmres = 0               # options only: 1 runs LGMRES in place of GMRES, solver 4 as DS-LGMRES (the reference's -solver 50),
                                      # solver 3 as AMG-LGMRES (51)
        self.hybrid = 0               # options only: 1 runs the hybrid solver (the reference's -solver 20, test/ij.c:4302-4435): a diagonally
                                      # scaled Krylov solver first, BoomerAMG behind it only if convergence is slower than cf_tol
        self.hybrid_solver_type = 1   # -solver_type: 1 PCG, 2 GMRES, 3 BiCGSTAB (test/ij.c:140, 1963); read with hybrid = 1 only
        self.cf_tol = 0.9             # -cf (test/ij.c:157, 1851); read with hybrid = 1 only
        self.neg_a = 0                # -negA 1: solve with -A (test/ij.c:4014-4017)
        self.num_components = 1       # -nc: columns of b and x (multivectors; test/ij.c:874-878, 3400-3404)
        self.k_dim = 5                # -k (GMRES restart length, test/ij.c:1731)
        self.aug_dim = 2              # -aug (LGMRES: augmentation vectors, test/ij.c:1736, :1761); read with lgmres = 1 only
        self.cgs = 1                  # -cgs (COGMRES: 1 classical Gram-Schmidt, 2 with reorthogonalisation; test/ij.c:1746-1750)
        self.unroll = 0               # -unroll (COGMRES: host loop unrolling of the reference; accepted, no effect; test/ij.c:1751-1755)
        self.flex = 0                 # -flex (flexible PCG: Polak-Ribiere beta)
        self.rhs = "one"              # one (-rhsisone default) | rand (-rhsrand) | xisone
        self.fromfile = None          # -fromfile <name>: matrix from IJ text files <name>.<rank %05d>
        self.rhsfromfile = None       # -rhsfromfile <name>: right-hand side from IJ text files
        self.coarsen_type = 10
        self.interp_type = 6
        self.P_max_elmts = 4
        self.trunc_factor = 0.0
        self.strong_threshold = 0.25
        self.max_row_sum = 1.0
        self.relax_type = -1          # -rlx
        self.relax_down = -1
        self.relax_up = -1
        self.relax_coarse = -1
        self.relax_order = 0          # -CF
        self.num_sweeps = 1           # -ns
        self.relax_wt = 1.0           # -w
        self.outer_wt = 1.0           # -ow
        self.cycle_type = 1           # -mu
        self.fcycle = 0
        self.max_levels = 25
        self.coarse_threshold = 9
        self.tol = 1.0e-8
        self.mg_max_iter = 100
        self.max_iter = 1000
        self.two_norm = 1
        self.precon_cycles = 1
        self.keep_transpose = 1
        self.num_threads = 1
        self.num_functions = 1        # -nf (systems of PDEs, unknown approach)
        self.filter_functions = 0     # -ff
        self.ns_down = self.ns_up = self.ns_coarse = -1   # -ns_down / -ns_up / -ns_coarse
        self.level_w = None           # -wl  value level
        self.level_ow = None          # -owl value level
        self.mixed = False            # fp32 matrix values inside the cycle (extension)
        self.cheby_order = 2          # -cheby_order    (test/ij.c:330-336 defaults)
        self.cheby_eig_est = 10       # -cheby_eig_est
        self.cheby_variant = 0        # -cheby_variant
        self.cheby_scale = 1          # -cheby_scale
        self.cheby_fraction = 0.3     # -cheby_fraction
        self.ilu_type = 0             # -ilu_type       (test/ij.c:447-457 defaults); 0, block Jacobi with ILU(k), is what this driver serves
        self.ilu_lfil = 0             # -ilu_lfil       level of fill k
        self.ilu_reordering = 1       # -ilu_reordering 0 none, 1 reverse Cuthill-McKee on the diagonal block
        self.ilu_tri_solve = 1        # -ilu_tri_solve  1 direct triangular solves (0 is refused: the iterative solves are the three fields below)
        self.ilu_iterative = 0        # 1: triangular solves as Jacobi sweeps (hypre_amd_ILUSetIterativeTriSolve); no command-line flag
        self.ilu_ljac_iters = 5       # sweeps of the lower solve (HYPRE_ILUSetLowerJacobiIters; test/ij.c default 5)
        self.ilu_ujac_iters = 5       # sweeps of the upper solve (HYPRE_ILUSetUpperJacobiIters)
        self.ilu_sm_max_iter = 1      # -ilu_sm_max_iter: applications per call of ILU as a BoomerAMG smoother (HYPRE_BoomerAMGSetILUMaxIter)
        # ILU as a level smoother of BoomerAMG (solvers 0, 1, 3), with the ilu_* fields above as its parameters; options only: the
        # command line keeps refusing -smtype / -smlv
        self.smooth_type = 6          # 5: ILU; 15: ILU inside conjugate-gradient steps; anything else has no effect
        self.smooth_num_levels = 0    # levels, from the finest, the smoother replaces the relaxation on
        self.smooth_num_sweeps = 1    # type 5: applications per level visit; type 15: conjugate-gradient steps
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown ij option %r" % k)
            setattr(self, k, v)


def stencil_values(opt):
    """test/ij.c:9703-9719 (laplacian), :10984-10993 (27pt), :10184-10215 (difconv)."""
    nx, ny, nz = opt.n
    cx, cy, cz = opt.c
    if opt.problem == "laplacian":
        v = np.zeros(4)
        v[1], v[2], v[3] = -cx, -cy, -cz
        if nx > 1:
            v[0] += 2.0 * cx
        if ny > 1:
            v[0] += 2.0 * cy
        if nz > 1:
            v[0] += 2.0 * cz
        return v
    if opt.problem == "27pt":
        v = np.zeros(2)
        v[0] = 26.0
        if nx == 1 or ny == 1 or nz == 1:
            v[0] = 8.0
        if nx * ny == 1 or nx * nz == 1 or ny * nz == 1:
            v[0] = 2.0
        v[1] = -1.0
        return v
    if opt.problem == "difconv":
        ax, ay, az = opt.a
        hinx, hiny, hinz = 1.0 / (nx + 1), 1.0 / (ny + 1), 1.0 / (nz + 1)
        v = np.zeros(7)
        # atype 0: forward differencing of the convection term (ij.c:10184-10215)
        if nx > 1:
            v[0] += 2.0 * cx / (hinx * hinx) - 1.0 * ax / hinx
        if ny > 1:
            v[0] += 2.0 * cy / (hiny * hiny) - 1.0 * ay / hiny
        if nz > 1:
            v[0] += 2.0 * cz / (hinz * hinz) - 1.0 * az / hinz
        v[1] = -cx / (hinx * hinx)
        v[2] = -cy / (hiny * hiny)
        v[3] = -cz / (hinz * hinz)
        v[4] = -cx / (hinx * hinx) + ax / hinx
        v[5] = -cy / (hiny * hiny) + ay / hiny
        v[6] = -cz / (hinz * hinz) + az / hinz
        return v
    raise ValueError(opt.problem)


def build_matrix(opt, comm=0, rank=0, nprocs=1):
    """Rank (p,q,r) = (id % P, (id / P) % Q, id / (P*Q))   (test/ij.c:9693-9695); -negA 1: the operator times -1
    (test/ij.c:4014-4017 hypre_ParCSRMatrixScale(A, -1): test/TEST_ij/posneg.jobs)."""
    A = _build_matrix(opt, comm=comm, rank=rank, nprocs=nprocs)
    if opt.neg_a:
        for blk in (A.contents.diag.contents, A.contents.offd.contents):
            if blk.num_nonzeros > 0:
                np.ctypeslib.as_array(blk.data, shape=(blk.num_nonzeros,))[:] *= -1.0
    return A


def _build_matrix(opt, comm=0, rank=0, nprocs=1):
    if opt.fromfile:
        return read_matrix(opt.fromfile, comm=comm)
    P, Q, R = opt.P if opt.P else (1, nprocs, 1)     # test/ij.c BuildParLaplacian: P = 1, Q = num_procs, R = 1
    if P * Q * R != nprocs:
        raise ValueError("P*Q*R must equal the number of ranks")
    p, q, r = rank % P, (rank // P) % Q, rank // (P * Q)
    if opt.problem == "rotate":
        # test/ij.c:11130-11240 BuildParRotate7pt: a 2-D problem, -n and -P read two values each
        if R != 1:
            raise ValueError("-rotate is two-dimensional: R must be 1")
        A = B.load_library().GenerateRotate7pt(comm, opt.n[0], opt.n[1], P, Q, p, q, opt.alpha,
                                               0.0 if opt.eps is None else opt.eps)
        B.check()
        return A
    if opt.problem == "vardifconv":
        # test/ij.c:11260-11370 BuildParVarDifConv; the right-hand side it returns is all ones (build_rhs_host)
        nx, ny, nz = opt.n
        A = B.load_library().GenerateVarDifConv(comm, nx, ny, nz, P, Q, R, p, q, r, 1.0 if opt.eps is None else opt.eps, None)
        B.check()
        return A
    kind = {"laplacian": "7pt", "27pt": "27pt", "difconv": "difconv"}[opt.problem]
    nx, ny, nz = opt.n
    if opt.sys_num_fun > 1:
        # test/ij.c:9718-9870: coupling matrix of -sysL_opt 0
        mtrx = {2: [2.0, 1.0, 1.0, 2.0], 3: [2.0, 1.0, 0.0, 1.0, 2.0, 1.0, 0.0, 1.0, 2.0]}.get(opt.sys_num_fun)
        if mtrx is None or opt.problem != "laplacian":
            raise ValueError("-sysL supports 2 or 3 functions of the 7-point operator")
        L = B.load_library()
        vals = np.ascontiguousarray(stencil_values(opt), dtype=np.float64)
        m = np.ascontiguousarray(mtrx, dtype=np.float64)
        A = L.GenerateSysLaplacian(comm, nx, ny, nz, P, Q, R, p, q, r, opt.sys_num_fun,
                                   m.ctypes.data_as(C.POINTER(C.c_double)), vals.ctypes.data_as(C.POINTER(C.c_double)))
        B.check()
        return A
    return B.laplacian(nx, ny, nz, P, Q, R, p, q, r, comm=comm, values=stencil_values(opt), kind=kind)


def read_matrix(name, comm=0):
    """test/ij.c:2824-2833 (build_matrix_type -1): HYPRE_IJMatrixRead + GetObject; the IJ shell is dropped and
    the ParCSR matrix lives on (host memory)."""
    L = B.load_library()
    ij = C.POINTER(B.IJMatrix)()
    L.HYPRE_IJMatrixRead(name.encode(), comm, B.HYPRE_PARCSR, C.byref(ij))
    B.check()
    obj = C.c_void_p()
    L.HYPRE_IJMatrixGetObject(ij, C.byref(obj))
    A = C.cast(obj, C.POINTER(B.ParCSRMatrix))
    ij.contents.object = None          # keep the matrix, free the shell
    L.HYPRE_IJMatrixDestroy(ij)
    return A


def read_vector(name, comm=0):
    """test/ij.c:3406-3432 (build_rhs_type 0): the local slice as a numpy array."""
    L = B.load_library()
    ij = C.POINTER(B.IJVector)()
    L.HYPRE_IJVectorRead(name.encode(), comm, B.HYPRE_PARCSR, C.byref(ij))
    B.check()
    obj = C.c_void_p()
    L.HYPRE_IJVectorGetObject(ij, C.byref(obj))
    vals = B.parvec_to_numpy(C.cast(obj, C.POINTER(B.ParVector)))
    L.HYPRE_IJVectorDestroy(ij)
    return vals


class HypreRand:
    """utilities/random.c (Park-Miller), used by -rhsrand."""

    def __init__(self, seed):
        m = 2147483647
        self.seed = min(max(seed, 1), m - 1)

    def next(self):
        a, m, q, r = 16807, 2147483647, 127773, 2836
        high, low = divmod(self.seed, q)
        test = a * low - r * high
        self.seed = test if test > 0 else test + m
        return self.seed / m


def build_rhs_host(opt, A, rank=0, allreduce=None):
    """(b, x0) as numpy arrays for this rank (test/ij.c:3465-3600)."""
    n = A.contents.diag.contents.num_rows
    if opt.rhsfromfile:
        b = read_vector(opt.rhsfromfile, comm=A.contents.comm)
        if len(b) != n:
            raise ValueError("right-hand side file holds %d entries for %d local rows" % (len(b), n))
        return b, np.zeros(n)
    if opt.problem == "vardifconv":
        # test/ij.c:2877-2879, 3856-3887: b from the generator (ones), random initial guess seeded with the rank
        rng = HypreRand(rank)
        return np.ones(n), np.array([rng.next() for _ in range(n)])
    if opt.rhs == "one":
        return np.ones(n), np.zeros(n)
    if opt.rhs == "rand":
        # HYPRE_ParVectorSetRandomValues(b, 22775): seed * (rank + 1) on every rank, then normalise
        rng = HypreRand(22775 * (rank + 1))
        b = np.array([2.0 * rng.next() - 1.0 for _ in range(n)])
        # the reference accumulates the dot product serially
        nrm2 = 0.0
        for v in b:
            nrm2 += v * v
        if allreduce is not None:
            nrm2 = allreduce(nrm2)
        return b * (1.0 / np.sqrt(nrm2)), np.zeros(n)
    if opt.rhs == "xisone":
        return None, np.zeros(n)      # b = A * ones is formed by the caller (needs a product)
    raise ValueError(opt.rhs)


def create_amg(opt, memory_location=DEVICE):
    """test/ij.c:4440-4660: the setter sequence of solver 0 / the preconditioner."""
    L = B.load_library()
    s = C.c_void_p()
    L.HYPRE_BoomerAMGCreate(C.byref(s))
    L.hypre_amd_BoomerAMGSetMemoryLocation(s, memory_location)
    L.hypre_amd_BoomerAMGSetNumThreads(s, opt.num_threads)
    L.HYPRE_BoomerAMGSetInterpType(s, opt.interp_type)
    L.HYPRE_BoomerAMGSetCoarsenType(s, opt.coarsen_type)
    L.HYPRE_BoomerAMGSetTol(s, opt.tol)
    L.HYPRE_BoomerAMGSetStrongThreshold(s, opt.strong_threshold)
    L.HYPRE_BoomerAMGSetMaxCoarseSize(s, opt.coarse_threshold)
    L.HYPRE_BoomerAMGSetTruncFactor(s, opt.trunc_factor)
    L.HYPRE_BoomerAMGSetPMaxElmts(s, opt.P_max_elmts)
    L.HYPRE_BoomerAMGSetCycleType(s, opt.cycle_type)
    L.HYPRE_BoomerAMGSetFCycle(s, opt.fcycle)
    L.HYPRE_BoomerAMGSetNumSweeps(s, opt.num_sweeps)
    if opt.relax_type > -1:
        L.HYPRE_BoomerAMGSetRelaxType(s, opt.relax_type)
    if opt.relax_down > -1:
        L.HYPRE_BoomerAMGSetCycleRelaxType(s, opt.relax_down, 1)
    if opt.relax_up > -1:
        L.HYPRE_BoomerAMGSetCycleRelaxType(s, opt.relax_up, 2)
    if opt.relax_coarse > -1:
        L.HYPRE_BoomerAMGSetCycleRelaxType(s, opt.relax_coarse, 3)
    L.HYPRE_BoomerAMGSetRelaxOrder(s, opt.relax_order)
    L.HYPRE_BoomerAMGSetRelaxWt(s, opt.relax_wt)
    L.HYPRE_BoomerAMGSetOuterWt(s, opt.outer_wt)
    L.HYPRE_BoomerAMGSetMaxLevels(s, opt.max_levels)
    L.HYPRE_BoomerAMGSetMaxRowSum(s, opt.max_row_sum)
    L.HYPRE_BoomerAMGSetMaxIter(s, opt.mg_max_iter)
    L.HYPRE_BoomerAMGSetKeepTranspose(s, opt.keep_transpose)
    L.HYPRE_BoomerAMGSetNumFunctions(s, opt.num_functions)
    L.HYPRE_BoomerAMGSetFilterFunctions(s, opt.filter_functions)
    for k, sweeps in ((1, opt.ns_down), (2, opt.ns_up), (3, opt.ns_coarse)):
        if sweeps > -1:
            L.HYPRE_BoomerAMGSetCycleNumSweeps(s, sweeps, k)
    if opt.level_w is not None:
        L.HYPRE_BoomerAMGSetLevelRelaxWt(s, opt.level_w[0], opt.level_w[1])
    if opt.level_ow is not None:
        L.HYPRE_BoomerAMGSetLevelOuterWt(s, opt.level_ow[0], opt.level_ow[1])
    if opt.mixed:
        L.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    L.HYPRE_BoomerAMGSetChebyOrder(s, opt.cheby_order)
    L.HYPRE_BoomerAMGSetChebyFraction(s, opt.cheby_fraction)
    L.HYPRE_BoomerAMGSetChebyEigEst(s, opt.cheby_eig_est)
    L.HYPRE_BoomerAMGSetChebyVariant(s, opt.cheby_variant)
    L.HYPRE_BoomerAMGSetChebyScale(s, opt.cheby_scale)
    if opt.smooth_num_levels > 0:
        # test/ij.c:4590-4640: the type before the level count (the count is refused while the type is not 5 | 15)
        L.HYPRE_BoomerAMGSetSmoothType(s, opt.smooth_type)
        L.HYPRE_BoomerAMGSetSmoothNumLevels(s, opt.smooth_num_levels)
        L.HYPRE_BoomerAMGSetSmoothNumSweeps(s, opt.smooth_num_sweeps)
        L.HYPRE_BoomerAMGSetILUType(s, opt.ilu_type)
        L.HYPRE_BoomerAMGSetILULevel(s, opt.ilu_lfil)
        L.HYPRE_BoomerAMGSetILULocalReordering(s, opt.ilu_reordering)
        L.HYPRE_BoomerAMGSetILUMaxIter(s, opt.ilu_sm_max_iter)
        L.HYPRE_BoomerAMGSetILUTriSolve(s, 0 if opt.ilu_iterative else 1)
        L.HYPRE_BoomerAMGSetILULowerJacobiIters(s, opt.ilu_ljac_iters)
        L.HYPRE_BoomerAMGSetILUUpperJacobiIters(s, opt.ilu_ujac_iters)
    B.check()
    return s


# ---------------------------------------------------------------------------
# command line of the reference driver (test/ij.c:521-2260), in-scope subset
# ---------------------------------------------------------------------------
# flag -> (attribute, converter, number of values); tuples of floats/ints for multi-valued flags
_VALUE_FLAGS = {
    "-solver": ("solver", int, 1), "-rlx": ("relax_type", int, 1), "-rlx_down": ("relax_down", int, 1),
    "-rlx_up": ("relax_up", int, 1), "-rlx_coarse": ("relax_coarse", int, 1), "-ns": ("num_sweeps", int, 1),
    "-ns_down": ("ns_down", int, 1), "-ns_up": ("ns_up", int, 1), "-ns_coarse": ("ns_coarse", int, 1),
    "-w": ("relax_wt", float, 1), "-ow": ("outer_wt", float, 1), "-CF": ("relax_order", int, 1),
    "-mu": ("cycle_type", int, 1), "-th": ("strong_threshold", float, 1), "-mxrs": ("max_row_sum", float, 1),
    "-tr": ("trunc_factor", float, 1), "-Pmx": ("P_max_elmts", int, 1), "-interptype": ("interp_type", int, 1),
    "-tol": ("tol", float, 1), "-max_iter": ("max_iter", int, 1), "-mg_max_iter": ("mg_max_iter", int, 1),
    "-mxl": ("max_levels", int, 1), "-coarse_th": ("coarse_threshold", int, 1), "-keepT": ("keep_transpose", int, 1),
    "-precon_cycles": ("precon_cycles", int, 1), "-k": ("k_dim", int, 1), "-cgs": ("cgs", int, 1), "-unroll": ("unroll", int, 1), "-nc": ("num_components", int, 1), "-negA": ("neg_a", int, 1), "-nf": ("num_functions", int, 1), "-flex": ("flex", int, 1),
    "-alpha": ("alpha", float, 1), "-eps": ("eps", float, 1), "-sysL": ("sys_num_fun", int, 1), "-ff": ("filter_functions", int, 1),
    "-cheby_order": ("cheby_order", int, 1), "-cheby_eig_est": ("cheby_eig_est", int, 1),
    "-cheby_variant": ("cheby_variant", int, 1), "-cheby_scale": ("cheby_scale", int, 1),
    "-cheby_fraction": ("cheby_fraction", float, 1),
    "-ilu_type": ("ilu_type", int, 1), "-ilu_lfil": ("ilu_lfil", int, 1), "-ilu_reordering": ("ilu_reordering", int, 1),
    "-ilu_tri_solve": ("ilu_tri_solve", int, 1), "-ilu_trisolve": ("ilu_tri_solve", int, 1),    # the reference parses the second spelling, its help shows the first
    "-ilu_sm_max_iter": ("ilu_sm_max_iter", int, 1),
    "-n": ("n", int, 3), "-P": ("P", int, 3), "-c": ("c", float, 3), "-a": ("a", float, 3),
    # extensions of this driver (no reference counterpart)
    "-amd_threads": ("num_threads", int, 1),
}
_SWITCH_FLAGS = {
    "-laplacian": ("problem", "laplacian"), "-27pt": ("problem", "27pt"), "-difconv": ("problem", "difconv"),
    "-rotate": ("problem", "rotate"), "-vardifconv": ("problem", "vardifconv"), "-rhsrand": ("rhs", "rand"), "-rhsisone": ("rhs", "one"), "-xisone": ("rhs", "xisone"),
    "-pmis": ("coarsen_type", 8), "-pmis1": ("coarsen_type", 9), "-hmis": ("coarsen_type", 10),
    "-fmg": ("fcycle", 1), "-amd_mixed": ("mixed", True),
}


def parse_cli(argv):
    """Reference `ij` flags -> IJOptions.  Flags outside the scope of this library are an error, never
    silently dropped."""
    opt = IJOptions()
    i = 0
    while i < len(argv):
        flag = argv[i]
        if flag in _SWITCH_FLAGS:
            attr, val = _SWITCH_FLAGS[flag]
            setattr(opt, attr, val)
            i += 1
        elif flag in _VALUE_FLAGS:
            attr, conv, count = _VALUE_FLAGS[flag]
            vals = [conv(v) for v in argv[i + 1:i + 1 + count]]
            if len(vals) != count:
                raise SystemExit("ij: %s needs %d value(s)" % (flag, count))
            setattr(opt, attr, vals[0] if count == 1 else tuple(vals))
            i += 1 + count
        elif flag in ("-fromfile", "-rhsfromfile"):
            if i + 1 >= len(argv):
                raise SystemExit("ij: %s needs a file name" % flag)
            setattr(opt, flag[1:], argv[i + 1])
            i += 2
        elif flag == "-rap":
            # test/ij.c:2157-2161 rap2: 0 = the Galerkin triple product this library builds (the default)
            if i + 1 >= len(argv) or int(argv[i + 1]) != 0:
                raise SystemExit("ij: -rap 1 (two-product coarse operator) is outside the scope of this driver")
            i += 2
        elif flag in ("-wl", "-owl"):
            val, lev = float(argv[i + 1]), int(argv[i + 2])
            if lev > -1:        # test/ij.c:4543-4550 applies the level weight only for level > -1
                setattr(opt, "level_w" if flag == "-wl" else "level_ow", (val, lev))
            i += 3
        elif flag.startswith("-ilu_"):
            # -ilu_droptol, -ilu_max_row_nnz (ILUT), -ilu_schur_max_iter, -ilu_nsh_droptol (Schur types), -ilu_ljac_iters,
            # -ilu_ujac_iters (iterative triangular solves), -ilu_iter_setup_* (iterative setup)
            raise SystemExit("ij: option %s is outside the scope of this driver (ILU: -ilu_type 0, -ilu_lfil, -ilu_reordering, "
                             "-ilu_tri_solve 1, -ilu_sm_max_iter)" % flag)
        else:
            raise SystemExit("ij: option %s is outside the scope of this driver" % flag)
    if not (opt.solver in SOLVERS and SOLVERS[opt.solver].cli):
        raise SystemExit("ij: -solver %d is outside the scope of this driver (0 AMG, 1 AMG-PCG, 2 DS-PCG, 3 AMG-GMRES, 4 DS-GMRES, "
                         "9 AMG-BiCGSTAB, 10 DS-BiCGSTAB, 16 AMG-COGMRES, 17 DS-COGMRES, 80 ILU, 81 ILU-GMRES, 82 ILU-FlexGMRES)" % opt.solver)
    if opt.interp_type not in (6, 3):
        # extended (14) and ext+i-if-no-common-C (7) are served by run() for options built in code; the command line keeps
        # refusing them: tests/test_ij_cli.py pins -interptype 7 as outside its scope
        raise SystemExit("ij: -interptype %d is outside the scope of this driver (6 ext+i, 3 direct)" % opt.interp_type)
    return check_options(opt)


def check_options(opt):
    """The combinations of options this driver serves, whether they came from the command line or were set in code
    (solvers 60 / 61, FlexGMRES, and lgmres = 1, only the latter); returns opt."""
    if opt.solver not in SOLVERS:
        raise SystemExit("ij: solver %d is outside the scope of this driver" % opt.solver)
    spec = SOLVERS[opt.solver]
    if opt.ilu_type != 0:
        raise SystemExit("ij: -ilu_type %d is outside the scope of this driver (0: block Jacobi with ILU(k); ILUT and the Schur, NSH, "
                         "RAS, ddPQ and RAP types are not served)" % opt.ilu_type)
    if opt.ilu_tri_solve != 1:
        raise SystemExit("ij: -ilu_tri_solve %d is outside the scope of this driver (1: direct triangular solves)" % opt.ilu_tri_solve)
    if opt.ilu_iterative not in (0, 1) or opt.ilu_ljac_iters < 0 or opt.ilu_ujac_iters < 0:
        raise SystemExit("ij: ilu_iterative is 0 (direct triangular solves) or 1 (Jacobi sweeps), ilu_ljac_iters and ilu_ujac_iters are >= 0")
    if opt.ilu_lfil < 0 or opt.ilu_reordering not in (0, 1):
        raise SystemExit("ij: -ilu_lfil takes a level of fill >= 0, -ilu_reordering 0 (none) or 1 (reverse Cuthill-McKee)")
    if opt.smooth_num_levels < 0 or opt.smooth_num_sweeps < 1 or opt.ilu_sm_max_iter < 0:
        raise SystemExit("ij: smooth_num_levels is >= 0, smooth_num_sweeps >= 1, -ilu_sm_max_iter >= 0")
    if opt.smooth_num_levels > 0:
        if opt.smooth_type not in (5, 15):
            raise SystemExit("ij: smooth_num_levels %d with smooth_type %d: the level smoothers served are 5 (ILU) and 15 (ILU inside "
                             "conjugate-gradient steps)" % (opt.smooth_num_levels, opt.smooth_type))
        if opt.num_components > 1:
            raise SystemExit("ij: -nc %d: ILU smoothing doesn't support multicomponent vectors" % opt.num_components)
        if opt.P is not None and int(np.prod(opt.P)) > 1:
            raise SystemExit("ij: ILU smoothing (smooth_type 5 | 15) on more than one rank is outside the scope of this driver")
        if opt.mixed:
            raise SystemExit("ij: ILU smoothing (smooth_type 5 | 15) doesn't support the mixed-precision hierarchy")
        if spec.precond != "amg" or opt.hybrid:
            raise SystemExit("ij: smooth_num_levels is read by BoomerAMG alone or behind PCG or GMRES (-solver 0 | 1 | 3 and their kin)")
    if spec.precond == "ilu" and (opt.num_components > 1 or opt.lgmres or opt.hybrid):
        raise SystemExit("ij: -solver %d (ILU) takes one component, and neither LGMRES nor the hybrid solver" % opt.solver)
    if opt.hybrid not in (0, 1) or (opt.hybrid and opt.solver != 0):
        raise SystemExit("ij: hybrid = %r with solver %d: the hybrid solver is chosen by hybrid = 1 alone, solver stays at its default"
                         % (opt.hybrid, opt.solver))
    if not opt.hybrid and (opt.hybrid_solver_type != 1 or opt.cf_tol != 0.9):
        raise SystemExit("ij: hybrid_solver_type and cf_tol are read by the hybrid solver only (hybrid = 1)")
    if opt.hybrid and (opt.hybrid_solver_type not in (1, 2, 3) or not 0.0 <= opt.cf_tol <= 1.0):
        raise SystemExit("ij: hybrid_solver_type is 1 (PCG), 2 (GMRES) or 3 (BiCGSTAB), cf_tol lies in [0, 1]")
    if opt.hybrid and (opt.num_components > 1 or opt.lgmres):
        raise SystemExit("ij: the hybrid solver takes one component and no LGMRES")
    if opt.lgmres not in (0, 1) or (opt.lgmres and opt.solver not in (3, 4)):
        raise SystemExit("ij: lgmres = %r with solver %d: LGMRES runs as solver 4 (DS-LGMRES, the reference's 50) or solver 3 "
                         "(AMG-LGMRES, 51)" % (opt.lgmres, opt.solver))
    if opt.aug_dim != 2 and not opt.lgmres:
        raise SystemExit("ij: aug_dim = %r is read by LGMRES only (lgmres = 1 with solver 3 | 4)" % opt.aug_dim)
    if opt.num_components < 1 or (opt.num_components > 1 and (opt.rhs != "one" or opt.rhsfromfile)):
        # test/ij.c:3400-3404 takes several components with the constant right-hand sides only
        raise SystemExit("ij: -nc %d needs -rhsisone in this driver" % opt.num_components)
    if opt.num_components > 1 and spec.method == "COGMRES":
        raise SystemExit("ij: -nc %d with -solver %d: COGMRES doesn't take multicomponent vectors in this driver (GMRES, -solver 3 | 4, does)"
                         % (opt.num_components, opt.solver))
    if opt.num_components > 1 and spec.precond == "amg":
        # BoomerAMG on multivectors (hypre_BoomerAMGSolve with num_vectors > 1) serves l1-Jacobi / Jacobi 7 / 18 and two-stage
        # Gauss-Seidel 11 / 12 over all points with a direct coarsest-level solve; the reference refuses hybrid Gauss-Seidel
        # (the defaults 13 / 14) with multicomponent vectors as well
        why = multivector_amg_refusal(opt)
        if why:
            raise SystemExit("ij: -nc %d with -solver %d: %s" % (opt.num_components, opt.solver, why))
    if opt.interp_type not in (6, 7, 14, 3):
        raise SystemExit("ij: interp_type %d is outside the scope of this driver (6 ext+i, 7 ext+i if no common C point, "
                         "14 extended, 3 direct)" % opt.interp_type)
    smoothers = (-1, 0, 3, 4, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 88, 89)
    for name in ("relax_type", "relax_down", "relax_up"):
        if getattr(opt, name) not in smoothers:
            raise SystemExit("ij: smoother %d is outside the scope of this driver" % getattr(opt, name))
    if opt.relax_coarse not in smoothers + (9, 19, 98, 99):
        raise SystemExit("ij: coarse solver %d is outside the scope of this driver" % opt.relax_coarse)
    weights = [opt.relax_wt, opt.outer_wt] + [w[0] for w in (opt.level_w, opt.level_ow) if w is not None]
    if any(w < 0 for w in weights):
        raise SystemExit("ij: negative (automatically estimated) relaxation weights are outside the scope of this driver")
    return opt


def resolved_smoothers(opt):
    """The smoothers (down, up, coarsest) the options give a hierarchy: HYPRE_BoomerAMGSetRelaxType sets the first two and the
    direct solve 9 on the coarsest level, -rlx_down / -rlx_up / -rlx_coarse override them (defaults 13 / 14 / 9)."""
    down = opt.relax_down if opt.relax_down > -1 else (opt.relax_type if opt.relax_type > -1 else 13)
    up = opt.relax_up if opt.relax_up > -1 else (opt.relax_type if opt.relax_type > -1 else 14)
    coarse = opt.relax_coarse if opt.relax_coarse > -1 else 9
    return down, up, coarse


def multivector_amg_refusal(opt):
    """Why BoomerAMG cannot take -nc N columns with these options ("" when it can): the smoothers and switches that
    hypre_BoomerAMGSolve serves on multivectors."""
    down, up, coarse = resolved_smoothers(opt)
    for where, t in (("down", down), ("up", up), ("coarse", coarse)):
        if t in (7, 18, 11, 12) or (where == "coarse" and t in (9, 19, 98, 99)):
            continue
        kind = {0: "Jacobi 0", 16: "Chebyshev 16"}.get(t, "hybrid Gauss-Seidel %d" % t if t in (3, 4, 6, 8, 13, 14, 88, 89) else "%d" % t)
        return "smoother %s (%s) doesn't support multicomponent vectors (served: 7, 18, 11, 12; direct coarse solve)" % (kind, where)
    if opt.relax_order != 0:
        return "C/F-ordered relaxation (-CF %d) doesn't support multicomponent vectors" % opt.relax_order
    if opt.mixed:
        return "mixed precision doesn't support multicomponent vectors"
    return ""


def _vector(A, values, comm, nv=1, memory_location=DEVICE):
    """This rank's `values` as a ParVector laid out like the rows of A; nv > 1: a multivector with the values in each of nv columns."""
    Am = A.contents
    where = dict(comm=comm, global_size=int(Am.global_num_rows), first=int(Am.row_starts[0]), location=memory_location)
    if nv > 1:
        return B.parmultivec_from_numpy(np.repeat(values[:, None], nv, axis=1), **where)
    return B.parvec_from_numpy(values, **where)


def device_vectors(opt, A, comm, rank, allreduce, memory_location=DEVICE):
    """(b, x0) of build_rhs_host as ParVectors in `memory_location`; -nc N: as multivectors, the same values in every column
    (test/ij.c:3483-3512).  -xisone: b = A * ones, a product on the device with the migrated A, read back and laid out like any other b."""
    L = B.load_library()
    b, x0 = build_rhs_host(opt, A, rank=rank, allreduce=allreduce)
    if b is None:
        if memory_location != DEVICE:
            raise SystemExit("ij: -xisone needs a product with A, which runs on the device only")
        ones, prod = _vector(A, np.ones(len(x0)), comm), _vector(A, np.zeros(len(x0)), comm)
        L.hypre_ParCSRMatrixMatvec(1.0, A, ones, 0.0, prod)
        b = B.parvec_to_numpy(prod)
        L.hypre_ParVectorDestroy(ones); L.hypre_ParVectorDestroy(prod)
    return tuple(_vector(A, v, comm, opt.num_components, memory_location) for v in (b, x0))


def closing_lines(opt, its, rel):
    """The driver's closing lines for every solver but the hybrid one.  The Krylov solvers are named in both lines, BoomerAMG
    and ILU alone in the first only."""
    spec = SOLVERS[opt.solver]
    tag = "LGMRES " if opt.lgmres else spec.tag
    return ["", "%sIterations = %d" % (tag, its),
            "Final %sRelative Residual Norm = %e" % ("" if spec.method in (None, "ILU") else tag, rel), ""]


def run(opt, comm=0, rank=0, nprocs=1, allreduce=None, out=None):
    """test/ij.c: build the problem, set up, solve on the device, print the driver's closing lines."""
    import sys
    out = out or sys.stdout
    L = B.load_library()
    if nprocs > 1 and opt.smooth_num_levels > 0:
        raise SystemExit("ij: ILU smoothing (smooth_type 5 | 15) on more than one rank is outside the scope of this driver")
    A = build_matrix(opt, comm=comm, rank=rank, nprocs=nprocs)
    if opt.hybrid:
        return run_hybrid(opt, A, comm=comm, rank=rank, allreduce=allreduce, out=out)
    spec = SOLVERS[opt.solver]
    if spec.precond == "ilu":
        return run_ilu(opt, A, comm=comm, rank=rank, allreduce=allreduce, out=out)
    amg = None
    if spec.precond == "amg":
        amg = create_amg(opt, memory_location=DEVICE)
        L.HYPRE_BoomerAMGSetup(amg, A, None, None)      # on the host matrix
        B.check()
    L.hypre_ParCSRMatrixMigrate(A, DEVICE)
    db, dx = device_vectors(opt, A, comm, rank, allreduce)
    if spec.method is None:
        its, rel, lines = solve_amg(opt, amg, A, db, dx, comm=comm)
    else:
        its, rel = krylov_solver(opt)(opt, A=A, b=db, x=dx, comm=comm, amg=amg)
        lines = []
    lines += closing_lines(opt, its, rel)
    L.HYPRE_ClearError(256)          # HYPRE_ERROR_CONV is reported through the iteration count, as the driver does
    B.check()
    if amg is not None:
        L.HYPRE_BoomerAMGDestroy(amg)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    if rank == 0:
        out.write("\n".join(lines) + "\n")
        out.flush()
    return its, rel


def solve_amg(opt, amg, A, db, dx, comm=0):
    """BoomerAMG alone (solver 0, test/ij.c:4440-4780): (iterations, final relative residual norm, the lines on the average
    convergence factor and the complexities that precede the closing lines)."""
    L = B.load_library()
    # ||b - A x0|| for the average convergence factor (par_amg_solve.c:237-256, 347-355)
    r0 = _vector(A, np.zeros(A.contents.diag.contents.num_rows), comm, opt.num_components)
    L.hypre_ParCSRMatrixMatvecOutOfPlace(-1.0, A, dx, 1.0, db, r0)
    L.hypre_ParVectorInnerProd.restype = C.c_double
    nrm0 = float(np.sqrt(L.hypre_ParVectorInnerProd(r0, r0)))
    nrmb = float(np.sqrt(L.hypre_ParVectorInnerProd(db, db)))
    L.hypre_ParVectorDestroy(r0)
    L.HYPRE_BoomerAMGSolve(amg, A, db, dx)
    its, rel = C.c_int(), C.c_double()
    L.HYPRE_BoomerAMGGetNumIterations(amg, C.byref(its))
    L.HYPRE_BoomerAMGGetFinalRelativeResidualNorm(amg, C.byref(rel))
    g, o, cyc = C.c_double(), C.c_double(), C.c_double()
    L.hypre_amd_BoomerAMGGetComplexities(amg, C.byref(g), C.byref(o))
    L.hypre_amd_BoomerAMGGetCycleOpCount(amg, C.byref(cyc))
    resid = rel.value * (nrmb if nrmb != 0.0 else 1.0)
    conv = (resid / nrm0) ** (1.0 / its.value) if its.value > 0 and nrm0 != 0.0 else 1.0
    nnz0 = float(A.contents.d_num_nonzeros)
    return its.value, rel.value, ["", " Average Convergence Factor = %f" % conv, "",
                                  "     Complexity:    grid = %f" % g.value,
                                  "                operator = %f" % o.value,
                                  "                   cycle = %f" % (cyc.value / nnz0 if nnz0 else 0.0), "", ""]


def krylov_solver(opt):
    """The solve_* wrapper of the options' Krylov method, to be called with A, b, x, comm and the preconditioner (amg or ilu) by
    keyword: solve_gmres takes amg in second place."""
    return globals()["solve_" + ("lgmres" if opt.lgmres else SOLVERS[opt.solver].method.lower())]


def _solve_krylov(name, setters, opt, A, b, x, comm, amg, amg_first=False, amg_max_iter=None, check_precond=False, ilu=None):
    """Create, set, Setup, Solve, read back and Destroy one HYPRE_ParCSR<name> solver (PCG, BiCGSTAB, GMRES, COGMRES, FlexGMRES,
    LGMRES), in the order of library calls the reference driver makes: the `setters`, (stem, value) pairs in order; then
    BoomerAMG (`amg`, tuned as a preconditioner: SetTol 0, SetMaxIter precon_cycles; before Create if
    `amg_first`, MaxIter set once more to `amg_max_iter` if given), the ILU object `ilu` (HYPRE_ILUSolve / HYPRE_ILUSetup) or the
    diagonal scaling preconditioner."""
    L = B.load_library()
    fn = lambda stem: getattr(L, "HYPRE_%s%s" % (name, stem))
    par = lambda stem: getattr(L, "HYPRE_ParCSR%s%s" % (name, stem))

    def tune_amg():
        L.HYPRE_BoomerAMGSetTol(amg, 0.0)
        L.HYPRE_BoomerAMGSetMaxIter(amg, opt.precon_cycles)
    if amg is not None and amg_first:
        tune_amg()
    g = C.c_void_p()
    par("Create")(comm, C.byref(g))
    for stem, value in setters:
        fn("Set" + stem)(g, value)
    if amg is not None:
        if not amg_first:
            tune_amg()
        if amg_max_iter is not None:
            fn("SetMaxIter")(g, amg_max_iter)
        fn("SetPrecond")(g, C.cast(L.HYPRE_BoomerAMGSolve, C.c_void_p), None, amg)
    elif ilu is not None:
        fn("SetPrecond")(g, C.cast(L.HYPRE_ILUSolve, C.c_void_p), C.cast(L.HYPRE_ILUSetup, C.c_void_p), ilu)
    else:
        fn("SetPrecond")(g, C.cast(L.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(L.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None)
    if check_precond:
        gotten = C.c_void_p()
        fn("GetPrecond")(g, C.byref(gotten))
        if gotten.value != (amg.value if amg is not None else ilu.value if ilu is not None else None):
            raise SystemExit("HYPRE_%sGetPrecond got bad precond" % name)
    par("Setup")(g, A, b, x)
    par("Solve")(g, A, b, x)
    its, rel = C.c_int(), C.c_double()
    fn("GetNumIterations")(g, C.byref(its))
    fn("GetFinalRelativeResidualNorm")(g, C.byref(rel))
    par("Destroy")(g)
    return its.value, rel.value


def solve_pcg(opt, A, b, x, comm=0, amg=None):
    """test/ij.c:5007-5027, 5179-5200: PCG behind BoomerAMG (solver 1, `amg` the set-up hierarchy) or behind the diagonal scaling
    preconditioner (solver 2); b and x may be multivectors (-nc N)."""
    return _solve_krylov("PCG", (("Tol", opt.tol), ("MaxIter", opt.max_iter), ("TwoNorm", opt.two_norm), ("Flex", opt.flex)),
                         opt, A, b, x, comm, amg, amg_first=True)


def solve_ds_pcg(opt, A, db, dx, comm=0):
    """PCG with the diagonal scaling preconditioner (solver 2)."""
    return solve_pcg(opt, A, db, dx, comm=comm)


def _gmres_setters(opt, early=(), late=()):
    """What the reference driver sets on GMRES and its variants, in its order; `early` and `late` are the variant's own."""
    return (("KDim", opt.k_dim),) + early + (("MaxIter", opt.max_iter), ("Tol", opt.tol), ("AbsoluteTol", 0.0)) + late


def solve_gmres(opt, amg, A, b, x, comm=0, ilu=None):
    """test/ij.c:6710-6790, 6919-6942, 7156-7215: GMRES(k) behind BoomerAMG (solver 3), ILU (81) or, with neither, the diagonal
    scaling preconditioner (4); b and x may be multivectors (-nc N)."""
    return _solve_krylov("GMRES", _gmres_setters(opt), opt, A, b, x, comm, amg, amg_first=True, ilu=ilu)


def solve_ds_gmres(opt, A, db, dx, comm=0):
    """GMRES(k) with the diagonal scaling preconditioner (solver 4)."""
    return solve_gmres(opt, None, A, db, dx, comm=comm)


def solve_cogmres(opt, A, b, x, comm=0, amg=None):
    """test/ij.c:8426-8440, 8583-8598, 8710-8722: COGMRES behind BoomerAMG (solver 16, `amg` the set-up hierarchy) or behind the
    diagonal scaling preconditioner (solver 17)."""
    return _solve_krylov("COGMRES", _gmres_setters(opt, early=(("Unroll", opt.unroll), ("CGS", opt.cgs)),
                                                   late=(("Logging", 3), ("PrintLevel", 3))),     # ioutdat (test/ij.c:686); inert here
                         opt, A, b, x, comm, amg, amg_max_iter=opt.mg_max_iter)


def solve_flexgmres(opt, A, b, x, comm=0, amg=None, ilu=None):
    """test/ij.c:7565-7578, 7720-7724, 7855-7943: FlexGMRES behind BoomerAMG (solver 61, `amg` the set-up hierarchy), ILU (82) or
    the diagonal scaling preconditioner (solver 60); b and x may be multivectors (-nc N).  modify_pc stays the default, which
    changes nothing."""
    return _solve_krylov("FlexGMRES", _gmres_setters(opt, late=(("Logging", 1), ("PrintLevel", 3))),   # ioutdat; inert here
                         opt, A, b, x, comm, amg, amg_max_iter=opt.mg_max_iter, check_precond=True, ilu=ilu)


def solve_lgmres(opt, A, b, x, comm=0, amg=None):
    """test/ij.c:7338-7560: LGMRES behind BoomerAMG (the reference's solver 51, `amg` the set-up hierarchy) or behind the diagonal
    scaling preconditioner (50); b and x may be multivectors (-nc N).  AugDim follows KDim, which it is clamped against."""
    return _solve_krylov("LGMRES", _gmres_setters(opt, early=(("AugDim", opt.aug_dim),),
                                                  late=(("Logging", 1), ("PrintLevel", 3))),      # ioutdat; inert here
                         opt, A, b, x, comm, amg, amg_max_iter=opt.mg_max_iter, check_precond=True)


def solve_bicgstab(opt, A, b, x, comm=0, amg=None):
    """test/ij.c:8002-8172, 8324-8367: BiCGSTAB behind BoomerAMG (solver 9, `amg` the set-up hierarchy, run as a preconditioner:
    SetTol 0, SetMaxIter precon_cycles; the iteration limit is then mg_max_iter, test/ij.c:8156) or behind the diagonal
    scaling preconditioner (solver 10); b and x may be multivectors (-nc N).  The reference driver also asks for the
    solver's table of norms (ioutdat); this one prints the closing lines alone, as for its other solvers."""
    return _solve_krylov("BiCGSTAB", (("MaxIter", opt.max_iter), ("Tol", opt.tol), ("AbsoluteTol", 0.0), ("Logging", 1), ("PrintLevel", 0)),
                         opt, A, b, x, comm, amg, amg_max_iter=opt.mg_max_iter)


def create_ilu(opt, preconditioner=False):
    """test/ij.c:9210-9233 (solver 80) and :7162-7186, 7861-7883 (the preconditioner of 81 / 82: one application, tolerance 0)
    as far as block-Jacobi ILU(k) has parameters.  The reference driver asks solver 80 for print level 2, the solver's own
    table; this one prints the closing lines alone, as for its other solvers."""
    L = B.load_library()
    s = C.c_void_p()
    L.HYPRE_ILUCreate(C.byref(s))
    L.HYPRE_ILUSetType(s, opt.ilu_type)
    L.HYPRE_ILUSetLevelOfFill(s, opt.ilu_lfil)
    L.HYPRE_ILUSetLocalReordering(s, opt.ilu_reordering)
    L.HYPRE_ILUSetTriSolve(s, opt.ilu_tri_solve)
    # the reference driver hands the sweep counts to 81 / 82 only (test/ij.c:7167-7168, 7866-7867); here 80 takes them too
    L.hypre_amd_ILUSetIterativeTriSolve(s, opt.ilu_iterative)
    L.HYPRE_ILUSetLowerJacobiIters(s, opt.ilu_ljac_iters)
    L.HYPRE_ILUSetUpperJacobiIters(s, opt.ilu_ujac_iters)
    L.HYPRE_ILUSetPrintLevel(s, 0)
    L.HYPRE_ILUSetMaxIter(s, 1 if preconditioner else opt.max_iter)
    L.HYPRE_ILUSetTol(s, 0.0 if preconditioner else opt.tol)
    B.check()
    return s


def run_ilu(opt, A, comm=0, rank=0, allreduce=None, out=None, memory_location=DEVICE):
    """`ij -solver 80 | 81 | 82`: ILU alone (test/ij.c:9204-9286), ILU-GMRES (:6710-6727, 7156-7195) and ILU-FlexGMRES
    (:7565-7578, 7855-7890).  memory_location HOST runs solver 80 on the library's host path (the Krylov solvers have none)."""
    import sys
    out = out or sys.stdout
    L = B.load_library()
    alone = SOLVERS[opt.solver].method == "ILU"
    if memory_location == DEVICE:
        L.hypre_ParCSRMatrixMigrate(A, DEVICE)
    elif not alone:
        raise SystemExit("ij: -solver %d in host memory: the Krylov solvers run on the device only" % opt.solver)
    db, dx = device_vectors(opt, A, comm, rank, allreduce, memory_location)
    ilu = create_ilu(opt, preconditioner=not alone)
    if alone:
        L.HYPRE_ILUSetup(ilu, A, db, dx)
        L.HYPRE_ILUSolve(ilu, A, db, dx)
        its, rel = C.c_int(), C.c_double()
        L.HYPRE_ILUGetNumIterations(ilu, C.byref(its))
        L.HYPRE_ILUGetFinalRelativeResidualNorm(ilu, C.byref(rel))
        its, rel = its.value, rel.value
    else:
        its, rel = krylov_solver(opt)(opt, A=A, b=db, x=dx, comm=comm, amg=None, ilu=ilu)
    L.HYPRE_ClearError(256)
    B.check()
    L.HYPRE_ILUDestroy(ilu)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    if rank == 0:
        out.write("\n".join(closing_lines(opt, its, rel)) + "\n")
        out.flush()
    return its, rel


def create_hybrid(opt):
    """test/ij.c:4308-4360: the setter sequence of solver 20, everything the reference driver hands over.  Logging is the
    driver's ioutdat (3); of its poutdat (1) the Krylov solver's digit is dropped, so that BiCGSTAB prints no table of
    norms: this driver prints the closing lines alone, as for its other solvers."""
    L = B.load_library()
    h = C.c_void_p()
    L.HYPRE_ParCSRHybridCreate(C.byref(h))
    L.HYPRE_ParCSRHybridSetTol(h, opt.tol)
    L.HYPRE_ParCSRHybridSetAbsoluteTol(h, 0.0)
    L.HYPRE_ParCSRHybridSetConvergenceTol(h, opt.cf_tol)
    L.HYPRE_ParCSRHybridSetSolverType(h, opt.hybrid_solver_type)
    L.HYPRE_ParCSRHybridSetRecomputeResidual(h, 0)
    L.HYPRE_ParCSRHybridSetLogging(h, 3)
    L.HYPRE_ParCSRHybridSetPrintLevel(h, 0)
    L.HYPRE_ParCSRHybridSetDSCGMaxIter(h, opt.max_iter)
    L.HYPRE_ParCSRHybridSetPCGMaxIter(h, opt.mg_max_iter)
    L.HYPRE_ParCSRHybridSetCoarsenType(h, opt.coarsen_type)
    L.HYPRE_ParCSRHybridSetStrongThreshold(h, opt.strong_threshold)
    L.HYPRE_ParCSRHybridSetTruncFactor(h, opt.trunc_factor)
    L.HYPRE_ParCSRHybridSetPMaxElmts(h, opt.P_max_elmts)
    L.HYPRE_ParCSRHybridSetMaxLevels(h, opt.max_levels)
    L.HYPRE_ParCSRHybridSetMaxRowSum(h, opt.max_row_sum)
    L.HYPRE_ParCSRHybridSetNumSweeps(h, opt.num_sweeps)
    L.HYPRE_ParCSRHybridSetInterpType(h, opt.interp_type)
    if opt.relax_type > -1:
        L.HYPRE_ParCSRHybridSetRelaxType(h, opt.relax_type)
    L.HYPRE_ParCSRHybridSetAggNumLevels(h, 0)
    L.HYPRE_ParCSRHybridSetAggInterpType(h, 4)
    L.HYPRE_ParCSRHybridSetNumPaths(h, 1)
    L.HYPRE_ParCSRHybridSetNumFunctions(h, opt.num_functions)
    L.HYPRE_ParCSRHybridSetNodal(h, 0)
    for k, t in ((1, opt.relax_down), (2, opt.relax_up), (3, opt.relax_coarse)):
        if t > -1:
            L.HYPRE_ParCSRHybridSetCycleRelaxType(h, t, k)
    L.HYPRE_ParCSRHybridSetRelaxOrder(h, opt.relax_order)
    L.HYPRE_ParCSRHybridSetKeepTranspose(h, opt.keep_transpose)
    L.HYPRE_ParCSRHybridSetMaxCoarseSize(h, opt.coarse_threshold)
    L.HYPRE_ParCSRHybridSetMinCoarseSize(h, 0)
    L.HYPRE_ParCSRHybridSetSeqThreshold(h, 0)
    L.HYPRE_ParCSRHybridSetRelaxWt(h, opt.relax_wt)
    L.HYPRE_ParCSRHybridSetOuterWt(h, opt.outer_wt)
    if opt.level_w is not None:
        L.HYPRE_ParCSRHybridSetLevelRelaxWt(h, opt.level_w[0], opt.level_w[1])
    if opt.level_ow is not None:
        L.HYPRE_ParCSRHybridSetLevelOuterWt(h, opt.level_ow[0], opt.level_ow[1])
    L.HYPRE_ParCSRHybridSetNonGalerkinTol(h, 0, None)
    B.check()
    return h


def run_hybrid(opt, A, comm=0, rank=0, allreduce=None, out=None):
    """hybrid = 1 (the reference's `ij -solver 20 [-cf v] [-solver_type t]`) on the device; the closing lines of
    test/ij.c:4419-4432.  Returns (iterations, AMG iterations, diagonally scaled iterations, final relative residual norm)."""
    L = B.load_library()
    L.hypre_ParCSRMatrixMigrate(A, DEVICE)
    db, dx = device_vectors(opt, A, comm, rank, allreduce)
    h = create_hybrid(opt)
    L.HYPRE_ParCSRHybridSetup(h, A, db, dx)
    L.HYPRE_ParCSRHybridSolve(h, A, db, dx)
    L.HYPRE_ClearError(256)
    B.check()
    its, pcg_its, dscg_its, rel = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    L.HYPRE_ParCSRHybridGetNumIterations(h, C.byref(its))
    L.HYPRE_ParCSRHybridGetPCGNumIterations(h, C.byref(pcg_its))
    L.HYPRE_ParCSRHybridGetDSCGNumIterations(h, C.byref(dscg_its))
    L.HYPRE_ParCSRHybridGetFinalRelativeResidualNorm(h, C.byref(rel))
    L.HYPRE_ParCSRHybridDestroy(h)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    if rank == 0:
        out.write("\n".join(["", "Iterations = %d" % its.value, "PCG_Iterations = %d" % pcg_its.value,
                             "DSCG_Iterations = %d" % dscg_its.value, "Final Relative Residual Norm = %e" % rel.value, ""]) + "\n")
        out.flush()
    return its.value, pcg_its.value, dscg_its.value, rel.value


def main(argv=None):
    """`python -m hypre_amd.ij <reference ij flags>`; under torch.distributed.run one rank per process
    (ranks may share a GPU: the halo then travels over gloo, staged through the host)."""
    import sys
    argv = sys.argv[1:] if argv is None else argv
    return launch(parse_cli(argv))


def launch(opt):
    """run(opt) in this process, or as one rank of the torch.distributed.run job this process belongs to"""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        run(opt)
        return 0
    import torch
    import torch.distributed as dist
    from . import distributed
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()

    def allsum(v):
        t = torch.tensor([v], dtype=torch.float64)
        dist.all_reduce(t)
        return float(t.item())

    comm = distributed.create_callback_comm(dist, rank, world)
    run(opt, comm=comm, rank=rank, nprocs=world, allreduce=allsum)
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
