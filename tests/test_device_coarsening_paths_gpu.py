"""Strength of connection, PMIS (setup_kernels.hip) and the extended+i interpolation with truncation (interp_kernels.hip:
extpi_rows_kernel, device_extpi) on unstructured rows, on every path the interpolation kernel can take.

Operands are seeded scipy CSR matrices, diagonal first, off-diagonals in random stored order, handed over as a one-rank
ParCSR.  HYPRE_BoomerAMGSetup (max_levels 2, PMIS, extended+i, every level sent to the device) runs once with the three
device switches off and once with them on.  Every case checks
  * device == host, array for array: C/F marker, P (row pointers, column order, value bits), the stored transpose of P,
    the coarse operator, the smoother diagonals;
  * device == a reference written here from the formulas alone (numpy): the strength pattern through its consequences
    (operands with dyadic values, rows exactly on both thresholds), the PMIS rules on the device's marker, the ext+i weights
    on the device's marker in np.longdouble;
  * the path: hypre_amd_GetDeviceInterpPath and the device counters.

The bound on the weights.  w_ij = -N_j / D with N_j = a_ij + sum_k a_ik a^-_kj / sigma_k over the strong F neighbours k,
sigma_k = sum of the entries of row k that have the sign opposite to a_kk and lie in the set or at i, and D = a~_ii.  The
kernel forms sigma_k by at most len(A_k) additions of same-signed numbers (no cancellation), divides once, multiplies
once and adds the product into N_j, which takes at most len(A_i) additions: every term of N_j carries at most
T_i = max_k len(A_k) + len(A_i) + 3 roundings of eps / 2, so |dN_j| <= T_i eps/2 Nabs_j where Nabs_j is N_j with absolute
values throughout; likewise |dD| <= T_i eps/2 Dabs.  With kappa_i = Dabs / |D| and the final division,
|dw_ij| <= (1 + kappa_i) / 2 * T_i * eps * Nabs_j / |D| (the eps/2 |w| of the division is inside: T_i counted it).  The
reference's own error (longdouble) is a thousandth of that.  C_BOUND = (1 + kappa) / 2 per row; the random operands keep
|a_ii| at twice the absolute off-diagonal sum, so |D| >= |a_ii| / 2, Dabs <= 3 |a_ii| / 2 and kappa <= 3 (asserted).  A row
with D == 0 is left unscaled: the bound is T_i eps/2 Nabs_j, and D == 0 arises only where all sums are exact (dyadic).

Two cases of the issue cannot be reached through the setup: PMIS (par_amg_setup.cpp, hypre_BoomerAMGCoarsenPMIS, "if
(measure[i] < 1) mine = F_PT") makes a point F only if it depends on a C point or influences nobody, so a strong F
neighbour k of i (which i depends on) always has a strong coupling — of the sign opposite to a_kk — to a C point, and
that point is in the set of i: sigma_k == 0 and "the only such coupling is to i" do not occur.  Nor does "all points C",
directed S included: take the sweep in which the first C point j appears.  Its measure exceeds 1, so some k has j in its
row of S.  Either k was made F at once (measure below 1), or k is a candidate of that sweep too, and the knock-out pass
of row k compares it with j ("if (measure[i] > measure[j]) CF[j] = 0; else if (measure[j] > measure[i]) CF[i] = 0": the
measures differ by their random parts, and j stays, so k goes), after which "if (CF[Sdj[jS]] > 0) mine = F_PT" makes k
an F point: a marker with a C point has an F point.  test_pmis_graphs[cycle] shows what a directed cycle gives.

The pattern of S is pinned twice: the host's S (hypre_BoomerAMGCreateS, exported) equals ref_strength() entry for entry,
and the device's S, which stays inside the setup, shows in arrays that are compared with the host's bit for bit — the
threshold rows are built so that one coupling more or less changes the marker or a row of P (test_strength_thresholds).

Rows with a zero diagonal and empty rows run with relax 7 only: hypre_ParCSRComputeL1Norms raises the error flag
for a zero smoother diagonal under options 1 and 4 ("if (std::fabs(l1[i]) == 0.0) hypre_error_in_arg(1)"), option 5
stores 1 instead.  No empty row is the last one: the host strength loop reads "Ada[Adi[i]]" before it looks at the row's
length, as the reference does, which for an empty last row lies behind the array.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from util import parcsr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
ROOM = (64, 128, 256, 1024)
NONE, THRESHOLD_ONLY, TABLES_EXHAUSTED = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
class Rows:
    """Rows of A under construction.  A strong coupling is -1 (dyadic) or in [-1, -1/2] (real); a weak one is given.  The
    diagonal, unless given, is twice the absolute off-diagonal sum; a row flagged negative is multiplied by -1 at the end,
    so its strong couplings are the positive ones.  With theta = 1/4 and max_row_sum = 1 the strong couplings are S."""

    def __init__(self, seed, real=False):
        self.rng = np.random.default_rng(seed)
        self.real = real
        self.rows, self.diag, self.neg = [], [], []

    def new(self, diag=None, neg=False):
        self.rows.append([]); self.diag.append(diag); self.neg.append(neg)
        return len(self.rows) - 1

    def add(self, i, j, v):
        assert i != j and all(c != j for c, _ in self.rows[i])
        self.rows[i].append((j, float(v)))

    def strong(self, i, j):
        self.add(i, j, -self.rng.uniform(0.5, 1.0) if self.real else -1.0)

    def cpoint(self):
        """a point PMIS makes C: it and a partner depend on each other, and whoever else depends on it makes its measure
        the larger of the two"""
        c, z = self.new(), self.new()
        self.strong(c, z); self.strong(z, c)
        return c

    def matrix(self):
        n = len(self.rows)
        ptr, col, val = [0], [], []
        for i, r in enumerate(self.rows):
            order = self.rng.permutation(len(r))
            s = sum(abs(v) for _, v in r)
            d = self.diag[i] if self.diag[i] is not None else (2.0 * s if s else 1.0)
            sign = -1.0 if self.neg[i] else 1.0
            col += [i] + [r[k][0] for k in order]
            val += [sign * d] + [sign * r[k][1] for k in order]
            ptr.append(len(col))
        return sp.csr_matrix((np.array(val), np.array(col, dtype=np.int32), np.array(ptr, dtype=np.int32)), shape=(n, n))


def random_operand(n, seed, real, neg_frac=0.2, edges=False):
    """n rows of 0 - 9 couplings to random points nearby: strong ones, weak ones of both signs, positive strong-sized ones
    (weak for a positive diagonal), rows with a negative diagonal, rows without strong couplings (marker -3), isolated
    points.  edges: four rows more, which nobody depends on (F points or -3), coupled to five C points of their own:
    one with |row sum| == 0.8 |a_ii| exactly, one just above, one with couplings equal to 0.25 and 0.9 times the largest,
    and that row again with a negative diagonal and positive couplings."""
    R = Rows(seed, real)
    rng = R.rng
    n -= 9 + (14 if edges else 0)                   # the last rows are added at the end
    for i in range(n):
        R.new(neg=rng.random() < neg_frac)
    for i in range(n):
        kind = rng.random()
        k = 0 if kind < 0.05 else int(rng.integers(1, 10))
        cand = np.setdiff1d(np.arange(max(0, i - 12), min(n, i + 13)), [i])
        for j in rng.choice(cand, min(k, cand.size), replace=False):
            t = rng.random()
            if kind < 0.12:                         # a row of weak couplings only
                R.add(i, j, rng.choice([-0.125, 0.125, 0.0625]) if not real else rng.uniform(-0.1, 0.1))
            elif t < 0.6:
                R.strong(i, j)
            elif t < 0.8:
                R.add(i, j, rng.choice([-0.125, -0.0625, 0.125]) if not real else rng.uniform(-0.1, 0.1))
            else:
                R.add(i, j, rng.choice([0.5, 1.0]) if not real else rng.uniform(0.3, 1.0))
        if kind >= 0.12 and k and not any(v <= -0.5 for _, v in R.rows[i]):
            R.rows[i][0] = (R.rows[i][0][0], -1.0)  # the scale of the row: strong by itself
    for _ in range(3):                              # F rows that depend on isolated points only: empty rows of P
        f = R.new()
        R.strong(f, R.new()); R.strong(f, R.new())
    if edges:
        c = [R.cpoint() for _ in range(5)]
        e0, e1, e2 = R.new(diag=10.0), R.new(diag=10.0), R.new(diag=8.0)
        R.add(e0, c[0], -1.0); R.add(e0, c[1], -1.0)        # 10 - 2 == 0.8 * 10: the row keeps its couplings (>)
        R.add(e1, c[0], -1.0); R.add(e1, c[1], -0.875)      # 10 - 1.875 > 8: it loses them when max_row_sum = 0.8
        R.add(e2, c[2], -1.0); R.add(e2, c[3], -0.25); R.add(e2, c[4], -0.9)     # == theta * min: weak (<)
        e3 = R.new(diag=8.0, neg=True)                      # the same on the other branch: == theta * max, weak (>)
        R.add(e3, c[2], -1.0); R.add(e3, c[3], -0.25); R.add(e3, c[4], -0.9)
    return R.matrix()


def long_row_operand(seed, real, direct=0, groups=(), a_extra=0, shared=0, common=False, pad_strong_f=0):
    """Point 0 is an F point nobody depends on.  It depends on `direct` C points and, for every entry g of groups, on an F
    point whose row of S holds g C points, the first `shared` of them the direct ones again (found present in the map),
    the others new (common: every group takes the first g points of one pool of C points instead); that F point's row of A has a_extra weak couplings more (to C points of other groups), one weak
    coupling back to point 0 and alternating in sign.  pad_strong_f more F neighbours share one C point.  The set of point
    0 has direct + sum(groups) - (shared per group) [+ 1 for the padding] points."""
    R = Rows(seed, real)
    i0 = R.new()
    dc = [R.cpoint() for _ in range(direct)]
    for c in dc:
        R.strong(i0, c)
    pool = list(dc)
    fs = []
    cpool = [R.cpoint() for _ in range(max(groups, default=0))] if common else []
    for g in groups:
        f = R.new()
        R.strong(i0, f)
        own = cpool[:g] if common else dc[:min(shared, g)] + [R.cpoint() for _ in range(g - min(shared, g))]
        for c in own:
            R.strong(f, c)
        R.add(f, i0, -0.125 if not real else -R.rng.uniform(0.01, 0.1))
        fs.append((f, own))
        pool += own
    for q, (f, own) in enumerate(fs):
        others = [c for c in dict.fromkeys(pool) if c not in own][:a_extra]
        for t, c in enumerate(others):
            R.add(f, c, (0.125 if t % 2 else -0.125) if not real else R.rng.uniform(-0.1, 0.1))
    if pad_strong_f:
        c = R.cpoint()
        for _ in range(pad_strong_f):
            f = R.new()
            R.strong(i0, f); R.strong(f, c)
    return R.matrix()


# ---------------------------------------------------------------------------------------------------------------------
# the library's side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def amg(gpu_lib):
    """the library, with every global switch of the setup restored afterwards"""
    from hypre_amd import binding as B
    L = gpu_lib
    try:
        yield L, B
    finally:
        L.hypre_amd_SetSetupDeviceRAP(1, 20000)
        L.hypre_amd_SetSetupDeviceInterp(1)
        L.hypre_amd_SetSetupDeviceCoarsen(1)
        L.hypre_amd_SetDeviceInterpWaves(0)
        L.HYPRE_ClearAllErrors()


def setup(L, B, A, on, theta=0.25, max_row_sum=1.0, pmx=0, trunc=0.0, relax=18, rung=0, waves=0):
    """two-level setup of A; returns the hierarchy's arrays, the device counters and the interpolation kernel's report"""
    from hypre_amd import ij
    L.hypre_amd_SetSetupDeviceRAP(on, 1)
    L.hypre_amd_SetSetupDeviceInterp(on * (1 + rung))
    L.hypre_amd_SetSetupDeviceCoarsen(on)
    L.hypre_amd_SetDeviceInterpWaves(waves)
    opt = ij.IJOptions(coarsen_type=8, interp_type=6, max_levels=2, strong_threshold=theta, max_row_sum=max_row_sum,
                       P_max_elmts=pmx, trunc_factor=trunc, relax_type=relax)
    Ap = parcsr(L, B, A, B.HYPRE_MEMORY_HOST)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    try:
        L.HYPRE_BoomerAMGSetup(s, Ap, None, None)
        B.check()                                   # the error flag is clear, whoever built the level
        out = dict(levels=L.hypre_amd_BoomerAMGGetNumLevels(s))
        out["coarsened"] = L.hypre_amd_SetSetupDeviceCoarsen(-1)
        out["interpolated"] = L.hypre_amd_SetSetupDeviceInterp(-1)
        rep = (C.c_int * 5)(-9, -9, -9, -9, -9)
        L.hypre_amd_GetDeviceInterpPath(rep)
        out["path"] = dict(zip(("first", "rung", "attempts", "count_then_write", "declined"), list(rep)))
        cf = C.cast(L.hypre_amd_BoomerAMGGetCFMarker(s, 0), C.POINTER(B.IntArray)).contents
        out["cf"] = B.fetch(cf.data, cf.size, np.int32, cf.memory_location)
        arrays = [(out["cf"],)]
        if out["levels"] == 2:
            Pl = C.cast(L.hypre_amd_BoomerAMGGetP(s, 0), C.POINTER(B.ParCSRMatrix))
            out["P"] = B.csr_to_arrays(Pl.contents.diag)
            arrays += [out["P"], B.csr_to_arrays(Pl.contents.diagT)]
            A1 = C.cast(L.hypre_amd_BoomerAMGGetA(s, 1), C.POINTER(B.ParCSRMatrix))
            arrays.append(B.csr_to_arrays(A1.contents.diag))
        for l in range(out["levels"]):
            l1p = L.hypre_amd_BoomerAMGGetL1Norms(s, l)
            if l1p:
                arrays.append((B.vec_to_numpy(C.cast(l1p, C.POINTER(B.Vector))),))
        out["arrays"] = arrays
    finally:
        L.HYPRE_BoomerAMGDestroy(s)
        L.hypre_ParCSRMatrixDestroy(Ap)
    return out


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def host_strength(L, B, A, theta, max_row_sum):
    """rows of the host routine's S"""
    Ap = parcsr(L, B, A, B.HYPRE_MEMORY_HOST)
    Sp = C.c_void_p()
    try:
        L.hypre_BoomerAMGCreateS(Ap, theta, max_row_sum, 1, None, C.byref(Sp))
        B.check()
        S = C.cast(Sp, C.POINTER(B.ParCSRMatrix))
        ii, jj, _ = B.csr_to_arrays(S.contents.diag)
        L.hypre_ParCSRMatrixDestroy(S)
    finally:
        L.hypre_ParCSRMatrixDestroy(Ap)
    return [jj[ii[i]:ii[i + 1]].astype(np.int64) for i in range(A.shape[0])]


def both(L, B, A, **kw):
    """host setup and device setup of A: the same arrays; returns the device's.  The host's S is the reference's,
    entry for entry in stored order."""
    theta, max_row_sum = kw.get("theta", 0.25), kw.get("max_row_sum", 1.0)
    for i, (r, h) in enumerate(zip(ref_strength(A, theta, max_row_sum), host_strength(L, B, A, theta, max_row_sum))):
        assert np.array_equal(r, h), "row %d of S: reference %s, host %s" % (i, r, h)
    host = setup(L, B, A, 0, **kw)
    assert host["coarsened"] == 0 and host["interpolated"] == 0
    dev = setup(L, B, A, 1, **kw)
    assert dev["coarsened"] == 1, "strength and PMIS did not run on the device"
    assert host["levels"] == dev["levels"] and len(host["arrays"]) == len(dev["arrays"])
    for q, (m0, m1) in enumerate(zip(host["arrays"], dev["arrays"])):
        assert len(m0) == len(m1)
        for a, b in zip(m0, m1):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), "array group %d differs between host and device" % q
    return dev


# ---------------------------------------------------------------------------------------------------------------------
# the reference: formulas only
# ---------------------------------------------------------------------------------------------------------------------
def ref_strength(A, theta, max_row_sum):
    """rows of S: the off-diagonal columns j, in stored order, with a_ij < theta min_k a_ik (a_ii >= 0) or
    a_ij > theta max_k a_ik (a_ii < 0); none if |row sum| > max_row_sum |a_ii| and max_row_sum < 1"""
    S = []
    for i in range(A.shape[0]):
        c, v = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
        if c.size == 0:
            S.append(np.zeros(0, dtype=np.int64)); continue
        assert c[0] == i
        d, off = v[0], v[1:]
        if max_row_sum < 1.0 and abs(float(np.sum(v.astype(LD)))) > abs(d) * max_row_sum:
            S.append(np.zeros(0, dtype=np.int64)); continue
        if d < 0:
            keep = off > theta * max(0.0, off.max(initial=0.0))
        else:
            keep = off < theta * min(0.0, off.min(initial=0.0))
        S.append(c[1:][keep].astype(np.int64))
    return S


def check_pmis(S, cf):
    """markers in {1, -1, -3}; -3 exactly on the empty rows of S; no two C points that depend on each other; an F point
    depends on a C point or influences nobody (hypre_BoomerAMGCoarsenPMIS: "if (measure[i] < 1) mine = F_PT", measure =
    the number of rows of S that hold i plus a random number below 1, and otherwise F only "if (CF[Sdj[jS]] > 0)").
    With an unsymmetric S a C point may depend on another one that does not depend on it: the knock-out pass compares a
    candidate with the candidates in ITS row only, and a point already settled as C is no candidate when the point it
    depends on becomes one in a later sweep.  On a symmetric S the rule is "no two C points joined"."""
    n = len(S)
    assert set(np.unique(cf)) <= {1, -1, -3}
    influences = np.zeros(n, dtype=np.int64)
    for r in S:
        influences[r] += 1
    for i in range(n):
        assert (cf[i] == -3) == (S[i].size == 0), "row %d: marker %d, %d strong couplings" % (i, cf[i], S[i].size)
        if cf[i] == 1:
            for j in S[i][cf[S[i]] == 1]:
                assert i not in S[j], "C points %d and %d depend on each other" % (i, j)
            assert influences[i] >= 1
        elif cf[i] == -1:
            assert np.any(cf[S[i]] == 1) or influences[i] == 0, "F point %d" % i


def ref_extpi(A, S, cf):
    """per row: the set's coarse columns in first-touch order, w (longdouble), the bound of the module docstring, kappa"""
    n = A.shape[0]
    f2c = np.cumsum(cf == 1) - 1
    rows = []
    row = lambda i: (A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]].astype(LD))
    for i in range(n):
        if cf[i] == 1:
            rows.append(([f2c[i]], np.array([1.0], dtype=LD), np.zeros(1), 0.0)); continue
        if cf[i] == -3:
            rows.append(([], np.zeros(0, dtype=LD), np.zeros(0), 0.0)); continue
        pos, strong_f = {}, set()
        for j in S[i]:
            if cf[j] == 1:
                pos.setdefault(int(j), len(pos))
            elif cf[j] == -1:
                strong_f.add(int(j))
                for k in S[j]:
                    if cf[k] == 1:
                        pos.setdefault(int(k), len(pos))
        N, Nabs = np.zeros(len(pos), dtype=LD), np.zeros(len(pos), dtype=LD)
        ci, vi = row(i)
        D, Dabs, T = vi[0], abs(vi[0]), 0
        for j, a in zip(ci[1:], vi[1:]):
            j = int(j)
            if j in pos:
                N[pos[j]] += a; Nabs[pos[j]] += abs(a)
            elif j in strong_f:
                ck, vk = row(j)
                T = max(T, ck.size)
                opp = (vk[1:] * (-1 if vk[0] < 0 else 1)) < 0
                inset = np.array([int(c) in pos or int(c) == i for c in ck[1:]], dtype=bool)
                sigma = np.sum(vk[1:][opp & inset])
                if sigma != 0:
                    for c, v in zip(ck[1:][opp & inset], vk[1:][opp & inset]):
                        if int(c) == i:
                            D += a * v / sigma; Dabs += abs(a * v / sigma)
                        else:
                            N[pos[int(c)]] += a * v / sigma; Nabs[pos[int(c)]] += abs(a * v / sigma)
                else:
                    D += a; Dabs += abs(a)
            elif cf[j] != -3:
                D += a; Dabs += abs(a)
        T += ci.size + 3
        if D != 0:
            kappa = float(Dabs / abs(D))
            w, lim = -N / D, (1.0 + kappa) / 2.0 * T * EPS * (Nabs / abs(D)).astype(np.float64)
        else:
            kappa = 0.0
            w, lim = N, T * EPS / 2.0 * Nabs.astype(np.float64)
        cols = [0] * len(pos)
        for j, p in pos.items():
            cols[p] = f2c[j]
        rows.append((cols, w, lim, kappa))
    return rows


def check_interpolation(A, dev, theta=0.25, max_row_sum=1.0, kappa_max=None):
    """the device's marker against the PMIS rules, its (untruncated) P against the reference on that marker: every row's
    columns as a set, every value within the bound.  Returns the sizes of the interpolatory sets."""
    S = ref_strength(A, theta, max_row_sum)
    cf = dev["cf"]
    check_pmis(S, cf)
    ref = ref_extpi(A, S, cf)
    ii, jj, aa = dev["P"]
    assert ii.shape == (A.shape[0] + 1,) and ii[0] == 0
    sizes = np.zeros(A.shape[0], dtype=np.int64)
    worst = 0.0
    for i, (cols, w, lim, kappa) in enumerate(ref):
        got_c, got_v = jj[ii[i]:ii[i + 1]], aa[ii[i]:ii[i + 1]]
        assert sorted(got_c.tolist()) == sorted(cols), "row %d: columns %s, reference %s" % (i, sorted(got_c.tolist())[:8], sorted(cols)[:8])
        if kappa_max is not None:
            assert kappa <= kappa_max, "row %d: the operand does not keep |a~_ii| away from 0 (kappa %.2f)" % (i, kappa)
        at = {c: k for k, c in enumerate(cols)}
        for c, v in zip(got_c.tolist(), got_v.tolist()):
            err, bound = abs(float(LD(v) - w[at[c]])), lim[at[c]]
            assert err <= bound, "row %d column %d: %r vs %r, error %.3e, bound %.3e" % (i, c, v, float(w[at[c]]), err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
        sizes[i] = len(cols) if cf[i] == -1 else 0
    print("worst error / bound %.3f, largest set %d" % (worst, sizes.max(initial=0)))
    return sizes


# ---------------------------------------------------------------------------------------------------------------------
# values, signs, shapes; one wave per row and four waves over all rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [0, 4])
@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("relax", [18, 7, 8])
def test_unstructured_rows(amg, waves, real, relax):
    """300 irregular rows: mixed-sign off-diagonals, negative diagonals (sgn = -1 for a strong F neighbour), weak
    neighbours of both signs, weak neighbours marked -3, isolated points, F rows that reach no C point.  relax 7, 18 and 8
    send the rows through the smoother diagonals of options 5, 1 and 4 (without ghost columns option 6, of relax 88,
    is the kernel's statement for option 4)."""
    L, B = amg
    A = random_operand(300, seed=11 + real, real=real)
    dev = both(L, B, A, relax=relax, waves=waves)
    assert dev["levels"] == 2 and dev["interpolated"] == 1
    assert dev["path"] == dict(first=0, rung=0, attempts=1, count_then_write=1, declined=NONE), dev["path"]
    sizes = check_interpolation(A, dev, kappa_max=3.0 if real else None)
    cf = dev["cf"]
    S = ref_strength(A, 0.25, 1.0)
    neg = A.data[A.indptr[:-1]] < 0
    f_rows = np.flatnonzero(cf == -1)
    assert np.any(cf == -3) and np.any(neg & (cf == -1)) and np.any(neg & (cf == 1))
    assert any(np.any((cf[S[i]] == -1) & neg[S[i]]) for i in f_rows), "no strong F neighbour with a negative diagonal"
    assert any(np.any(cf[A.indices[A.indptr[i] + 1:A.indptr[i + 1]]] == -3) for i in f_rows), "no weak neighbour marked -3"
    assert np.any(np.diff(dev["P"][0])[f_rows] == 0), "no F row without a C point within two steps"
    assert sizes.max() < 64


@pytest.mark.parametrize("waves", [0, 4])
def test_unscaled_row_and_threshold_ties(amg, waves):
    """dyadic rows on the edges: a~_ii exactly 0 (1 - 4 * 1/4: the row is left unscaled, its weight is a_ic itself);
    couplings equal to theta * min (weak: the comparison is strict, or the four would join the set)"""
    L, B = amg
    R = Rows(5)
    i0 = R.new(diag=1.0)
    c = R.cpoint()
    R.strong(i0, c)
    weak = [R.cpoint() for _ in range(4)]
    for q in weak:
        R.add(i0, q, -0.25)
    for q in weak + [c]:
        R.strong(R.new(), q)                     # somebody else depends on each of them as well
    A = R.matrix()
    dev = both(L, B, A, waves=waves)
    check_interpolation(A, dev)
    ii, jj, aa = dev["P"]
    assert dev["cf"][i0] == -1 and ii[1] - ii[0] == 1 and aa[0] == -1.0
    assert dev["path"]["rung"] == 0 and dev["path"]["declined"] == NONE


@pytest.mark.parametrize("theta", [0.0, 0.25, 0.9])
@pytest.mark.parametrize("max_row_sum", [0.8, 1.0])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_strength_thresholds(amg, theta, max_row_sum, n):
    """dyadic operands (every sum exact) at the thread-block edges, with rows exactly on both thresholds (random_operand,
    edges).  The pattern of S shows in the markers (-3 exactly on the empty rows, the PMIS rules) and in the sets of P —
    the edge rows are F points whose neighbours are C points, so their rows of P hold exactly their rows of S — both
    checked against the reference's S."""
    L, B = amg
    A = random_operand(n, seed=n, real=False, neg_frac=0.3, edges=True)
    assert A.shape[0] == n
    S = ref_strength(A, theta, max_row_sum)
    e0, e1, e2, e3 = n - 4, n - 3, n - 2, n - 1
    assert S[e0].size == 2 and S[e1].size == (0 if max_row_sum < 1.0 else 1 if theta == 0.9 else 2)
    assert S[e2].size == S[e3].size == {0.0: 3, 0.25: 2, 0.9: 1}[theta] and A.data[A.indptr[e3]] < 0
    dev = both(L, B, A, theta=theta, max_row_sum=max_row_sum)
    assert dev["levels"] == 2
    check_interpolation(A, dev, theta=theta, max_row_sum=max_row_sum)
    ii, cf = dev["P"][0], dev["cf"]
    for e in (e0, e1, e2, e3):
        assert cf[e] == (-1 if S[e].size else -3) and np.all(cf[S[e]] == 1) and ii[e + 1] - ii[e] == S[e].size


@pytest.mark.parametrize("waves", [0, 4])
@pytest.mark.parametrize("shape", ["clique", "star", "directed", "cycle", "path", "no_couplings"])
def test_pmis_graphs(amg, shape, waves):
    """S a clique of 40 (one C point), a star (a single C point in all), a directed unsymmetric pattern, a directed cycle
    (every point depends on the next one only: the nearest a marker comes to "all points C" — C points that depend on C
    points, and still an F point after every run of them), a path of 2000 points (many sweeps), and empty (every marker
    -3, no coarse level)"""
    L, B = amg
    R = Rows(3)
    if shape == "clique":
        p = [R.new() for _ in range(40)]
        for a in p:
            for b in p:
                if a != b:
                    R.strong(a, b)
        for _ in range(40):                    # and ordinary rows around it
            R.strong(R.new(), R.cpoint())
    elif shape == "star":
        hub = R.new()
        leaves = [R.new() for _ in range(200)]
        for l in leaves:
            R.strong(l, hub)
        R.strong(hub, leaves[0])
    elif shape == "directed":
        p = [R.new() for _ in range(300)]
        for a in p:
            for b in R.rng.choice(300, 3, replace=False):
                if a != b and b > a - 100:
                    R.strong(a, int(b))
    elif shape == "cycle":
        p = [R.new() for _ in range(300)]
        for a in p:
            R.strong(a, (a + 1) % 300)
    elif shape == "path":
        p = [R.new() for _ in range(2000)]
        for a in range(2000):
            for b in (a - 1, a + 1):
                if 0 <= b < 2000:
                    R.strong(a, b)
    else:
        for _ in range(200):
            R.new()
    A = R.matrix()
    dev = both(L, B, A, waves=waves)
    S = ref_strength(A, 0.25, 1.0)
    cf = dev["cf"]
    if shape == "no_couplings":
        assert np.all(cf == -3) and dev["levels"] == 1
        return
    check_interpolation(A, dev)
    if shape == "clique":
        assert np.sum(cf[:40] == 1) == 1
    if shape == "star":
        assert np.sum(cf == 1) == 1 and cf[0] == 1 and dev["P"][0][-1] == 201
    if shape == "cycle":
        c = cf == 1
        print("directed cycle: %d C points of 300, %d of them depend on a C point" % (c.sum(), np.sum(c & np.roll(c, -1))))
        assert 0 < c.sum() < 300
        assert np.any(c & np.roll(c, -1)), "no C point depends on a C point: the directed rule of check_pmis is not exercised"


# ---------------------------------------------------------------------------------------------------------------------
# batches of 64 neighbours, chunks of 64 flattened entries
# ---------------------------------------------------------------------------------------------------------------------
def chunk_shapes(lens):
    """lens: entries each of a row's neighbours contributes, in stored order, taken in batches of 64 neighbours whose
    entries are flattened and cut into chunks of 64.  Returns (a neighbour starts inside a chunk that the one before it
    had loaded, a neighbour's entries lie in three chunks or more)."""
    shared = three = False
    for b in range(0, len(lens), 64):
        e0, before = 0, False
        for l in lens[b:b + 64]:
            if l:
                e1 = e0 + l
                shared |= before and e0 % 64 != 0
                three |= (e1 - 1) // 64 - e0 // 64 >= 2
                e0, before = e1, True
    return shared, three


@pytest.mark.parametrize("waves", [0, 4])
@pytest.mark.parametrize("strong", [63, 64, 65, 128, 129])
def test_strong_neighbour_batches(amg, strong, waves):
    """point 0 with 63 ... 129 strong neighbours (the sb loop's batch edges; its row of A has strong + 1 entries: 65 and
    130 entries in the weights pass): 30 C points, the others F points with rows of S of 1, 63, 64, 65 and 130 entries
    — one chunk of 64 flattened entries then spans the end of one neighbour's row and the start of the next, and the
    130-entry row spans three chunks — out of one pool of 130 C points, so the set has 160 points (rung 2)"""
    L, B = amg
    lens = [1, 63, 64, 65, 130, 2, 61, 3]
    groups = [lens[q % len(lens)] for q in range(strong - 30)]
    A = long_row_operand(strong, real=True, direct=30, groups=groups, common=True, a_extra=70)
    assert A.indptr[1] - A.indptr[0] == strong + 1
    dev = both(L, B, A, waves=waves)
    sizes = check_interpolation(A, dev, kappa_max=3.0)
    assert dev["cf"][0] == -1 and sizes[0] == sizes.max() == 160
    # the chunks of 64 flattened entries, from the operand: the set pass flattens the rows of S of the F neighbours of a
    # batch of 64 strong neighbours, the weights pass the rows of A of the strong F neighbours among 64 entries of row 0
    cf, S = dev["cf"], ref_strength(A, 0.25, 1.0)
    isf = lambda j: cf[j] == -1
    s_lens = [len(S[j]) if isf(j) else 0 for j in S[0]]
    strong0 = set(S[0].tolist())
    a_lens = [A.indptr[j + 1] - A.indptr[j] if j in strong0 and isf(j) else 0 for j in A.indices[A.indptr[0] + 1:A.indptr[1]]]
    for name, lens in (("S", s_lens), ("A", a_lens)):
        shared, three = chunk_shapes(lens)
        assert shared and three, "%s: no chunk shared by two neighbours (%s) or no neighbour over three chunks (%s)" % (name, shared, three)
    rung = next(r for r in range(4) if sizes[0] <= ROOM[r])
    assert dev["path"] == dict(first=0, rung=rung, attempts=rung + 1, count_then_write=1, declined=NONE), (dev["path"], sizes[0])


# ---------------------------------------------------------------------------------------------------------------------
# the ladder
# ---------------------------------------------------------------------------------------------------------------------
def set_operand(size, real=True, direct=60):
    """point 0 with an interpolatory set of exactly `size` points: 60 direct C points, the rest through F neighbours of 10
    new C points each — the set passes 64 (and every later table size) in the middle of a ballot, with len below capR
    before the chunk"""
    direct = min(direct, size)
    rest = size - direct
    groups = [10] * (rest // 10) + ([rest % 10] if rest % 10 else [])
    return long_row_operand(1000 + size, real=real, direct=direct, groups=groups)


@pytest.mark.parametrize("size,rung", [(64, 0), (65, 1), (128, 1), (129, 2), (256, 2), (257, 3), (1024, 3)])
@pytest.mark.parametrize("waves", [0, 4])
def test_ladder(amg, size, rung, waves):
    """a set of exactly 64 ... 1024 points from the first rung: the rung that holds it, one attempt per rung on the way;
    65 and 129 are reached in the middle of a ballot (len + popcount > capR with len < capR before the chunk)"""
    L, B = amg
    A = set_operand(size)
    dev = both(L, B, A, waves=waves)
    sizes = check_interpolation(A, dev, kappa_max=3.0)
    assert sizes[0] == size == sizes.max()
    assert dev["interpolated"] == 1
    assert dev["path"] == dict(first=0, rung=rung, attempts=rung + 1, count_then_write=1, declined=NONE), dev["path"]


@pytest.mark.parametrize("size,rung", [(64, 0), (128, 1), (256, 2), (1024, 3)])
def test_table_filled_by_a_ballot(amg, size, rung):
    """no direct C point: every member of the set is appended by a ballot, the last ballot makes len + popcount == capR
    exactly, and the row still fits (the overflow test is >, not >=)"""
    L, B = amg
    A = set_operand(size, direct=0)
    dev = both(L, B, A)
    sizes = check_interpolation(A, dev, kappa_max=3.0)
    assert sizes[0] == size == sizes.max() and not np.any(dev["cf"][ref_strength(A, 0.25, 1.0)[0]] == 1)
    assert dev["path"] == dict(first=0, rung=rung, attempts=rung + 1, count_then_write=1, declined=NONE), dev["path"]


@pytest.mark.parametrize("first", [1, 3])
def test_first_rung_forced(amg, first):
    """the ladder entered at rung 1 and at rung 3: a set of 129 points needs rung 2"""
    L, B = amg
    A = set_operand(129)
    dev = both(L, B, A, rung=first)
    check_interpolation(A, dev, kappa_max=3.0)
    want = max(first, 2)
    assert dev["path"] == dict(first=first, rung=want, attempts=want - first + 1, count_then_write=1, declined=NONE), dev["path"]


def test_set_beyond_the_last_rung(amg):
    """1025 points: the device declines ("tables exhausted"), the host loop builds the level, the error flag stays clear
    (setup() checks it) and the level is the host's"""
    L, B = amg
    A = set_operand(1025)
    dev = both(L, B, A)
    sizes = check_interpolation(A, dev, kappa_max=3.0)
    assert sizes[0] == 1025
    assert dev["interpolated"] == 0
    assert dev["path"] == dict(first=0, rung=-1, attempts=4, count_then_write=1, declined=TABLES_EXHAUSTED), dev["path"]


# ---------------------------------------------------------------------------------------------------------------------
# the guard on the map's occupants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strong,rung", [(191, 0), (192, 1), (3071, 3), (3072, -1)])
def test_map_guard(amg, strong, rung):
    """A row's strong F neighbours all enter its map, beside a set of up to capR points; the map has 4 capR slots and a
    probe ends only at a free one.  The kernel starts a row only if strong < 3 capR: 191 strong neighbours (188 of them F)
    are the last count rung 0 admits, 192 the first it refuses — that row goes to rung 1 with the host's bits — and 3072
    pass the last rung's guard: the device declines, the host builds the level."""
    L, B = amg
    A = long_row_operand(strong, real=True, direct=3, groups=[2, 2], shared=1, pad_strong_f=strong - 5)
    assert len(ref_strength(A, 0.25, 1.0)[0]) == strong
    dev = both(L, B, A)
    sizes = check_interpolation(A, dev, kappa_max=3.0)
    assert dev["cf"][0] == -1 and sizes.max() < 64
    if rung >= 0:
        assert dev["interpolated"] == 1
        assert dev["path"] == dict(first=0, rung=rung, attempts=rung + 1, count_then_write=1, declined=NONE), dev["path"]
    else:
        assert dev["interpolated"] == 0
        assert dev["path"] == dict(first=0, rung=-1, attempts=4, count_then_write=1, declined=TABLES_EXHAUSTED), dev["path"]


# ---------------------------------------------------------------------------------------------------------------------
# truncation and storage
# ---------------------------------------------------------------------------------------------------------------------
def rescale(w, lim, keep):
    """A row cut down to the entries `keep`, with its sum restored: w'_k = w_k * total / kept, total and kept the sums of
    all and of the kept weights; left alone if kept is 0 or equals total.  lim_j bounds the error of the device's w_j.
    The device adds its own weights one by one (n = len(w) additions at most), divides and multiplies once, so to first
    order   |d total| <= sum lim + n eps/2 sum |w|,   |d kept| <= sum_kept lim + n eps/2 sum_kept |w|,
            |d w'_k|  <= lim_k |total / kept| + |w'_k| (|d total| / |total| + |d kept| / |kept| + eps),
    eps for the roundings of the division and the product, eps/2 each.  Returns w' and that bound."""
    total, kept = w.sum(), w[keep].sum()
    wk, lk = w[keep], lim[keep]
    if kept == 0 or kept == total:
        return wk, lk
    n = w.size
    d_total = lim.sum() + n * EPS / 2 * float(np.abs(w).sum())
    d_kept = lk.sum() + n * EPS / 2 * float(np.abs(wk).sum())
    out = wk * (total / kept)
    return out, lk * float(abs(total / kept)) + np.abs(out).astype(np.float64) * (d_total / float(abs(total)) + d_kept / float(abs(kept)) + EPS)


def ref_truncate(cols, w, lim, tol, pmx):
    """the relative threshold, then the pmx largest (the order of equal ones is not the library's: rows with ties are
    compared only where every order gives the same row), each with the row sum restored; columns, weights, bounds"""
    cols, w, lim = np.array(cols), w.copy(), np.asarray(lim, dtype=np.float64)
    if tol > 0 and w.size:
        keep = ~(np.abs(w) < tol * np.abs(w).max())
        w, lim = rescale(w, lim, keep)
        cols = cols[keep]
    if 0 < pmx < w.size:
        order = np.argsort(-np.abs(w), kind="stable")[:pmx]
        w, lim = rescale(w, lim, order)
        cols = cols[order]
    return cols, w, lim


@pytest.mark.parametrize("waves", [0, 4])
@pytest.mark.parametrize("pmx,trunc", [(1, 0.0), (2, 0.0), (4, 0.0), (4, 0.3), (2, 0.9), (100, 0.0), (100, 0.3)])
def test_truncation_without_ties(amg, pmx, trunc, waves):
    """random real weights: the rows the device keeps are the reference's — the same columns, as sets — and every row
    keeps its sum.  P_max_elmts 1, 2 and 4; together with a threshold, 0.9 dropping all but the largest entry of most
    rows; P_max_elmts above every row length (nothing cut, storage still strided).  Weights within the bound of
    rescale(), applied once per truncation step to the bound of the untruncated row."""
    L, B = amg
    A = random_operand(300, seed=21, real=True, neg_frac=0.0)
    dev = both(L, B, A, pmx=pmx, trunc=trunc, waves=waves)
    assert dev["interpolated"] == 1
    assert dev["path"] == dict(first=0, rung=0, attempts=1, count_then_write=0, declined=NONE), dev["path"]
    S = ref_strength(A, 0.25, 1.0)
    cf = dev["cf"]
    check_pmis(S, cf)
    ii, jj, aa = dev["P"]
    cut, worst = 0, 0.0
    for i, (cols, w, lim, kappa) in enumerate(ref_extpi(A, S, cf)):
        got_c, got_v = jj[ii[i]:ii[i + 1]], aa[ii[i]:ii[i + 1]]
        if cf[i] != -1:
            assert got_c.tolist() == list(cols); continue
        tc, tw, tl = ref_truncate(cols, w, lim, trunc, pmx)
        cut += tc.size < len(cols)
        assert sorted(got_c.tolist()) == sorted(tc.tolist()), "row %d keeps %s, the reference %s" % (i, got_c, tc)
        at = {c: k for k, c in enumerate(tc.tolist())}
        for c, v in zip(got_c.tolist(), got_v.tolist()):
            err, bound = abs(float(LD(v) - tw[at[c]])), float(tl[at[c]])
            assert err <= bound, "row %d column %d: %r vs %r, error %.3e, bound %.3e" % (i, c, v, float(tw[at[c]]), err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
    print("worst error / bound %.3f" % worst)
    assert (cut > 20) == (pmx < 100 or trunc > 0)


@pytest.mark.parametrize("pmx", [1, 2, 4])
def test_truncation_with_ties(amg, pmx):
    """dyadic weights (F rows that depend on 2 - 9 C points with equal couplings): which of the equal entries a row keeps
    is decided by the quicksort's tie order, which the device must share with the host (both() compares the bits)"""
    L, B = amg
    R = Rows(8)
    cs = [R.cpoint() for _ in range(60)]
    for q in range(120):
        f = R.new()
        for c in R.rng.choice(60, int(R.rng.integers(2, 10)), replace=False):
            R.strong(f, cs[int(c)])
    A = R.matrix()
    dev = both(L, B, A, pmx=pmx)
    assert dev["interpolated"] == 1 and dev["path"]["count_then_write"] == 0
    ii = dev["P"][0]
    assert np.diff(ii).max() == pmx and np.any(dev["cf"] == -1)


@pytest.mark.parametrize("waves", [0, 4])
@pytest.mark.parametrize("pmx,trunc", [(2, 0.0), (4, 0.5)])
def test_kept_sum_guards(amg, pmx, trunc, waves):
    """The two rows that a truncation step leaves unscaled, in the count step (2, 0) and in the threshold step (4, 0.5),
    on dyadic operands (every weight exact).  Row a: weights +1, -1 and 1/8 — the two kept ones add up to 0, and without
    the guard the row would be multiplied by 1/8 / 0.  Row b: weights 1, 1/2 and 0 — the dropped one is 0, the kept sum
    equals the row sum.  Each is an F point with one C neighbour and one F neighbour that has two C neighbours, to which
    the row itself has weak positive couplings: N = -1, p - 1/2, q - 1/2 over D = 1."""
    L, B = amg
    R = Rows(9)
    rows = []
    for p, q in ((1.5, 0.375), (None, 0.5)):
        i = R.new(diag=1.0)
        c1, c2, c3, k = R.cpoint(), R.cpoint(), R.cpoint(), R.new()
        R.strong(i, c1); R.strong(i, k); R.strong(k, c2); R.strong(k, c3)
        if p:
            R.add(i, c2, p)
        R.add(i, c3, q)
        rows.append(i)
    A = R.matrix()
    dev = both(L, B, A, pmx=pmx, trunc=trunc, waves=waves)
    assert dev["interpolated"] == 1 and dev["path"]["count_then_write"] == 0 and dev["path"]["declined"] == NONE
    cf = dev["cf"]
    S = ref_strength(A, 0.25, 1.0)
    check_pmis(S, cf)
    ref = ref_extpi(A, S, cf)
    ii, jj, aa = dev["P"]
    want = ([1.0, -1.0, 0.125], [1.0, 0.5, 0.0])
    for i, full in zip(rows, want):
        cols, w, lim, kappa = ref[i]
        assert cf[i] == -1 and sorted(w.tolist()) == sorted(full), (i, w)
        tc, tw, _ = ref_truncate(cols, w, lim, trunc, pmx)
        assert tc.size == 2 and w.sum() != 0
        if full[2]:
            assert tw.sum() == 0, "row a: the kept sum is not 0"
        else:
            assert tw.sum() == w.sum(), "row b: the kept sum is not the row sum"
        got = dict(zip(jj[ii[i]:ii[i + 1]].tolist(), aa[ii[i]:ii[i + 1]].tolist()))
        assert got == dict(zip(tc.tolist(), [float(x) for x in full[:2]])) == dict(zip(tc.tolist(), tw.astype(np.float64).tolist())), (i, got)


@pytest.mark.parametrize("waves", [0, 4])
@pytest.mark.parametrize("max_row_sum", [0.8, 1.0])
def test_zero_diagonals_and_empty_rows(amg, max_row_sum, waves):
    """300 dyadic rows of which 40 store a diagonal of 0 and 12 store nothing at all (relax 7 and no empty last row:
    module docstring).  A zero diagonal takes the branch of a positive one in the strength test and as a strong F
    neighbour (sgn = 1); with max_row_sum 0.8 such a row has no strong couplings unless its row sum is 0.  An empty row
    is marked -3 and skipped wherever another row holds its column."""
    L, B = amg
    A = random_operand(300, seed=41, real=False)
    n = A.shape[0]
    rng = np.random.default_rng(42)
    pick = rng.choice(n - 1, 52, replace=False)
    zero, empty = pick[:40], set(pick[40:].tolist())
    ptr, col, val = [0], [], []
    for i in range(n):
        if i not in empty:
            col += A.indices[A.indptr[i]:A.indptr[i + 1]].tolist()
            val += A.data[A.indptr[i]:A.indptr[i + 1]].tolist()
            if i in zero:
                val[ptr[-1]] = 0.0
        ptr.append(len(col))
    A = sp.csr_matrix((np.array(val), np.array(col, dtype=np.int32), np.array(ptr, dtype=np.int32)), shape=(n, n))
    assert A.nnz == len(val) and np.sum(A.data[A.indptr[:-1][np.diff(A.indptr) > 0]] == 0) == 40
    dev = both(L, B, A, relax=7, max_row_sum=max_row_sum, waves=waves)
    assert dev["levels"] == 2 and dev["interpolated"] == 1 and dev["path"]["rung"] == 0
    check_interpolation(A, dev, max_row_sum=max_row_sum)
    cf, S, plen = dev["cf"], ref_strength(A, 0.25, max_row_sum), np.diff(dev["P"][0])
    assert all(cf[i] == -3 and plen[i] == 0 for i in empty)
    assert any(np.any(np.isin(A.indices[A.indptr[i]:A.indptr[i + 1]], list(empty))) for i in np.flatnonzero(cf == -1))
    if max_row_sum == 1.0:
        assert np.any((cf[zero] == -1) & (plen[zero] > 0)) and np.any(cf[zero] == 1)
        assert any(np.any(np.isin(S[i][cf[S[i]] == -1], zero)) for i in np.flatnonzero(cf == -1)), "no strong F neighbour with a zero diagonal"
    else:
        assert np.any(cf[zero] == -3)


def test_no_truncation_counts_then_writes(amg):
    """P_max_elmts = 0 and trunc_factor = 0: lengths first, then columns and values"""
    L, B = amg
    A = random_operand(257, seed=31, real=True)
    dev = both(L, B, A, pmx=0, trunc=0.0)
    check_interpolation(A, dev, kappa_max=3.0)
    assert dev["path"] == dict(first=0, rung=0, attempts=1, count_then_write=1, declined=NONE), dev["path"]


def test_threshold_alone_is_declined(amg):
    """trunc_factor without P_max_elmts: row lengths would depend on the weights; the device declines ("threshold only")
    before any attempt and the host loop builds the level"""
    L, B = amg
    A = random_operand(257, seed=32, real=True)
    dev = both(L, B, A, pmx=0, trunc=0.3)
    assert dev["interpolated"] == 0 and dev["levels"] == 2
    assert dev["path"]["attempts"] == 0 and dev["path"]["rung"] == -1 and dev["path"]["declined"] == THRESHOLD_ONLY, dev["path"]
