"""CPU: extended (interp_type 14) and extended+i "if no common C point" (7) interpolation beside extended+i (6).

Type 7 is pinned by two goldens of the reference's regression set (test/TEST_ij/interp.saved, 4 ranks).  Type 14 has no job
there; it is checked against a restatement of the weight formula in numpy longdouble (dictionaries per row, written from

    w_ij = -( a_ij + sum_{k in F_i^s} a_ik a^-_kj / sum_{l in D} a^-_kl ) / a~_ii ,

D = C^_i u {i} for types 6 and 7 and C^_i for type 14), by its pattern (that of type 6), by P 1 = 1 on rows of zero row sum
and by rank invariance.  The same restatement runs against types 6 and 7, which the goldens pin: that validates it.

The bound on a weight.  The library forms a weight from n_t numerator terms t (a_ij and one a_ik a^-_kj / d_k per
distributing F neighbour k), n_s terms s of the diagonal a~_ii (a_ii, the weak couplings, the lumped a_ik and the "+i"
shares a_ik a^-_ki / d_k) and, per distributing neighbour, a denominator d_k of q_k terms of one sign.  A term carries at
most q_k + 2 roundings (its denominator's sum, a division, a product), the two sums n_t and n_s more, the final division one.
With N the count of all these operations the textbook bound for recursive summation (every operation within 2^-53 relative,
gamma_N = N 2^-53 / (1 - N 2^-53) <= N 2^-52) gives

    |w - w_ref| <= N 2^-52 ( sum |t| + |w_ref| sum |s| ) / |a~_ii| ,

N and both sums taken from the restatement's own count: no constant is fitted."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_dist_golden import run_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_interp.json")))
LD = np.longdouble


@pytest.mark.parametrize("name", sorted(GOLD))
def test_reference_goldens_of_type_7(name):
    case = GOLD[name]
    out = run_ranks(case["ranks"], case)
    for key in ("conv_factor", "grid", "operator"):
        assert abs(out[key] - case["expect"][key]) < 5.1e-7, (key, out[key], case["expect"][key])


# ---------------------------------------------------------------------------
# level 0 of a host hierarchy: A, S, the C/F marker and P
# ---------------------------------------------------------------------------
def level0(lib, **kw):
    from hypre_amd import binding as B, ij
    opt = ij.check_options(ij.IJOptions(**kw))
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_HOST)
    try:
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, 0), C.POINTER(B.ParCSRMatrix)).contents
        Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, 0), C.POINTER(B.ParCSRMatrix)).contents
        ia = C.cast(lib.hypre_amd_BoomerAMGGetCFMarker(s, 0), C.POINTER(B.IntArray)).contents
        out = dict(A=B.csr_to_arrays(Al.diag), P=B.csr_to_arrays(Pl.diag), cf=B.fetch(ia.data, ia.size, np.int32, ia.memory_location))
        Sp = C.c_void_p()
        lib.hypre_BoomerAMGCreateS(A, opt.strong_threshold, opt.max_row_sum, 1, None, C.byref(Sp))
        B.check()
        S = C.cast(Sp, C.POINTER(B.ParCSRMatrix))
        si, sj, _ = B.csr_to_arrays(S.contents.diag)
        lib.hypre_ParCSRMatrixDestroy(S)
        out["S"] = [set(int(j) for j in sj[si[i]:si[i + 1]]) for i in range(len(si) - 1)]
    finally:
        lib.HYPRE_BoomerAMGDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)
    return out


PROBLEMS = {
    "7pt": dict(n=(9, 8, 7)),
    "27pt": dict(n=(7, 7, 6), problem="27pt"),
    "difconv": dict(n=(8, 7, 6), problem="difconv", a=(3.0, 2.0, 1.0)),
    # h = 1/9, 1/8, 1/7: -1/h^2 + a/h > 0 in every direction — the couplings of the sign of the diagonal the sign test drops
    "difconv-positive": dict(n=(8, 7, 6), problem="difconv", a=(30.0, 20.0, 10.0)),
    "rotate": dict(n=(24, 20, 1), problem="rotate", alpha=60.0, eps=0.1),
}
TWO_LEVELS = dict(max_levels=2, P_max_elmts=0, trunc_factor=0.0, coarsen_type=8)
_level0 = {}


def hierarchy(lib, problem, interp_type):
    """computed once per (problem, type), shared by the tests below, never changed"""
    key = (problem, interp_type)
    if key not in _level0:
        _level0[key] = level0(lib, interp_type=interp_type, **dict(PROBLEMS[problem], **TWO_LEVELS))
    return _level0[key]


def restated_rows(h, interp_type):
    """{i: {coarse column: (w_ref, bound)}} for the F rows, from the formula of the module docstring"""
    ai, aj, aa = h["A"]
    cf, S = h["cf"], h["S"]
    n = len(cf)
    row = [{int(aj[k]): LD(aa[k]) for k in range(ai[i], ai[i + 1])} for i in range(n)]
    coarse = np.cumsum(cf >= 0) - 1
    is_c = lambda j: cf[j] >= 0
    is_f = lambda j: cf[j] < 0 and cf[j] != -3
    out = {}
    for i in range(n):
        if not is_f(i):
            continue
        Cs = {j for j in S[i] if is_c(j)}
        Fs = {k for k in S[i] if is_f(k)}
        hat = set(Cs)
        for k in Fs:
            Ck = {j for j in S[k] if is_c(j)}
            if interp_type != 7 or not (Ck & Cs):
                hat |= Ck
        D = hat | ({i} if interp_type != 14 else set())
        num = {j: [row[i][j]] if j in row[i] else [] for j in hat}            # the terms of every numerator
        diag = [row[i][i]]
        ops = 0
        for k, a_ik in row[i].items():
            if k == i or k in hat:
                continue
            if k in Fs:
                opposite = lambda v, d=row[k][k]: (v < 0) if d >= 0 else (v > 0)
                bar = {l: v for l, v in row[k].items() if l != k and l in D and opposite(v)}
                d_k = sum(bar.values(), LD(0))
                if d_k == 0:
                    diag.append(a_ik)
                    continue
                ops = max(ops, len(bar) + 2)
                for l, v in bar.items():
                    (diag if l == i else num[l]).append(a_ik * v / d_k)
            elif cf[k] != -3:
                diag.append(a_ik)                                             # weak: lumped
        a_tilde = sum(diag, LD(0))
        sum_s = sum(abs(s) for s in diag)
        out[i] = {}
        for j in hat:
            w = -sum(num[j], LD(0)) / a_tilde
            N = len(num[j]) + len(diag) + ops + 1
            bound = N * LD(2.0) ** -52 * (sum(abs(t) for t in num[j]) + abs(w) * sum_s) / abs(a_tilde)
            out[i][int(coarse[j])] = (w, bound)
    return out


@pytest.mark.parametrize("interp_type", [6, 7, 14])
@pytest.mark.parametrize("problem", sorted(PROBLEMS))
def test_weights_are_those_of_the_formula(lib, problem, interp_type):
    h = hierarchy(lib, problem, interp_type)
    pi, pj, pa = h["P"]
    ref = restated_rows(h, interp_type)
    assert len(ref) > 20
    worst = 0.0
    for i, want in ref.items():
        got = {int(pj[k]): pa[k] for k in range(pi[i], pi[i + 1])}
        assert set(got) == set(want), (problem, interp_type, i)
        for j, (w, bound) in want.items():
            err = abs(LD(got[j]) - w)
            worst = max(worst, float(err / bound) if bound else 0.0)
            assert err <= bound, (problem, interp_type, i, j, float(w), got[j], float(err), float(bound))
    print("%s type %d: largest error / bound = %.3f" % (problem, interp_type, worst))


@pytest.mark.parametrize("problem", sorted(PROBLEMS))
def test_extended_has_the_pattern_of_extended_plus_i(lib, problem):
    p6, p14 = hierarchy(lib, problem, 6)["P"], hierarchy(lib, problem, 14)["P"]
    assert np.array_equal(p6[0], p14[0]) and np.array_equal(p6[1], p14[1])


def test_extended_interpolates_constants_where_the_row_sum_is_zero(lib):
    h = hierarchy(lib, "7pt", 14)
    ai, aj, aa = h["A"]
    pi, pj, pa = h["P"]
    ref = restated_rows(h, 14)
    rows = [i for i in ref if ai[i + 1] - ai[i] == 7 and np.sum(aa[ai[i]:ai[i + 1]]) == 0.0]
    assert len(rows) > 10
    for i in rows:
        w = pa[pi[i]:pi[i + 1]]
        # the weights' own bounds, and one rounding per addition of the row sum
        bound = sum(b for _, b in ref[i].values()) + len(w) * LD(2.0) ** -52 * np.sum(np.abs(w))
        assert abs(np.sum(w.astype(LD)) - 1) <= bound, (i, float(np.sum(w)), float(bound))


def test_type_7_sets_lie_between_direct_and_extended(lib):
    opts = dict(n=(12, 11, 10), problem="27pt", **TWO_LEVELS)
    h6, h7 = level0(lib, interp_type=6, **opts), level0(lib, interp_type=7, **opts)
    assert np.array_equal(h6["cf"], h7["cf"])
    cf, S = h7["cf"], h7["S"]
    coarse = np.cumsum(cf >= 0) - 1
    smaller = 0
    for i in np.flatnonzero(cf < 0):
        s6 = set(h6["P"][1][h6["P"][0][i]:h6["P"][0][i + 1]].tolist())
        s7 = set(h7["P"][1][h7["P"][0][i]:h7["P"][0][i + 1]].tolist())
        assert s7 <= s6
        assert {int(coarse[j]) for j in S[i] if cf[j] >= 0} <= s7
        smaller += s7 < s6
    assert smaller > 0          # the "common C point" branch was taken


@pytest.mark.parametrize("interp_type", [7, 14])
def test_host_setup_of_the_new_types_does_not_depend_on_the_thread_count(lib, interp_type):
    from hypre_amd import binding as B, ij
    hier = []
    try:
        for threads in (1, 8):
            lib.hypre_amd_SetHostThreads(threads)
            opt = ij.IJOptions(n=(40, 38, 36), coarsen_type=8, relax_type=18, interp_type=interp_type)
            A = ij.build_matrix(opt)
            s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_HOST)
            lib.HYPRE_BoomerAMGSetup(s, A, None, None)
            B.check()
            nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
            lv = []
            for l in range(nl):
                Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
                lv.append(B.csr_to_arrays(Al.contents.diag))
                if l < nl - 1:
                    Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, l), C.POINTER(B.ParCSRMatrix))
                    lv.append(B.csr_to_arrays(Pl.contents.diag))
            hier.append(lv)
            lib.HYPRE_BoomerAMGDestroy(s)
            lib.hypre_ParCSRMatrixDestroy(A)
    finally:
        lib.hypre_amd_SetHostThreads(lib.hypre_amd_HostCpuShare())
    assert len(hier[0]) == len(hier[1]) and len(hier[0]) > 4
    for m0, m1 in zip(hier[0], hier[1]):
        for a, b in zip(m0, m1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("interp_type", [14, 7])
def test_distributed_interpolation_is_rank_invariant(interp_type):
    """As test_dist_golden.py::test_distributed_direct_interpolation_is_rank_invariant: -pmis1 and slabs in z keep the
    C/F splitting of one rank, l1-Jacobi (relax 18) keeps the smoother independent of the partition; three levels, no
    truncation (the reasons are given there)."""
    opts = {"n": [14, 13, 12], "coarsen_type": 9, "interp_type": interp_type, "relax_type": 18, "max_levels": 3, "P_max_elmts": 0}
    one = run_ranks(1, {"options": dict(opts, rhs="one")})
    four = run_ranks(4, {"options": dict(opts, rhs="one", P=[1, 1, 4])})
    assert one["levels"] == four["levels"] and one["sizes"] == four["sizes"]
    assert abs(one["grid"] - four["grid"]) < 1e-12 and abs(one["operator"] - four["operator"]) < 1e-12
    assert one["iterations"] == four["iterations"]


def _setup_error(lib, **kw):
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(n=(8, 8, 8), **{k: v for k, v in kw.items() if k != "interp_type"})
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_HOST)
    lib.HYPRE_BoomerAMGSetInterpType(s, kw["interp_type"])
    try:
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        with pytest.raises(B.HypreAmdError) as e:
            B.check()
    finally:
        lib.HYPRE_BoomerAMGDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)
        lib.HYPRE_ClearAllErrors()
    return str(e.value)


def test_other_types_keep_failing_and_the_message_names_the_four(lib):
    msg = _setup_error(lib, interp_type=8)
    for t in ("3", "6", "7", "14"):
        assert t in msg.split("interp_type", 1)[1].replace("(", " ").replace(",", " ").split(), msg


@pytest.mark.parametrize("interp_type", [7, 14])
def test_systems_are_refused_with_the_new_types(lib, interp_type):
    assert "num_functions > 1" in _setup_error(lib, interp_type=interp_type, num_functions=2)


def test_driver_takes_the_new_types_in_code_and_refuses_them_on_the_command_line():
    from hypre_amd import ij
    for t in (7, 14):
        assert ij.check_options(ij.IJOptions(interp_type=t)).interp_type == t
    with pytest.raises(SystemExit):
        ij.check_options(ij.IJOptions(interp_type=8))
    with pytest.raises(SystemExit):
        ij.parse_cli(["-interptype", "14"])
