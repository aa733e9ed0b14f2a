"""The batched vector operations (hypre_SeqVectorMassInnerProd / MassDotpTwo / MassAxpy, mass_kernels.hip) against the
one-at-a-time calls they replace, bit for bit: every sum equals hypre_SeqVectorInnerProd of the same pair, the update
equals k calls of hypre_SeqVectorAxpy in the order 0 .. k-1, `unroll` changes nothing and the inputs are left alone.
Sizes: empty, one element (tail only), one pair, an odd length below one workgroup, more than one workgroup with a tail,
196 workgroups (100 003), and the two odd lengths that pass a grid once: 524 288 + 515 takes a partial second trip through
the 1024 x 256 x 2 grid of a dot product, 1 048 576 + 515 through the 2048 x 256 x 2 grid of the update as well (and a
whole second trip and a partial third of the dot's) — lanes that went round once and lanes that went round twice meet in
one sum.  k on both sides of the chunk of 8, and three chunks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 255, 4097, 100003, 524288 + 515, 1048576 + 515)
COUNTS = (1, 2, 7, 8, 9, 17)
KMAX = max(COUNTS)
SHIFT = 1021              # the z_j of the two large sizes are windows of one seed block, this far apart

_cache = {}


def _vectors(n):
    """host data of one size, drawn once: x, y, KMAX vectors z and KMAX coefficients (fixed seed per size).  Above
    200 000 elements the z_j are overlapping windows of one block of n + KMAX * SHIFT numbers instead of KMAX x n."""
    if n not in _cache:
        rng = np.random.default_rng(20260000 + n)
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        if n > 200000:
            block = rng.standard_normal(n + KMAX * SHIFT)
            block.setflags(write=False)
            z = [block[j * SHIFT:j * SHIFT + n] for j in range(KMAX)]
        else:
            z = rng.standard_normal((KMAX, n))
            z.setflags(write=False)
        _cache[n] = dict(x=x, y=y, z=z, alpha=rng.standard_normal(KMAX))
        for k in ("x", "y", "alpha"):
            _cache[n][k].setflags(write=False)
    return _cache[n]


def _array(B, vecs):
    return (C.POINTER(B.Vector) * len(vecs))(*vecs)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_batched_sums_and_update_have_the_bits_of_the_single_calls(gpu_lib, n):
    from hypre_amd import binding as B
    lib = gpu_lib
    h = _vectors(n)
    x, y = B.vec_from_numpy(h["x"]), B.vec_from_numpy(h["y"])
    z = [B.vec_from_numpy(h["z"][j]) for j in range(KMAX)]
    one_x = np.array([lib.hypre_SeqVectorInnerProd(x, z[j]) for j in range(KMAX)])
    one_y = np.array([lib.hypre_SeqVectorInnerProd(y, z[j]) for j in range(KMAX)])
    B.check()
    if n:
        ref = np.array([float(np.dot(h["x"], h["z"][j])) for j in range(KMAX)])
        assert np.allclose(one_x, ref, rtol=0, atol=1e-12 * n)            # the yardstick itself is a dot product
    for k in COUNTS:
        zs = _array(B, z[:k])
        for unroll in (0, 4, 8):
            r = np.full(k, np.nan)
            assert lib.hypre_SeqVectorMassInnerProd(x, zs, k, unroll, B._rp(r)) == 0
            print("n", n, "k", k, "unroll", unroll, "MassInnerProd max |diff|", float(np.max(np.abs(r - one_x[:k]))))
            assert _bits(r) == _bits(one_x[:k]), (n, k, unroll, r, one_x[:k])
            rx, ry = np.full(k, np.nan), np.full(k, np.nan)
            assert lib.hypre_SeqVectorMassDotpTwo(x, y, zs, k, unroll, B._rp(rx), B._rp(ry)) == 0
            print("n", n, "k", k, "unroll", unroll, "MassDotpTwo max |diff|", float(np.max(np.abs(rx - one_x[:k]))), float(np.max(np.abs(ry - one_y[:k]))))
            assert _bits(rx) == _bits(one_x[:k]), (n, k, unroll)
            assert _bits(ry) == _bits(one_y[:k]), (n, k, unroll)
        # y += sum_j alpha_j z_j: k single updates in order against the batched one, as raw bytes
        alpha = np.array(h["alpha"][:k])
        step = B.vec_from_numpy(h["y"])
        for j in range(k):
            lib.hypre_SeqVectorAxpy(float(alpha[j]), z[j], step)
        want = B.vec_to_numpy(step)
        lib.hypre_SeqVectorDestroy(step)
        for unroll in (0, 4, 8):
            got = B.vec_from_numpy(h["y"])
            assert lib.hypre_SeqVectorMassAxpy(B._rp(alpha), zs, got, k, unroll) == 0
            out = B.vec_to_numpy(got)
            lib.hypre_SeqVectorDestroy(got)
            print("n", n, "k", k, "unroll", unroll, "MassAxpy max |diff|", float(np.max(np.abs(out - want))) if n else 0.0)
            assert out.tobytes() == want.tobytes(), (n, k, unroll)
        assert _bits(alpha) == _bits(h["alpha"][:k])
    B.check()
    # the inputs are what they were
    assert B.vec_to_numpy(x).tobytes() == _bits(h["x"]) and B.vec_to_numpy(y).tobytes() == _bits(h["y"])
    for j in range(KMAX):
        assert B.vec_to_numpy(z[j]).tobytes() == _bits(h["z"][j])
    for v in [x, y] + z:
        lib.hypre_SeqVectorDestroy(v)


def test_an_operand_may_appear_twice(gpu_lib):
    """COGMRES hands MassDotpTwo the previous direction both as y and as one of the z_j, and a norm is <x, x>."""
    from hypre_amd import binding as B
    lib = gpu_lib
    h = _vectors(4097)
    z = [B.vec_from_numpy(h["z"][j]) for j in range(3)]
    zs = _array(B, z)
    rx, ry = np.zeros(3), np.zeros(3)
    lib.hypre_SeqVectorMassDotpTwo(z[2], z[1], zs, 3, 0, B._rp(rx), B._rp(ry))
    for j in range(3):
        assert rx[j] == lib.hypre_SeqVectorInnerProd(z[2], z[j]) and ry[j] == lib.hypre_SeqVectorInnerProd(z[1], z[j])
    B.check()
    for v in z:
        lib.hypre_SeqVectorDestroy(v)


def test_no_vectors_is_a_no_op_and_host_operands_are_refused(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    h = _vectors(255)
    x, y = B.vec_from_numpy(h["x"]), B.vec_from_numpy(h["y"])
    r = np.full(2, 7.0)
    assert lib.hypre_SeqVectorMassInnerProd(x, None, 0, 0, B._rp(r)) == 0
    assert lib.hypre_SeqVectorMassDotpTwo(x, y, None, 0, 0, B._rp(r), B._rp(r)) == 0
    assert lib.hypre_SeqVectorMassAxpy(None, None, y, 0, 0) == 0
    assert list(r) == [7.0, 7.0] and B.vec_to_numpy(y).tobytes() == _bits(h["y"])
    B.check()
    host = B.vec_from_numpy(h["y"], location=B.HYPRE_MEMORY_HOST)
    for call in (lambda: lib.hypre_SeqVectorMassInnerProd(x, _array(B, [host]), 1, 0, B._rp(r)),
                 lambda: lib.hypre_SeqVectorMassDotpTwo(x, host, _array(B, [y]), 1, 0, B._rp(r), B._rp(r)),
                 lambda: lib.hypre_SeqVectorMassAxpy(B._rp(r), _array(B, [x]), host, 1, 0)):
        lib.HYPRE_ClearAllErrors()
        assert call() != 0 and b"device memory" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    for v in (x, y, host):
        lib.hypre_SeqVectorDestroy(v)
