"""Shared helpers for the tests: seeded inputs, small sparse matrices, and stand-alone host programs."""
import json
import os
import shutil
import subprocess

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# address and undefined-behaviour sanitizers, every warning an error; no contraction into fused multiply-adds and no -march,
# so that what a program computes depends on IEEE double arithmetic alone
HOST_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
              "-ffp-contract=off"]


def run_host_program(source, tmp_path, flags=HOST_FLAGS, cxx=None, timeout=120):
    """Builds the stand-alone program tests/<source> (its own main, host code only, hypre_amd/csrc on the include path) and
    runs it once; both must succeed.  Returns what it printed.  Nothing is loaded into python."""
    cxx = cxx or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / os.path.splitext(os.path.basename(source))[0])
    build = subprocess.run([cxx] + list(flags) + ["-I", os.path.join(ROOT, "hypre_amd", "csrc"), os.path.join(ROOT, "tests", source), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    return run.stdout


def assert_recorded_traces(stdout, which):
    """The `trace <run> <hash>` lines of a Krylov host check against tests/golden/krylov_host_traces.json: the same runs, and
    for each the same sequence of vector operations with the same scalars as the recorded commit's."""
    with open(os.path.join(ROOT, "tests", "golden", "krylov_host_traces.json")) as f:
        recorded = json.load(f)[which]
    printed = dict(line[len("trace "):].rsplit(" ", 1) for line in stdout.splitlines() if line.startswith("trace "))
    assert printed == recorded, {k: (printed.get(k), recorded.get(k)) for k in set(printed) | set(recorded) if printed.get(k) != recorded.get(k)}


def lcg_vector(n, seed=1):
    """Deterministic values in (-1, 1) from a fixed LCG (no platform RNG)."""
    out = np.empty(n)
    s = np.uint64(seed * 2654435761 % (2 ** 32) + 12345)
    a = np.uint64(6364136223846793005)
    c = np.uint64(1442695040888963407)
    with np.errstate(over="ignore"):
        for i in range(n):
            s = s * a + c
            out[i] = (float(s >> np.uint64(11)) / float(1 << 53)) * 2.0 - 1.0
    return out


def rand_vector(n, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def laplace_3d(nx, ny, nz, stencil=7):
    """Global 7- or 27-point Laplacian, diagonal first in every row."""
    N = nx * ny * nz
    rows, cols, vals = [], [], []
    idx = lambda x, y, z: (z * ny + y) * nx + x
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                r = idx(x, y, z)
                if stencil == 7:
                    nb = [(0, 0, -1), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
                    d = 6.0
                else:
                    nb = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                          if (dx, dy, dz) != (0, 0, 0)]
                    d = 26.0
                rows.append(r); cols.append(r); vals.append(d)
                for dx, dy, dz in nb:
                    X, Y, Z = x + dx, y + dy, z + dz
                    if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz:
                        rows.append(r); cols.append(idx(X, Y, Z)); vals.append(-1.0)
    # build CSR by hand to keep the stored order (scipy's coo->csr would sort/merge)
    rows = np.array(rows); cols = np.array(cols, dtype=np.int32); vals = np.array(vals)
    indptr = np.zeros(N + 1, dtype=np.int32)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr).astype(np.int32)
    A = sp.csr_matrix((vals, cols, indptr), shape=(N, N))
    return A


def parcsr(L, B, M, location):
    """one-rank ParCSR matrix whose diagonal block is M in its stored order (empty ghost block)"""
    n, m = M.shape
    par = L.hypre_ParCSRMatrixCreate(0, n, m, None, None, 0, 0, 0)
    L.hypre_ParCSRMatrixInitialize_v2(par, B.HYPRE_MEMORY_HOST)
    L.hypre_CSRMatrixDestroy(par.contents.diag)
    par.contents.diag = B.csr_from_arrays(n, m, M.indptr, M.indices, M.data, B.HYPRE_MEMORY_HOST)
    if location != B.HYPRE_MEMORY_HOST:
        L.hypre_ParCSRMatrixMigrate(par, location)
    B.check()
    return par


def random_csr(nrows, ncols, min_nnz, max_nnz, seed=0, empty_frac=0.0):
    """Rows with a uniformly random number of entries in [min_nnz, max_nnz], unsorted columns."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(min_nnz, max_nnz + 1, nrows)
    if empty_frac > 0:
        counts[rng.random(nrows) < empty_frac] = 0
    counts = np.minimum(counts, ncols)
    indptr = np.zeros(nrows + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(counts)
    indices = np.empty(indptr[-1], dtype=np.int32)
    for r in range(nrows):
        indices[indptr[r]:indptr[r + 1]] = rng.choice(ncols, counts[r], replace=False)
    data = rng.uniform(-1, 1, indptr[-1])
    return sp.csr_matrix((data, indices, indptr), shape=(nrows, ncols))


def banded_csr(nrows, ncols, min_nnz, max_nnz, band, seed=0, empty_frac=0.0):
    """Rows with a uniformly random number of entries in [min_nnz, max_nnz] at random, unsorted columns within `band` of the
    row's own position (scaled to the column range): the locality of an operator on a mesh, all values distinct."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(min_nnz, max_nnz + 1, nrows)
    if empty_frac > 0:
        counts[rng.random(nrows) < empty_frac] = 0
    indptr = np.zeros(nrows + 1, dtype=np.int32)
    lo = np.empty(nrows, dtype=np.int64)
    hi = np.empty(nrows, dtype=np.int64)
    for r in range(nrows):
        c = int(r * (ncols - 1) / max(nrows - 1, 1))
        lo[r], hi[r] = max(0, c - band), min(ncols, c + band + 1)
        counts[r] = min(counts[r], hi[r] - lo[r])
    indptr[1:] = np.cumsum(counts)
    indices = np.empty(indptr[-1], dtype=np.int32)
    for r in range(nrows):
        indices[indptr[r]:indptr[r + 1]] = lo[r] + rng.choice(hi[r] - lo[r], counts[r], replace=False)
    data = rng.uniform(-1, 1, indptr[-1])
    return sp.csr_matrix((data, indices, indptr), shape=(nrows, ncols))


def transpose_reference(indptr, indices, data, nrows, ncols):
    """(ti, tj, ta) of the transpose of a CSR matrix in plain numpy: a stable sort of the row-major entries by column, so
    row c of the transpose lists the rows holding column c in ascending order (seq_mv/csr_matop.c:1043-1270), values alongside."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    rows = np.repeat(np.arange(nrows), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    ti = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=ncols))])
    return ti, rows[order], np.asarray(data)[order]
