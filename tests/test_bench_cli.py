"""CPU: bench.py's command line and its output dump.  A plain run is the default and --full opts into the extra figures;
--steps below 1 is refused; --dump-outputs writes float64 arrays of at most 64 MB, every row of a small iterate and the
same seeded sample of a large one on every run."""
import sys

import numpy as np
import pytest

import bench

LIMIT_BYTES = 64 << 20


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)


def test_full_and_dump_outputs_parse(monkeypatch, tmp_path):
    a = _parse(monkeypatch, "--steps", "3", "--full", "--dump-outputs", str(tmp_path))
    assert (a.steps, a.full, a.dump_outputs) == (3, True, str(tmp_path))


@pytest.mark.parametrize("steps", ["0", "-1"])
def test_steps_below_one_are_refused(monkeypatch, steps):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", steps)


def test_dump_writes_every_row_of_a_small_iterate(tmp_path):
    u = np.random.default_rng(5).standard_normal(1000)
    bench.dump_outputs(str(tmp_path / "out"), u, 0, 1)
    got = np.load(tmp_path / "out" / "u.npy")
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, u)


def test_dump_samples_a_large_iterate_the_same_rows_every_time(tmp_path):
    u = np.arange(bench.DUMP_VALUES + 54321, dtype=np.float64)        # value = row index
    bench.dump_outputs(str(tmp_path / "a"), u, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), u, 0, 1)
    a, b = np.load(tmp_path / "a" / "u.npy"), np.load(tmp_path / "b" / "u.npy")
    assert a.dtype == np.float64 and a.size == bench.DUMP_VALUES
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < u.size     # distinct rows, in order
    assert (tmp_path / "a" / "u.npy").stat().st_size <= LIMIT_BYTES


def test_dump_of_several_ranks_stays_within_the_limit(tmp_path):
    world = 4
    for rank in range(world):
        bench.dump_outputs(str(tmp_path), np.full(bench.DUMP_VALUES, float(rank)), rank, world)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["u_rank%d.npy" % r for r in range(world)]
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= LIMIT_BYTES
    for rank in range(world):
        assert np.all(np.load(tmp_path / ("u_rank%d.npy" % rank)) == rank)
