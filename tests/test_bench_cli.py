"""bench.py's command line beside the timed loop (no GPU): --full and --dump-outputs are
there, and dump_outputs writes the fleet's arrays as float64 .npy files within its size cap."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class _StubFleet:
    """The two calls dump_outputs makes, with the shapes of a horizon-N fleet."""

    def __init__(self, B, N=20):
        rs = np.random.RandomState(3)
        m = 7 * (N + 1) + 10 * N + 7
        self._st = dict(rec=rs.rand(B, 16), x=rs.rand(B, 7), Xw=rs.rand(B, N + 1, 7), Uw=rs.rand(B, N, 3),
                        y=rs.rand(B, m), rho=rs.rand(B))
        self._post = rs.rand(B, N, 3), rs.rand(B, N, 3)
        self._post[0][-1] = np.nan   # a landing that flew no step reads NaN
        self._post[1][-1] = np.nan

    def state(self):
        return self._st

    def posterior(self):
        return self._post


def test_dump_outputs_writes_float64_arrays(tmp_path):
    import bench
    fl = _StubFleet(5)
    bench.dump_outputs(fl, str(tmp_path / "out"))
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(n + ".npy" for n in ("records", "x", "Xw", "Uw", "y", "rho", "post_mean", "post_var"))
    got = {n[:-4]: np.load(tmp_path / "out" / n) for n in names}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["records"], fl.state()["rec"]) and np.array_equal(got["Xw"], fl.state()["Xw"])
    assert np.array_equal(got["post_mean"][:-1], fl.posterior()[0][:-1]) and np.all(got["post_var"][-1] == 0.0)
    bench.dump_outputs(fl, str(tmp_path / "out"), rank=2)
    assert os.path.exists(tmp_path / "out" / "records_rank2.npy")


def test_dump_outputs_keeps_to_64_mb(tmp_path):
    import bench
    fl = _StubFleet(16384)   # ~92 MB of state
    bench.dump_outputs(fl, str(tmp_path))
    files = [tmp_path / n for n in os.listdir(tmp_path)]
    assert sum(os.path.getsize(f) for f in files) <= 64 * 2 ** 20
    rec = np.load(tmp_path / "records.npy")
    assert 1 < len(rec) < 16384 and np.array_equal(rec, fl.state()["rec"][:len(rec)])


def test_options(capsys):
    import bench
    old = sys.argv
    sys.argv = ["bench.py", "--help"]
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    finally:
        sys.argv = old
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text and "--steps" in text
