"""bench.py --dump-outputs (bench.dump_outputs) on the CPU, with a stand-in for the model: one
float64 <name>.npy per field of DUMP_FIELDS, whole while everything fits DUMP_MAX_BYTES, and
past it every larger field cut to the same fixed sample of points, so that two runs (two
builds) dump the same points."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Fields:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.f = {n: rng.standard_normal((2, 5, 7, 9)) for n in ("uVel", "vVel", "wVel", "theta", "salt")}
        self.f["etaN"] = rng.standard_normal((2, 7, 9))

    def get(self, name):
        return self.f[name].copy()


def _load(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d))}


def test_dump_outputs_whole(tmp_path):
    import bench
    m = _Fields(1)
    bench.dump_outputs(m, str(tmp_path / "out"))
    got = _load(str(tmp_path / "out"))
    assert set(got) == set(bench.DUMP_FIELDS)
    for n, a in got.items():
        assert a.dtype == np.float64 and np.array_equal(a, m.f[n]), n


def test_dump_outputs_sampled_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench
    cap = 6 * 8 * 200     # room for 200 points a field: the 3-D fields (630) are cut, etaN (126) is not
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    m = _Fields(2)
    bench.dump_outputs(m, str(tmp_path / "a"))
    bench.dump_outputs(m, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(x.nbytes for x in a.values()) <= cap
    idx = None
    for n in bench.DUMP_FIELDS:
        assert a[n].dtype == np.float64 and np.array_equal(a[n], b[n]), n
        if n == "etaN":
            assert np.array_equal(a[n], m.f[n])
            continue
        assert a[n].shape == (200,)
        flat = m.f[n].reshape(-1)
        here = np.flatnonzero(np.isin(flat, a[n]))
        assert np.array_equal(flat[here], a[n]), n      # the points in their own order
        assert idx is None or np.array_equal(idx, here), n   # the same points of every field
        idx = here


def test_plain_and_full_options_parse(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
