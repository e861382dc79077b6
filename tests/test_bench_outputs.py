"""bench.py --dump-outputs: the frames of the last timed step as DIR/<field>.npy (CPU: dump_outputs on made-up frames)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _frames(n, payload_len=1024):
    rng = np.random.default_rng(5)
    out = []
    for i in range(n):
        f = {k: i + 1 for k in bench.DUMP_INT}
        f.update({k: np.float32(0.25 * i - 1.0) for k in bench.DUMP_FLT})
        f["start"] = 17322 * i + 19_999_000                      # beyond float32's exact integers
        f["header"] = bytes(rng.integers(0, 256, 20, dtype=np.uint8))
        f["payload"] = bytes(rng.integers(0, 256, payload_len - (i % 2) * 24, dtype=np.uint8))
        out.append(f)
    return out


def test_every_frame_written_as_float_arrays(tmp_path):
    fr = _frames(5)
    names = bench.dump_outputs(str(tmp_path), fr)
    assert sorted(p[:-4] for p in os.listdir(tmp_path)) == names
    for n in names:
        assert np.load(tmp_path / (n + ".npy")).dtype in (np.float32, np.float64)
    g = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert g["frame_index"].tolist() == list(range(5))
    assert g["start"].tolist() == [f["start"] for f in fr]
    assert g["payload"].shape == (5, 1024) and g["header"].shape == (5, 20)
    for i, f in enumerate(fr):
        L = len(f["payload"])
        assert g["payload_len"][i] == L and bytes(g["payload"][i, :L].astype(np.uint8)) == f["payload"]
        assert (g["payload"][i, L:] == -1).all()
        assert bytes(g["header"][i].astype(np.uint8)) == f["header"]
        assert all(g[k][i] == np.float32(f[k]) for k in bench.DUMP_FLT)


def test_large_outputs_are_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * 4200)
    fr = _frames(100)
    bench.dump_outputs(str(tmp_path / "a"), fr)
    bench.dump_outputs(str(tmp_path / "b"), fr)
    ia, ib = (np.load(tmp_path / d / "frame_index.npy") for d in ("a", "b"))
    assert 0 < len(ia) < 100 and ia.tolist() == ib.tolist() and (np.diff(ia) > 0).all()
    total = sum(os.path.getsize(tmp_path / "a" / p) for p in os.listdir(tmp_path / "a"))
    assert total <= 40 * 4200 + 16 * 128                     # + the .npy headers
    assert np.load(tmp_path / "a" / "start.npy").tolist() == [fr[int(i)]["start"] for i in ia]
