"""oracle.fixtures: a golden fixture over the committed-file size limit is stored as row blocks beside it and
read back bit for bit; every committed fixture file is under 1 MiB."""
import glob
import os

import numpy as np

from oracle import fixtures

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_split_fixture_round_trip(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    feats = rng.standard_normal((7, 40, 50)).astype(np.float32)  # incompressible rows, 8 kB each
    feats[2] = 0.0  # and one that compresses to nothing, so the blocks come out uneven
    arrays = {"features": feats, "tokens": np.arange(21, dtype=np.int64).reshape(7, 3), "max_length": np.int64(128)}
    monkeypatch.setattr(fixtures, "PART_LIMIT", 20000)
    path = str(tmp_path / "fx.npz")
    files = fixtures.save_fixture(path, arrays)
    assert files[0] == path and len(files) > 2 and all(os.path.getsize(f) <= 20000 for f in files)
    assert sorted(files) == sorted(glob.glob(str(tmp_path / "*")))
    assert "features" not in np.load(path).files
    got = fixtures.load_fixture(path)
    assert sorted(got) == sorted(arrays)
    for k, v in arrays.items():
        assert got[k].dtype == np.asarray(v).dtype and got[k].tobytes() == np.asarray(v).tobytes(), k
    # a later, smaller version of the fixture fits one file: the parts of the earlier split go away
    small = dict(arrays, features=feats[:1])
    assert fixtures.save_fixture(path, small) == [path] and glob.glob(str(tmp_path / "*")) == [path]
    np.testing.assert_array_equal(fixtures.load_fixture(path)["features"], feats[:1])


def test_committed_fixtures_under_one_mib():
    files = glob.glob(os.path.join(GOLD, "*"))
    assert files
    over = {os.path.basename(f): os.path.getsize(f) for f in files if os.path.getsize(f) > 1 << 20}
    assert not over, over
