import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "news-recommendation-tc_amd")
for p in (PKG, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs on the GPU box)")
    config.addinivalue_line("markers", "slow: long-running")


class GoldenParts(dict):
    """A fixture stored as <name>.0.npz, <name>.1.npz, ... (no committed file
    is larger than 1 MiB; tests/golden/make_golden.py save_parts), read like
    the one .npz it stands for: the same keys in the same order (``files``)
    and the same arrays, pieces "<key>@@<i>of<n>" concatenated along axis 0."""

    def __init__(self, stem):
        import glob

        import numpy as np

        got = {}
        paths = glob.glob(glob.escape(stem) + ".[0-9]*.npz")
        for path in paths:
            with np.load(path, allow_pickle=False) as z:
                got.update({k: z[k] for k in z.files})
        assert paths and "__keys__" in got, f"no fixture {stem}.npz or {stem}.<i>.npz"
        for k in got["__keys__"].tolist():
            if k in got:
                self[k] = got.pop(k)
            else:
                n = int(next(p for p in got if p.startswith(k + "@@")).rsplit("of", 1)[1])
                self[k] = np.concatenate([got.pop(f"{k}@@{i}of{n}") for i in range(n)], axis=0)
        assert list(got) == ["__keys__"], sorted(got)  # every stored piece belongs to a key

    @property
    def files(self):
        return list(self)


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    cache = {}

    def load(name):
        if name not in cache:
            path = os.path.join(GOLDEN, name + ".npz")
            cache[name] = np.load(path, allow_pickle=False) if os.path.exists(path) else GoldenParts(path[:-4])
        return cache[name]

    return load
