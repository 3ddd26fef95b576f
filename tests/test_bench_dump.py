"""bench.py --dump-outputs: the MSM's affine point as msm_point.npy, float64 (2, 16) of 16-bit limbs,
least significant first; the identity as zeros.  CPU only."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _point(a):
    return tuple(sum(int(a[r, k]) << (16 * k) for k in range(16)) for r in range(2))


def test_dump_outputs_round_trips_a_point_and_the_identity(tmp_path):
    bench = _bench()
    p = ((1 << 253) + 0xFFFF0000FFFF, (0xABCD << 240) | 1)
    for name, pt, exp in (("a", p, p), ("b", None, (0, 0))):
        d = str(tmp_path / name / "nested")
        bench.dump_outputs(d, pt)
        assert os.listdir(d) == ["msm_point.npy"]
        a = np.load(os.path.join(d, "msm_point.npy"))
        assert a.dtype == np.float64 and a.shape == (2, 16)
        assert (a >= 0).all() and (a < 65536).all() and (a == np.floor(a)).all()
        assert _point(a) == exp
