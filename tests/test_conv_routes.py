"""CPU check of the convolution routing (csrc/conv.hip): for every case and fd_tuning setting in tests/golden/conv_routes.npz
(written by tests/golden/make_conv_routes.py), the size queries, the BatchNorm / statistics flags and the weight re-layout jobs
give the recorded answers.  These calls only fill host structs; no GPU is needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib_path():
    from fusiondepth_amd import build
    return build.build(verbose=False)


def test_conv_routes_match_the_table(lib_path):
    sys.path.insert(0, GOLDEN)
    try:
        import make_conv_routes as gen
    finally:
        sys.path.remove(GOLDEN)
    z = np.load(os.path.join(GOLDEN, "conv_routes.npz"))
    descs, settings = z["desc"], [str(s) for s in z["settings"]]
    assert len(descs) > 500 and len(settings) == len(gen.SETTINGS)
    got = gen.evaluate(descs, settings)
    for key in ("sizes", "bn_ok", "njobs", "jobs"):
        want = z[key]
        bad = np.argwhere(got[key] != want)
        assert bad.size == 0, "%s differs for %d entries; first: setting %r, case %s: got %s, want %s" % (
            key, len(bad), settings[bad[0][0]], descs[bad[0][1]].tolist(), got[key][tuple(bad[0][:2])].tolist(),
            want[tuple(bad[0][:2])].tolist())
