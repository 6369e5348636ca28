"""CPU: the geometries ss.active packs for the cloud kernels -- ftpGeometry, ftpMappingGeometry and GrayCode._geometry, for every
rig of the active goldens -- equal tests/golden/active_geom.npz byte for byte.  The fixture was written by the packing code as it
stood before the three builders were given one helper for the triangulation's entries (tests/golden/make_golden_active_geom.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_active_geom as MG                 # noqa: E402


def test_packed_geometries_equal_the_fixture_byte_for_byte():
    z = np.load(MG.OUT)
    want = {k: z[k] for k in z.files}
    got = MG.geometries()
    assert sorted(got) == sorted(want) and len(want) >= 100
    # all three builders are in it, and the rig without a depth offset only through the two that need no epipole
    assert {k.rsplit("/", 1)[1] for k in want} == {"ftp", "mapping", "graycode"}
    assert "active_ref/graycode/t2_zero_roi/graycode" in want and "active_ref/graycode/t2_zero_roi/ftp" not in want
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype == np.float64 and got[k].shape == (68,)
        assert got[k].tobytes() == want[k].tobytes(), k
        assert got[k].flags.c_contiguous and got[k].flags.writeable
