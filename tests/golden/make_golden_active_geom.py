"""The packed geometries of ss.active for every rig of the active goldens: the 68 doubles of ftpGeometry, ftpMappingGeometry
and GrayCode._geometry, as the package packed them when this fixture was written (tests/golden/active_geom.npz).  They are the
input of the cloud kernels, and a disparity of exactly 0 does not survive a last-bit difference in them, so a change of the packing
code must reproduce them byte for byte (tests/test_active_geom_cpu.py).

    python tests/golden/make_golden_active_geom.py        (needs no GPU)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "active_geom.npz")


def _entries():
    """-> (key, rig json entry, z_plane, period, roi) of every case of the active goldens that carries a rig"""
    def load(name):
        with open(os.path.join(HERE, name)) as f:
            return json.load(f)
    cloud, mapping, stereo, ref = (load(n + ".json") for n in ("ftp_cloud_cases", "ftp_mapping_cases", "stereo_ftp_cases",
                                                                "active_ref_cases"))
    for name, c in sorted(cloud["cases"].items()):
        yield "ftp_cloud/" + name, c["rig"], c["z_plane"], c["period"], c["roi"]
    for name, c in sorted(mapping["cloud"].items()):
        yield "ftp_mapping/" + name, c["rig"], 1000.0, mapping["period"], c["roi"]
    for group in ("reference", "cloud"):
        for name, c in sorted(stereo[group].items()):
            yield "stereo_ftp/%s/%s" % (group, name), c["rig"], c["z_plane"], stereo["period"], c["roi"]
    for group in ("ftp", "mapping", "phase_only", "graycode"):
        for name, c in sorted(ref[group].items()):
            # (GrayCode's roi holds end coordinates, not a size: the whole image serves here)
            yield "active_ref/%s/%s" % (group, name), c["rig"], c.get("z_plane", 1000.0), 12.0, None if group == "graycode" else c.get("roi")


def geometries():
    """-> {key: float64 [68]}; a builder that refuses a rig (T[2] == 0 for ftpGeometry) leaves its key out"""
    import simplestereo_amd as ss
    a = ss.active
    out = {}
    for key, r, z_plane, period, roi in _entries():
        roi = None if roi is None else tuple(roi)

        def rig():
            return ss.StereoRig(tuple(r["res1"]), tuple(r["res2"]), r["intrinsic1"], r["intrinsic2"], r["distCoeffs1"], r["distCoeffs2"],
                                r["R"], r["T"])
        for what, build in (("ftp", lambda: a.ftpGeometry(rig(), z_plane, period, roi).geom),
                            ("mapping", lambda: a.ftpMappingGeometry(rig(), period, roi).geom),
                            ("graycode", lambda: a.GrayCode(rig())._geometry())):
            try:
                g = build()
            except ValueError:
                continue
            assert g.dtype == np.float64 and g.shape == (68,)
            out["%s/%s" % (key, what)] = g
    return out


if __name__ == "__main__":
    g = geometries()
    np.savez_compressed(OUT, **g)
    print("wrote %s: %d geometries, %d bytes" % (OUT, len(g), os.path.getsize(OUT)))
