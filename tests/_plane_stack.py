"""What the tests of the shared plane-stack front (Gray code and phase shift: one check, one staging, one device frame) hold the
code to, recorded from the commit BEFORE the fold and kept under tests/golden/:
  plane_stack_errors.json         ssamd_last_error() of every bad argument of the two decoders' argument-error tests, per route
  phaseshift_parent_digests.json  SHA-256 of phaseShiftDecode's bytes on the MI355X, host route, every recorded case and modulation
  plane_stack_geometry.json       the packed triangulation geometry of GrayCode and StructuredLightRig on the recorded rigs
The lists of bad arguments live here, so the older tests and the recorded messages read one list.

    python tests/_plane_stack.py errors | geometry | digests      (digests needs the GPU; run on the commit to record FROM)"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTES = ("host", "device")


def phase_bad(maps):
    """the bad arguments of ssamd_phaseshift_decode on 20 planes of 4 x 8, 3 x-periods and 2 y-periods; ``maps`` a float32 [4, 8]"""
    return [dict(planes=None), dict(out=None), dict(tx=None), dict(ty=None), dict(h=-1), dict(w=-1), dict(x0=-1), dict(y0=-1), dict(x0=1), dict(y0=1), dict(w=9),
            dict(h=5), dict(n=16), dict(n=24), dict(nx=0, ny=5), dict(nx=9, ny=-4), dict(ny=0, nx=5), dict(ny=9, nx=-4), dict(thr2=-1), dict(pw=0), dict(ph=0),
            dict(pw=65537), dict(ph=65537), dict(mx=maps.ctypes.data), dict(my=maps.ctypes.data), dict(hc=1 << 16, wc=1 << 15), dict(hc=-4), dict(wc=-8),
            dict(tx=np.array([64.0, 0.0, 5.0])), dict(tx=np.array([64.0, -16.0, 5.0])), dict(tx=np.array([np.inf, 16.0, 5.0])),
            dict(ty=np.array([32.0, np.nan])), dict(ty=np.array([-0.0, 8.0]))]


def gray_bad(maps):
    """the bad arguments of ssamd_graycode_decode on 14 planes of 4 x 8, a 13 x 6 projector; ``maps`` a float32 [4, 8]"""
    return [dict(planes=None), dict(out=None), dict(h=-1), dict(x0=-1), dict(x0=1), dict(y0=1), dict(w=9), dict(n=12), dict(ncol=17, nrow=-10),
            dict(nrow=-1, ncol=8), dict(thr=-1), dict(thr=257), dict(pw=0), dict(ph=65537), dict(mx=maps.ctypes.data), dict(my=maps.ctypes.data),
            dict(hc=1 << 16, wc=1 << 15), dict(hc=-4)]


def label(kw, maps):
    """a bad argument as the key of the recorded messages: no address in it"""
    def value(v):
        if isinstance(v, np.ndarray):
            return repr(v.tolist())
        return "maps" if v == maps.ctypes.data else repr(v)
    return ", ".join("%s=%s" % (k, value(kw[k])) for k in sorted(kw))


class Calls:
    """the two decoders on valid defaults, one argument replaced at a time; -> (return code, ssamd_last_error())"""

    def __init__(self):
        from simplestereo_amd import _native
        self.lib = _native.lib()
        self.planes = np.zeros((20, 4, 8), np.uint8)
        self.out = np.zeros((4, 8, 3), np.float64)
        self.maps = np.zeros((4, 8), np.float32)

    def _done(self, rc):
        text = self.lib.ssamd_last_error()
        return rc, text.decode() if isinstance(text, bytes) else text

    def phase(self, route, **kw):
        dp = ctypes.POINTER(ctypes.c_double)
        a = dict(planes=self.planes.ctypes.data, n=20, hc=4, wc=8, mx=None, my=None, x0=0, y0=0, h=4, w=8, nx=3, ny=2, tx=np.array([64.0, 16.0, 5.0]),
                 ty=np.array([32.0, 8.0]), pw=64, ph=32, thr2=0, out=self.out.ctypes.data)
        a.update(kw)
        args = (a["planes"], a["n"], a["hc"], a["wc"], a["mx"], a["my"], a["x0"], a["y0"], a["h"], a["w"], a["nx"], a["ny"],
                None if a["tx"] is None else a["tx"].ctypes.data_as(dp), None if a["ty"] is None else a["ty"].ctypes.data_as(dp), a["pw"], a["ph"], a["thr2"], a["out"])
        return self._done(self.lib.ssamd_phaseshift_decode_device(*args, None) if route == "device" else self.lib.ssamd_phaseshift_decode(*args, -1))

    def gray(self, route, **kw):
        a = dict(planes=self.planes.ctypes.data, n=14, hc=4, wc=8, mx=None, my=None, x0=0, y0=0, h=4, w=8, ncol=4, nrow=3, pw=13, ph=6, thr=5, out=self.out.ctypes.data)
        a.update(kw)
        args = (a["planes"], a["n"], a["hc"], a["wc"], a["mx"], a["my"], a["x0"], a["y0"], a["h"], a["w"], a["ncol"], a["nrow"], a["pw"], a["ph"], a["thr"], a["out"], None)
        return self._done(self.lib.ssamd_graycode_decode_device(*args, None) if route == "device" else self.lib.ssamd_graycode_decode(*args, -1))

    def messages(self):
        """{"phaseshift" | "graycode": {route: {label: message}}} of the build that is loaded"""
        got = {}
        for name, call, bad in (("phaseshift", self.phase, phase_bad(self.maps)), ("graycode", self.gray, gray_bad(self.maps))):
            got[name] = {route: {label(kw, self.maps): call(route, **kw)[1] for kw in bad} for route in ROUTES}
        return got


def geometries(ss):
    """{rig: {"GrayCode" | "StructuredLightRig": hex of the 68 packed doubles}} on the rigs of phaseshift_cases.json"""
    import _graycode_ref as G
    import _phaseshift_ref as P
    got = {}
    for name, c in sorted(P.load()[0]["rigs"].items()):
        rig = G.make_rig(ss, c["rig"])
        got[name] = {"GrayCode": ss.active.GrayCode(rig)._geometry().tobytes().hex(), "StructuredLightRig": ss.StructuredLightRig(rig)._geometry().tobytes().hex()}
    return got


def front_inputs():
    """[(name, (mapx, mapy) | None, region (x, y, w, h))] on the 67 x 37 camera: what together takes every mode of the decoders' front
    and fails every condition of its window (tests/_graycode_ref.front says which)"""
    import _graycode_ref as G
    import _stereo_ftp_ref as S
    full = (0, 0, 67, 37)
    r = G.rig((67, 37), (13, 6), "none", dist1=[0.9, 0.3, 0.002, -0.003, 0.02])      # of test_decode_through_the_undistortion_maps
    und = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], (67, 37))
    holes = (und[0].copy(), und[1].copy())
    holes[0][10, 20], holes[1][12, 33], holes[0][30, 50] = np.nan, np.nan, np.nan
    holes[0][20, 29], holes[1][25, 40] = np.inf, np.inf
    yy, xx = np.mgrid[0:37, 0:67].astype(np.float32)
    reversed_columns = (np.ascontiguousarray(xx[:, ::-1]), yy)
    # (inside a row the reversed columns of four neighbours still span 3: they take the window, its shifts descending; a column
    # spread over 6 needs neighbours more than two columns apart)
    stretched = ((3 * xx) % 65, yy)
    return [("whole", None, full), ("roi", None, (3, 5, 64, 30)), ("undistortion", und, full), ("undistortion with holes", holes, full),
            ("reversed columns", reversed_columns, full), ("columns three apart", stretched, full)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_key(name, m):
    return "%s, min_modulation %s" % (name, m)


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _record(name, what):
    with open(os.path.join(GOLDEN, name), "w") as f:
        json.dump(what, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", name)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import simplestereo_amd
    if sys.argv[1] == "errors":
        _record("plane_stack_errors.json", Calls().messages())
    elif sys.argv[1] == "geometry":
        _record("plane_stack_geometry.json", geometries(simplestereo_amd))
    elif sys.argv[1] == "digests":
        import test_gpu_phaseshift as T
        got = {}
        for case in sorted(T.META["decode"]):
            c = T.META["decode"][case]
            stack, maps, _, _ = T._decode_case(case)
            for m in T.MODULATIONS:
                got[digest_key(case, m)] = digest(simplestereo_amd.active.phaseShiftDecode(stack, c["periods"], T.PROJ, maps=maps, roi=c["roi"], min_modulation=m))
        _record("phaseshift_parent_digests.json", got)
