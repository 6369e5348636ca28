"""CPU tier of ss.active.GrayCode: the numpy restatement tests/_graycode_ref.py against itself (pattern -> decode round trip, the
literal and the vectorised getProjPixel), ``grayCodePattern`` against it, the third public header include/ssamd_graycode.h against
its ctypes rows (with the two older headers unchanged), the host-side geometry, the roi reading and the exceptions.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _graycode_ref as G
import _plane_stack as X
from test_native_signatures_cpu import SCALARS, _is_pointer_class, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


# ------------------------------------------------------------------------------------------------ the restatement
def test_bit_counts_are_opencvs_formula(ss):
    sizes = (1, 2, 3, 5, 720, 1024, 1080, 1280, 1920, 4096, 65535, 65536)
    assert [G.num_bits(v) for v in sizes] == [0, 1, 2, 3, 10, 10, 11, 11, 11, 12, 16, 16]
    assert [G.num_bits(2 ** k) for k in range(17)] == list(range(17))
    assert [ss.active._gray_bits(v) for v in sizes] == [G.num_bits(v) for v in sizes]
    assert G.num_patterns(1920, 1080) == 44 and G.num_patterns(1, 1) == 0 and G.num_patterns(65536, 65536) == 64


@pytest.mark.parametrize("res", [(1, 1), (2, 1), (5, 3), (13, 6), (1024, 768), (1280, 720)])
def test_decode_of_the_pattern_returns_every_projector_pixel(res):
    w, h = res
    pat = G.pattern(w, h)
    assert pat.shape == (G.num_patterns(w, h), h, w) and pat.dtype == np.uint8
    got = G.decode(pat, w, h, 5, shape=(h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(got[..., 0], xx) and np.array_equal(got[..., 1], yy)
    assert np.array_equal(pat[0::2], 255 - pat[1::2])


def test_literal_and_vectorised_getprojpixel_agree():
    stack = G.random_stack(11, 14, 7, 9)
    for thr in (0, 1, 5, 256):
        lit = G.decode_literal(list(stack), 13, 6, thr)
        vec = G.decode(stack, 13, 6, thr)
        assert np.array_equal(lit, vec)
        if thr == 5:
            valid = vec[..., 0] >= 0
            assert 0 < valid.sum() < valid.size                               # a mix
    assert G.gray_to_dec([]) == 0 and G.gray_to_dec([1, 0, 0]) == 7 and G.gray_to_dec([1, 1, 0]) == 4


def test_render_is_decoded_back():
    rng = np.random.default_rng(3)
    px, py = rng.integers(0, 13, (7, 9)), rng.integers(0, 6, (7, 9))
    got = G.decode(G.render(px, py, 13, 6, 40, extra=2), 13, 6, 5)
    assert np.array_equal(got[..., 0], px) and np.array_equal(got[..., 1], py)


@pytest.mark.parametrize("res", [(1, 1), (2, 1), (5, 3), (13, 6), (320, 200)])
def test_pattern_equals_the_restatement(ss, res):
    got = ss.active.grayCodePattern(res)
    assert got.dtype == np.uint8 and np.array_equal(got, G.pattern(*res))


def test_generate_writes_the_reference_files(ss, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    target = str(tmp_path / "codes")
    assert ss.active.generateGrayCodeImgs(target, (13, 6)) == 14
    assert sorted(os.listdir(target)) == sorted([str(i) + ".png" for i in range(14)] + ["black.png", "white.png"])
    pat = G.pattern(13, 6)
    for i in range(14):
        with Image.open(os.path.join(target, "%d.png" % i)) as im:
            assert im.mode == "L" and np.array_equal(np.array(im), pat[i])
    with Image.open(os.path.join(target, "white.png")) as im:
        assert np.array_equal(np.array(im), np.full((6, 13), 255, np.uint8))
    with Image.open(os.path.join(target, "black.png")) as im:
        assert not np.array(im).any()


# ------------------------------------------------------------------------------------------------ the third header
@pytest.fixture(scope="module")
def graycode_header():
    with open(os.path.join(ROOT, "include", "ssamd_graycode.h")) as f:
        return f.read()


def test_graycode_header_parses_and_matches_its_ctypes_rows(graycode_header):
    from simplestereo_amd import _native
    protos = _prototypes(graycode_header)
    assert sorted(protos) == ["ssamd_graycode_cloud", "ssamd_graycode_cloud_device", "ssamd_graycode_decode", "ssamd_graycode_decode_device",
                              "ssamd_graycode_offsets", "ssamd_graycode_offsets_device"]
    assert set(protos) == set(re.findall(r"\b(ssamd_[a-z0-9_]+)\s*\(", graycode_header))
    assert int(re.search(r"#define SSAMD_GRAYCODE_VERSION (\d+)", graycode_header).group(1)) == _native.GRAYCODE_VERSION == 1
    assert int(re.search(r"#define SSAMD_GRAYCODE_BLOCK (\d+)", graycode_header).group(1)) == _native.GRAYCODE_BLOCK
    assert protos["ssamd_graycode_decode"] == ("int", ["ptr", "int", "int", "int", "ptr", "ptr"] + ["int"] * 9 + ["ptr", "ptr", "int"])
    assert protos["ssamd_graycode_offsets_device"] == ("int", ["ptr", "int", "ptr", "ptr"])
    assert protos["ssamd_graycode_cloud_device"] == ("int", ["ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr", "ptr"])
    lib = _native.lib()
    for name, (ret, kinds) in protos.items():
        fn = getattr(lib, name)                                                 # exported from the same library
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            assert _is_pointer_class(t) if kind == "ptr" else t is SCALARS[kind], (name, i, t, kind)


def test_the_older_headers_do_not_know_graycode():
    for name, count in (("ssamd.h", 54), ("ssamd_active.h", 4)):
        with open(os.path.join(ROOT, "include", name)) as f:
            header = f.read()
        assert "graycode" not in header.lower()
        assert len(_prototypes(header)) == count


def test_abi_argument_errors_need_no_device():
    """SSAMD_EINVAL for what include/ssamd_graycode.h lists, decided before any device is looked for"""
    from simplestereo_amd import _native
    lib = _native.lib()
    planes = np.zeros((14, 4, 8), np.uint8)
    out = np.zeros((4, 8, 2), np.int32)
    maps = np.zeros((4, 8), np.float32)
    geom = np.ones(68)

    def decode(planes=planes.ctypes.data, n=14, hc=4, wc=8, mx=None, my=None, x0=0, y0=0, h=4, w=8, ncol=4, nrow=3, pw=13, ph=6, thr=5,
               out=out.ctypes.data):
        return lib.ssamd_graycode_decode(planes, n, hc, wc, mx, my, x0, y0, h, w, ncol, nrow, pw, ph, thr, out, None, -1)

    bad = X.gray_bad(maps)
    for kw in bad:
        assert decode(**kw) == _native.EINVAL, kw
        assert lib.ssamd_last_error()
    assert decode(h=0) == 0 and decode(w=0, planes=None, out=None) == 0                  # an empty region does nothing
    n = ctypes.c_int(7)
    gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def cloud(geom=gp, out=out.ctypes.data, npoints=ctypes.byref(n), h=4, **kw):
        a = dict(planes=planes.ctypes.data, n=14, hc=4, wc=8, mx=None, my=None, x0=0, y0=0, w=8, ncol=4, nrow=3, pw=13, ph=6, thr=5)
        a.update(kw)
        return lib.ssamd_graycode_cloud(a["planes"], a["n"], a["hc"], a["wc"], a["mx"], a["my"], a["x0"], a["y0"], h, a["w"], a["ncol"], a["nrow"],
                                        a["pw"], a["ph"], a["thr"], geom, 0, out, npoints, -1)

    assert cloud(geom=None) == _native.EINVAL and cloud(out=None) == _native.EINVAL and cloud(npoints=None) == _native.EINVAL
    assert cloud(thr=300) == _native.EINVAL and cloud(n=10) == _native.EINVAL
    for i in (12, 36, 40, 67):
        g = geom.copy()
        g[i] = np.inf
        assert cloud(geom=g.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == _native.EINVAL, i
    assert cloud(h=0) == 0 and n.value == 0
    assert lib.ssamd_graycode_offsets(None, 3, out.ctypes.data, -1) == _native.EINVAL
    assert lib.ssamd_graycode_offsets(out.ctypes.data, -1, out.ctypes.data, -1) == _native.EINVAL
    assert lib.ssamd_graycode_offsets(out.ctypes.data, (1 << 21) + 1, out.ctypes.data, -1) == _native.EINVAL
    assert lib.ssamd_graycode_offsets_device(out.ctypes.data, 2, None, None) == _native.EINVAL
    assert lib.ssamd_graycode_cloud_device(out.ctypes.data, 1 << 16, 1 << 15, 0, 0, gp, None, out.ctypes.data, None) == _native.EINVAL


# ------------------------------------------------------------------------------------------------ the host side of GrayCode
RIGS = {"d5": G.rig((67, 37), (13, 6), "d5"), "none_dist": G.rig((40, 30), (1280, 720), None),
        "t2_zero": G.rig((48, 32), (64, 32), "none", T=(-200.0, 0.0, 0.0), R=np.eye(3),
                         K1=[[1024.0, 0, 24.0], [0, 1024.0, 16.0], [0, 0, 1]], K2=[[1024.0, 0, 24.0], [0, 1024.0, 16.0], [0, 0, 1]]),
        "d12_camera_dist": G.rig((67, 37), (1280, 720), "d12", dist1=[-0.2, 0.08, 0.001, -0.002, 0.01])}


@pytest.mark.parametrize("name", sorted(RIGS))
def test_attributes_geometry_and_maps_equal_the_restatement(ss, name):
    import _stereo_ftp_ref as S
    r = RIGS[name]
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    assert ss.active.GrayCodeSingle is ss.active.GrayCode and not hasattr(gc, "graycode")
    assert gc.num_patterns == G.num_patterns(*r["res2"]) and gc.rig.res2 == tuple(r["res2"])
    want = G.geometry(r)
    got = gc._geometry()
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(gc.Rectify1.ravel(), want[40:49]) and np.array_equal(gc.Rectify2.ravel(), want[49:58])
    assert gc.R_inv.shape == (4, 4) and np.array_equal(gc.R_inv[:3, :3].ravel(), want[58:67]) and gc.R_inv[3].tolist() == [0, 0, 0, 1]
    mx, my = gc._maps()
    wx, wy = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], tuple(r["res1"]))
    assert mx.dtype == np.float32 and np.array_equal(mx, wx) and np.array_equal(my, wy)
    if r["T"][2] != 0:                                                           # StereoFTP builds its maps through the same function
        fringe = S.build_fringe(12.0, dims=(64, 8), stripeColor="r")
        sx, sy = ss.active.StereoFTP(gc.rig, fringe, 12.0)._host_maps()
        assert np.array_equal(sx, mx) and np.array_equal(sy, my)


def test_roi_is_read_as_the_reference_loops_read_it(ss):
    f = ss.active._gray_roi
    assert f(None, (67, 37)) == (0, 0, 67, 37)
    assert f((3, 5, 20, 9), (67, 37)) == (3, 5, 17, 4)                          # range(5, 9) x range(3, 20)
    assert f((0, 0, 67, 37), (67, 37)) == (0, 0, 67, 37)
    assert f((10, 5, 10, 30), (67, 37))[2:] == (0, 25) and f((10, 5, 4, 3), (67, 37))[2:] == (0, 0)      # empty ranges
    assert f((10, 40, 500, 3), (67, 37))[2:] == (490, 0)                        # no row: the reference reads nothing
    for bad in ((0, 0, 68, 37), (0, 0, 67, 38), (-1, 0, 5, 5), (0, -2, 5, 5), (0, 0, 5), (0, 0, 5.0, 5), (0, 0, True, 5), 7):
        with pytest.raises(ValueError):
            f(bad, (67, 37))


def test_empty_regions_and_empty_stacks_need_no_device(ss):
    r = RIGS["d5"]
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    stack = G.random_stack(1, 14, 37, 67)
    pts = gc.getCloud(stack, roi=(5, 5, 5, 30))
    assert pts.shape == (0, 1, 3) and pts.dtype == np.float64
    assert gc.getCloud(stack, roi=(5, 9, 30, 9), dense=True).shape == (0, 25, 3)
    d = ss.active.grayCodeDecode(stack, (13, 6), roi=(7, 3, 7, 20))
    assert d.shape == (17, 0, 2) and d.dtype == np.int32


# ------------------------------------------------------------------------------------------------ exceptions
def test_exceptions_are_raised_before_any_native_call(ss, monkeypatch, tmp_path):
    a = ss.active
    assert {"grayCodePattern", "generateGrayCodeImgs", "grayCodeDecode", "GrayCode", "GrayCodeSingle"} <= set(a.__all__)
    assert "GrayCodeDouble" in a.__doc__ and not hasattr(a, "GrayCodeDouble") and "and Gray code are not here" not in a.__doc__

    def no_native(*args, **kw):
        raise AssertionError("a native call")
    monkeypatch.setattr(a._native, "lib", no_native)
    r = RIGS["d5"]
    rig = G.make_rig(ss, r)
    gc = a.GrayCode(rig)
    stack = G.random_stack(1, 14, 37, 67)
    # resolutions
    for bad in ((0, 5), (5, 65537), (5,), (5.0, 3), (True, 3), 7, "ab"):
        with pytest.raises(ValueError):
            a.grayCodePattern(bad)
        with pytest.raises(ValueError):
            a.grayCodeDecode(stack, bad)
    with pytest.raises(ValueError):
        a.generateGrayCodeImgs(str(tmp_path / "x"), (0, 0))
    big = G.make_rig(ss, dict(r, res2=[65537, 6]))
    with pytest.raises(ValueError):
        a.GrayCode(big)
    # images
    for bad in (stack.astype(np.float32), [stack[0].astype(np.uint16)], "name.png", 5, {"a": 1}, [[1, 2], [3, 4]]):
        with pytest.raises(TypeError):
            a.grayCodeDecode(bad, (13, 6))
        with pytest.raises(TypeError):
            gc.getCloud(bad)
    for bad in (stack[0], stack[None], [stack[0][None]], [stack[0], stack[1][:, :-1]]):
        with pytest.raises(ValueError):
            a.grayCodeDecode(bad, (13, 6))
    with pytest.raises(ValueError, match="needs 14 pattern images, got 13"):
        a.grayCodeDecode(stack[:13], (13, 6))
    with pytest.raises(ValueError, match="needs 14 pattern images, got 2"):
        gc.getCloud(list(stack[:2]))
    # thresholds
    for bad in (-1, 257, 5.0, "5", None, True):
        with pytest.raises(ValueError, match="white_thr"):
            a.grayCodeDecode(stack, (13, 6), white_thr=bad)
        with pytest.raises(ValueError, match="white_thr"):
            a.GrayCode(rig, white_thr=bad)
    assert a.GrayCode(rig, black_thr=77, white_thr=256).black_thr == 77
    # maps
    m = np.zeros((37, 67), np.float32)
    for bad in (m, (m,), (m, m, m), (m, m[:-1]), (m[:, :-1], m)):
        with pytest.raises(ValueError):
            a.grayCodeDecode(stack, (13, 6), maps=bad)
    for bad in ((m, m.astype(np.float64)), (m.tolist(), m), (m, None)):
        with pytest.raises(TypeError):
            a.grayCodeDecode(stack, (13, 6), maps=bad)
    # roi
    for bad in ((0, 0, 68, 37), (-1, 0, 5, 5), (0, 0, 5), (0, 0, 5.5, 5)):
        with pytest.raises(ValueError):
            a.grayCodeDecode(stack, (13, 6), roi=bad)
        with pytest.raises(ValueError):
            gc.getCloud(stack, roi=bad)
    # getCloud: sizes, in the reference's words
    with pytest.raises(ValueError, match="Image size of 0 is mismatch!"):
        gc.getCloud(stack[:, :-1])
    with pytest.raises(ValueError, match="Image size of 3 is mismatch!"):
        gc.getCloud([stack[0], stack[1], stack[2], stack[3][:, :-1]] + list(stack[4:]))
    # a tilted projector sensor
    tilted = a.GrayCode(G.make_rig(ss, dict(r, distCoeffs2=[0.0] * 12 + [0.01, 0.0])))
    with pytest.raises(NotImplementedError):
        tilted.getCloud(stack)


def test_paths_must_be_8_bit_gray_files_of_res1(ss, monkeypatch, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = ss.active
    r = RIGS["d5"]
    gc = a.GrayCode(G.make_rig(ss, r))
    stack = G.random_stack(1, 14, 37, 67)
    paths = []
    for i in range(14):
        paths.append(str(tmp_path / ("%d.png" % i)))
        Image.fromarray(stack[i]).save(paths[-1])
    rgb = str(tmp_path / "rgb.png")
    Image.fromarray(np.zeros((37, 67, 3), np.uint8)).save(rgb)
    small = str(tmp_path / "small.png")
    Image.fromarray(np.zeros((36, 67), np.uint8)).save(small)
    deep = str(tmp_path / "deep.png")
    Image.fromarray(np.zeros((37, 67), np.uint16)).save(deep)

    def no_native(*args, **kw):
        raise AssertionError("a native call")
    monkeypatch.setattr(a._native, "lib", no_native)
    with pytest.raises(ValueError, match="pass arrays"):
        gc.getCloud([rgb] + paths[1:])
    with pytest.raises(ValueError, match="pass arrays"):
        gc.getCloud(paths[:5] + [deep] + paths[6:])
    with pytest.raises(ValueError, match=re.escape("Image size of %s is mismatch!" % small)):
        gc.getCloud(paths[:2] + [small] + paths[3:])
    with pytest.raises(ValueError, match="needs 14 pattern images"):
        gc.getCloud(paths[:13])
    assert [np.array_equal(p, s) for p, s in zip(gc._load(paths + [rgb], (67, 37)), stack)] == [True] * 14      # extra files are not opened
    monkeypatch.setitem(__import__("sys").modules, "PIL", None)
    with pytest.raises(ImportError, match="PIL"):
        gc.getCloud(paths)
    with pytest.raises(ImportError, match="PIL"):
        a.generateGrayCodeImgs(str(tmp_path / "y"), (13, 6))
