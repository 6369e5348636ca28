"""The ASW kernel forms as the tests force them: the catalogue of option sets with what the planner must then say, the one
place that asks it, the raw cost dump and the bit-for-bit comparison of two dumps.  Helper module, not a test.

A form is a pair (opts, expect): SSAMD_* options, and the values (or predicates) that ssamd_asw_kernel_form and
ssamd_asw_geometry must report under them for the call's shape.  `forced` sets the options, asks, and fails with the whole plan
if the form would not run.  Both queries are host-side: tests/test_asw_forms_cpu.py puts every row of the GPU tests -- their
forced_rows(), each (form, W, H, params) -- through them without a device.  None of the options is SSAMD_ASW_COST_KEYS's
business: the cost-image hook forces no form."""
import contextlib

import numpy as np
from simplestereo_amd import _native


def planned(W, rows, p):
    """what the planner runs for a call's shape and parameters (StereoASW's keyword names): the thirteen keys of the two queries"""
    a = (W, rows, p["winSize"], p["maxDisparity"], p.get("minDisparity", 0))
    return dict(_native.asw_kernel_form(*a), **_native.asw_geometry(*a))


class FormMismatch(AssertionError):
    """the planner does not run the forced form; .key is the first key of the expectation that it misses"""

    def __init__(self, form, key, want, plan, p):
        AssertionError.__init__(self, "the form did not run", form, key, plan[key], "a predicate" if callable(want) else want, plan, p)
        self.key, self.planned = key, plan


@contextlib.contextmanager
def forced(form, W, rows, p, expect=None):
    """the form's options set for the block, after the planner has said that its expectation (and `expect`) holds: yields the
    plan.  `form` is a builder's pair, a name of FORMS, or bare options, which need `expect` unless they are empty."""
    opts, own = FORMS[form] if isinstance(form, str) else (form, {}) if isinstance(form, dict) else form
    assert expect is not None or not (isinstance(form, dict) and form), ("forced options have to say what must run", form)
    with _native.options(**opts):
        f = planned(W, rows, p)
        for k, v in dict(own, **(expect or {})).items():
            if not (v(f[k]) if callable(v) else f[k] == v):
                raise FormMismatch(form, k, v, f, p)
        yield f


def also(form, **expect):
    """a form held to more than its builder derives (the number of chunks, the grid: what a test's shape adds)"""
    return form[0], dict(form[1], **expect)


# ---- builders of the parametrised families: (opts, expect) from the tile ---------------------------------------------------------
def _geom(geom):
    v = [int(s) for s in geom.split(",")]
    return v + [0, 8][len(v) - 2:]


def tile(geom, **extra):
    """the tile SSAMD_ASW_GEOM = "XG,DG[,JC[,RX]]" -- XG groups of RX (8 or 4) columns, DG groups of 4 disparities -- on whichever of
    the two workgroup-wide kernels the planner then takes"""
    XG, DG, _, RX = _geom(geom)
    return dict(SSAMD_ASW_GEOM=geom, **extra), dict(wave_kernel=0, tile_columns=RX, tile_x=RX * XG, chunk_d=4 * DG)


def workgroup_tile(geom, win=None, **extra):
    """asw_aggregate_kernel on that tile, with tap-column chunks of JC (whole window rows for 0, and for a JC that is no shorter than
    the window `win`, if that is given)"""
    JC, RX = _geom(geom)[2:]
    whole = JC % RX or (win is not None and JC >= win)
    return also(tile(geom, SSAMD_ASW_WAVE="0", SSAMD_ASW_PIPE="0", **extra), phase_shifted=0, chunk_columns=0 if whole else JC)


def pipe_tile(XG, DG, JC, dephase=None, static=None, persist=None, **extra):
    """asw_aggregate_pipe_kernel on a tile of 8 XG columns x 4 DG disparities with tap-column chunks of JC; the wave order
    (SSAMD_ASW_DEPHASE), the compile-time strides (SSAMD_ASW_STATIC) and the persistent form's workers (SSAMD_ASW_PERSIST) where given"""
    given = dict(SSAMD_ASW_DEPHASE=dephase, SSAMD_ASW_STATIC=static, SSAMD_ASW_PERSIST=persist)
    extra.update((k, str(v)) for k, v in given.items() if v is not None)
    form = also(tile("%d,%d,0,8" % (XG, DG), SSAMD_ASW_WAVE="0", SSAMD_ASW_PIPE=str(JC), **extra), phase_shifted=1, chunk_columns=JC)
    return form if dephase is None else also(form, build_first_waves=int(dephase))


def wave(rx, **extra):
    """asw_aggregate_wave_kernel on its rx-column register tile (8 or 4); SSAMD_ASW_WAVE_MERGE, _WG, _UNROLL and _RD among `extra`
    (None: left unset): WG waves make a workgroup, RD = 4 leaves the six-per-lane kernel for groups of four"""
    extra = {k: v for k, v in extra.items() if v is not None}
    expect = dict(wave_kernel=int(rx), phase_shifted=0, tile_columns=int(rx))
    if "SSAMD_ASW_WAVE_WG" in extra:
        expect["threads"] = 64 * int(extra["SSAMD_ASW_WAVE_WG"])
    if extra.get("SSAMD_ASW_WAVE_RD") == "4":
        expect["chunk_d"] = lambda d: d % 4 == 0
    return dict(SSAMD_ASW_WAVE="1", SSAMD_ASW_WAVE_RX=str(rx), **extra), expect


# the workgroup kernels, whichever the planner then picks: the standard the wave kernel's maps and costs are held to
NO_WAVE = (dict(SSAMD_ASW_WAVE="0"), dict(wave_kernel=0))

# ---- the named forms (tests/golden/asw_band_cases.json lists them per case) ----------------------------------------------------------
_PIPE = dict(phase_shifted=1, wave_kernel=0)
FORMS = {
    "planner": (dict(SSAMD_AUTOTUNE="0"), dict()),
    "wave4": wave(4),
    "wave8": wave(8),
    "wave6": also(wave(4), chunk_d=18),
    "wave4x5": also(wave(4, SSAMD_ASW_WAVE_RD="4"), chunk_d=20),
    "pipe": (dict(SSAMD_ASW_WAVE="0", SSAMD_AUTOTUNE="0"), _PIPE),
    "pipe_evol0": (dict(SSAMD_ASW_WAVE="0", SSAMD_ASW_EVOL="0"), _PIPE),
    "pipe8": (dict(SSAMD_ASW_WAVE="0", SSAMD_ASW_PIPE="8"), dict(_PIPE, chunk_columns=8)),
    "pipe8_evol0": (dict(SSAMD_ASW_WAVE="0", SSAMD_ASW_PIPE="8", SSAMD_ASW_EVOL="0"), dict(_PIPE, chunk_columns=8)),
    "workgroup": (dict(SSAMD_ASW_WAVE="0", SSAMD_ASW_PIPE="0"), dict(phase_shifted=0, wave_kernel=0)),
    "chunks": (dict(SSAMD_AUTOTUNE="0"), dict(n_chunks=lambda n: n > 1)),
}

# (XG, DG, JC) of the phase-shifted kernel's tiles that tests/test_gpu_pipe_build.py and tests/test_gpu_pipe_persist.py run
PIPE_TILES = {"120x196": (15, 49, 16), "216x68": (27, 17, 16), "88x260": (11, 65, 16), "48x36": (6, 9, 8), "120x100": (15, 25, 16)}


# ---- the raw cost dump ----------------------------------------------------------------------------------------------------------------
def cost_dump(L, R, p, keys=False):
    """ssamd_asw_costs: the aggregated fp32 costs [H, W, nD] of the form in force (NaN where a candidate does not exist); with
    `keys` the 32-bit cost images of asw_cost_key instead, as bit patterns in the float32 array (test hook SSAMD_ASW_COST_KEYS)"""
    H, W = L.shape[:2]
    mind = p.get("minDisparity", 0)
    c = np.empty((H, W, p["maxDisparity"] - mind + 1), np.float32)
    with _native.options(**(dict(SSAMD_ASW_COST_KEYS="1") if keys else {})):
        _native.check(_native.lib().ssamd_asw_costs(L.ctypes.data, R.ctypes.data, H, W, p["winSize"], p["maxDisparity"], mind,
                                                    float(p.get("gammaC", 5.0)), float(p.get("gammaP", 17.5)), c.ctypes.data, -1))
    return c


def same_costs(got, want):
    """bit for bit: the number of words of two float dumps that differ -- in whether they are NaN (a candidate that does not exist),
    or, where neither is, in their 32 bits"""
    nan, got_nan = np.isnan(want), np.isnan(got)
    return int(np.count_nonzero(np.where(nan | got_nan, nan != got_nan, got.view(np.uint32) != want.view(np.uint32))))


class counted:
    """``with counted("tail_splits") as n: ...``: n.delta is the growth of the device context's counter since the block began, and
    stays what it was when the block ended"""

    def __init__(self, name):
        self.name, self._end = name, None

    def __enter__(self):
        self._start = _native.counter(self.name)
        return self

    def __exit__(self, *exc):
        self._end = _native.counter(self.name)

    @property
    def delta(self):
        return (_native.counter(self.name) if self._end is None else self._end) - self._start
