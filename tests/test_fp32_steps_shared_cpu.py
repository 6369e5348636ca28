"""CPU tier, plain text: the fp32 steps the ASW kernel families share -- the Lab distance, the support weight, the truncated
absolute difference, the 8-disparity e pair -- are written once, in csrc/common.hip.h, and the unaligned pixel read once, in
csrc/lab_kernels.hip.h; no family grows a copy of its own again.  No GPU, no compiler.  (asw_exact_kernels.hip.h, the fp64
pass, is not on the list: it has its own weight function and reads the TAD where it needs the bytes.)"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplestereo_amd", "csrc")
FAMILIES = ["asw_kernels.hip.h", "asw_pipe_kernel.hip.h", "asw_wave_kernel.hip.h", "asw_wave6_kernel.hip.h", "asw_wave_front.inc",
            "asw_wave_row.inc", "asw_alt_kernels.hip.h", "asw_prepass_kernels.hip.h"]
UNALIGNED_TYPEDEF = r"typedef\s+\w+\s+__attribute__\s*\(\(\s*aligned\s*\(\s*1\s*\)\s*\)\)"
# in none of FAMILIES, in common.hip.h: regular expressions on the text without comments
COMMON_ONLY = {"v_sad_u8": r"__builtin_amdgcn_sad_u8", "v_sqrt_f32": r"__builtin_amdgcn_sqrtf",
               "a direct call of asw_weight_finish": r"\basw_weight_finish\s*\("}
HELPERS = ["asw_lab_dist2", "asw_support_weight", "asw_support_weights", "asw_tad", "asw_tad8"]


def _code(name):
    """the file without its comments (prose may name the functions)"""
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def test_no_kernel_family_holds_a_shared_step_itself():
    for name in FAMILIES:
        code = _code(name)
        for what, rx in dict(COMMON_ONLY, **{"an unaligned-read typedef": UNALIGNED_TYPEDEF}).items():
            m = re.search(rx, code)
            assert m is None, f"{name}: {what} -- it belongs in common.hip.h / lab_kernels.hip.h: {m.group(0)}"


def test_common_holds_each_step_and_its_helpers_once():
    code = _code("common.hip.h")
    for what, rx in COMMON_ONLY.items():
        assert re.search(rx, code), what
    for fn in HELPERS:
        assert len(re.findall(r"__forceinline__\s+\w+\s+%s\s*\(" % fn, code)) >= 1, fn
    # one definition of the arithmetic: the builtins appear where the helpers are defined and nowhere else in the file
    assert len(re.findall(COMMON_ONLY["v_sad_u8"], code)) == 1
    assert len(re.findall(r"fmaf\s*\(\s*db\s*,\s*db", code)) == 1
    assert "asw_alt_weight" not in "".join(_code(n) for n in os.listdir(CSRC))


def test_every_family_builds_its_weights_and_differences_through_the_helpers():
    used = {n: [fn for fn in HELPERS if re.search(r"\b%s\s*\(" % fn, _code(n))] for n in FAMILIES}
    assert {"asw_lab_dist2", "asw_support_weights", "asw_tad8"} <= set(used["asw_kernels.hip.h"]), used
    assert {"asw_lab_dist2", "asw_support_weights", "asw_tad8"} <= set(used["asw_pipe_kernel.hip.h"]), used
    assert "asw_support_weight" in used["asw_wave_front.inc"], used
    assert {"asw_support_weight", "asw_tad"} <= set(used["asw_alt_kernels.hip.h"]), used
    assert "asw_tad" in used["asw_prepass_kernels.hip.h"], used


def test_the_unaligned_pixel_read_occurs_once_under_csrc():
    """`uint8 [n][3]` pixel p as one 4-byte read at byte 3 p: load_bgr of lab_kernels.hip.h, and every other reader calls it"""
    where = []
    for name in sorted(os.listdir(CSRC)):
        code = _code(name)
        # a 4-byte unaligned read whose address is a multiple of 3 bytes into an image
        where += [name] * len(re.findall(r"u32_unaligned\s*\*\s*>\s*\(\s*[^;]*\b3\s*\*", code))
        where += [name] * len(re.findall(r"const\s+uint8_t\s*\*\s*const\s+b\s*=[^;]*\b3\s*\*[^;]*;[^}]*u32_unaligned\s*\*\s*>\s*\(\s*b\s*\)", code))
    assert where == ["lab_kernels.hip.h"], where
    for name in ("asw_prepass_kernels.hip.h", "gsw_kernels.hip.h", "lab_kernels.hip.h"):
        assert re.search(r"\bload_bgr\s*\(", _code(name)), name
    for name in ("asw_prepass_kernels.hip.h", "rig_kernels.hip.h", "lab_kernels.hip.h"):
        assert re.search(r"\blab_record(s_pair)?\s*\(", _code(name)), name
    assert len(re.findall(r"\bbgr_to_lab\s*\(", "".join(_code(n) for n in os.listdir(CSRC)))) == 2       # its definition, and lab_record
