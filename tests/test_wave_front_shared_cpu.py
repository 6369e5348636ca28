"""CPU tier, plain text: the two wave kernels share ONE front half (csrc/asw_wave_front.inc) and ONE row-staging block
(csrc/asw_wave_row.inc), neither grows a copy of its own again, and no compile-time experiment switch comes back into csrc/.
No GPU, no compiler."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplestereo_amd", "csrc")
SHARED = ["asw_wave_front.inc", "asw_wave_row.inc"]
WAVE_HEADERS = ["asw_wave_kernel.hip.h", "asw_wave6_kernel.hip.h"]
# what only the shared text does: LDS-DMA of the e tile, the support weight (common.hip.h's helper: the square root and
# asw_weight_finish behind it are in neither the kernels nor the shared text, tests/test_fp32_steps_shared_cpu.py), the tap offsets
# of the merged build
SHARED_ONLY = ["__builtin_amdgcn_global_load_lds", "asw_support_weight(", "tapoff["]
# names a preprocessor conditional may test: the ones the build itself defines (simplestereo_amd/build.py, the translation units,
# the compiler).  A compile-time variant of a kernel is a source tree of its own (tools/ab_tree.py), not an #ifdef.
CONDITIONAL_NAMES = {"SSAMD_PIPE_INSTANCE", "SSAMD_WAVE6_INSTANCE", "GM_HOST_TABLES", "__HIPCC__", "__HIP_DEVICE_COMPILE__"}


def _code(name):
    """the file without its comments (prose may name the functions)"""
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def test_each_wave_kernel_includes_the_shared_text_once_and_holds_none_of_it_itself():
    for name in WAVE_HEADERS:
        code = _code(name)
        for inc in SHARED:
            assert len(re.findall(r'#include\s+"%s"' % re.escape(inc), code)) == 1, (name, inc)
        for line in code.splitlines():
            for what in SHARED_ONLY:
                assert what not in line, f"{name}: own use of {what} -- it belongs in {' / '.join(SHARED)}: {line.strip()}"


def test_the_shared_text_holds_what_the_kernels_may_not():
    code = "".join(_code(inc) for inc in SHARED)
    for what in SHARED_ONLY:
        assert what in code, what
    assert "build_merged" in _code(SHARED[0])
    for name in WAVE_HEADERS:
        assert "build_merged(" in _code(name), name


def test_preprocessor_conditionals_test_only_names_the_build_defines():
    seen = set()
    for name in sorted(os.listdir(CSRC)):
        code = _code(name).replace("\\\n", " ")
        for m in re.finditer(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b([^\n]*)", code, flags=re.M):
            names = set(re.findall(r"[A-Za-z_]\w*", m.group(2))) - {"defined"}
            assert names, f"{name}: conditional without a name: {m.group(0).strip()}"
            assert names <= CONDITIONAL_NAMES, f"{name}: compile-time switch {sorted(names - CONDITIONAL_NAMES)}: {m.group(0).strip()}"
            seen |= names
    assert seen == CONDITIONAL_NAMES          # the list holds no name that is gone
