"""CPU tier, plain text: the four ASW aggregation kernels share ONE epilogue (csrc/asw_epilogue.inc) and none of them grows a
copy of its own again.  No GPU, no compiler."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplestereo_amd", "csrc")
EPILOGUE = "asw_epilogue.inc"
KERNEL_HEADERS = ["asw_kernels.hip.h", "asw_pipe_kernel.hip.h", "asw_wave_kernel.hip.h", "asw_wave6_kernel.hip.h"]
SHARED = "asw_shared.hip.h"          # what the four and the epilogue share (asw_cost_key's definition among it): no kernel, no epilogue
CALLS = ["asw_exact_select<", "asw_exact_merge<", "asw_cost_key("]


def _code(name):
    """the file without its comments (prose may name the functions)"""
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def test_each_kernel_includes_the_epilogue_once_and_calls_nothing_of_it_itself():
    for name in KERNEL_HEADERS:
        code = _code(name)
        assert len(re.findall(r'#include\s+"%s"' % re.escape(EPILOGUE), code)) == 1, name
        for line in code.splitlines():
            for call in CALLS:
                assert call not in line, f"{name}: own call of {call} -- it belongs in {EPILOGUE}: {line.strip()}"


def test_the_epilogue_holds_the_calls_and_is_the_only_file_that_merges():
    code = _code(EPILOGUE)
    for call in CALLS:
        assert call in code, call
    assert EPILOGUE not in _code(SHARED)
    holders = [f for f in sorted(os.listdir(CSRC)) if "asw_exact_merge<true>" in open(os.path.join(CSRC, f)).read()]
    assert holders == [EPILOGUE]
