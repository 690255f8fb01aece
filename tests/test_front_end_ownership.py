"""The roadmap, tree and map-preprocessing front ends follow the ownership rule stated at the top of csrc/device_scratch.h:
device and pinned memory lives in DeviceScratch / DeviceBuffer / PinnedBuffer, never in a bare allocation call, and a HIP
call's result goes through HIP_TRY, never into a comparison of the front end's own.  Plain text checks of the sources."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "art_planner_amd", "csrc")


def _code(header):
    with open(os.path.join(CSRC, header)) as f:
        return f.read()


@pytest.mark.parametrize("header", ["roadmap.h", "roadmap_many.h", "preprocess.h", "tree.h"])
def test_no_bare_allocation_calls(header):
    calls = re.findall(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(", _code(header))
    assert calls == [], (header, calls)


@pytest.mark.parametrize("header", ["roadmap.h", "preprocess.h"])
def test_one_error_style(header):
    code = _code(header)
    assert re.search(r"\bokk\b", code) is None, header
    # `call(...) == hipSuccess`, `hipSuccess != call(...)`, in any spacing
    compared = re.findall(r"[=!]=\s*hipSuccess\b|\bhipSuccess\s*[=!]=", code)
    assert compared == [], (header, compared)
    assert "HIP_TRY(" in code and "ARTP_TRY(" in code, header
