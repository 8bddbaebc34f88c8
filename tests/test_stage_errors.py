"""A HIP failure inside a stage file reaches `glh_last_error()`.

Every stage export validates in glimpse_hip.hip and runs in a translation unit of its own (tests/stage_calls.py lists
them); the message of a HIP call that fails there is kept by `glh::fail` (csrc/glh_stage.h), which glimpse_hip.hip defines.
Where no device is present the first HIP call of a valid job fails, so each export must return GLH_E_HIP with that call,
the runtime's words and the stage file's own name and line in the message.  Skipped where a device is present: there the
calls succeed (tests/test_gpu_stage_times.py).
"""
import re

import pytest

from tests import stage_calls

GLH_E_HIP = -2


def _no_device():
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    try:
        return _lib.device_count() < 1
    except _lib.GlhError:
        return True


@pytest.mark.parametrize("stage", list(stage_calls.STAGES))
def test_a_failed_hip_call_is_reported_from_every_stage_file(stage):
    from glimpse_amd import _lib

    if not _no_device():
        pytest.skip("a device is present: the HIP calls succeed")
    # the smallest legal input: 2 x 2 cells (a gradient needs two each way), one heading, a window and a Gaussian of one cell
    call = stage_calls.calls(nx=2, ny=2, headings=1, window=1, radius=0)[stage]
    with pytest.raises(_lib.GlhError) as info:
        call(False)
    message = _lib.load().glh_last_error().decode()
    print(stage, info.value.code, message)
    assert info.value.code == GLH_E_HIP
    found = re.fullmatch(r"(hip\w+)\(.*\) failed: (.+) \((.+):(\d+)\)", message)
    assert found, message
    assert found.group(3).endswith(stage_calls.STAGES[stage][0]) and int(found.group(4)) > 0
    assert message in str(info.value)
