"""The times of the thirteen stage exports of the six stage files (tests/stage_calls.py), which all come from the events
of csrc/glh_stage.h: with `return_times=True` each wrapper returns a dict whose keys are the stage's `*_TIMES` in order,
every `*_ms` finite and not negative, the copies taking some time -- and the result's bytes are those of the call without
times.

The DEM is 65 x 17 cells, one more than a 64 x 16 tile each way, with one origin, 8 headings, a 3 x 3 window, a Gaussian
of radius 1 and one triangle: the smallest that cross a tile boundary, not workload sizes.
"""
import math

import numpy as np
import pytest

from tests import stage_calls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calls():
    return stage_calls.calls(nx=65, ny=17, headings=8, window=3, radius=1)


def _bytes(result):
    arrays = result if isinstance(result, tuple) else (result,)
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


@pytest.mark.parametrize("stage", list(stage_calls.STAGES))
def test_times_are_named_finite_and_leave_the_result_alone(calls, stage):
    from glimpse_amd import _lib

    names = getattr(_lib, stage_calls.STAGES[stage][1])
    *result, times = calls[stage](True)
    result = result[0] if len(result) == 1 else tuple(result)
    print(stage, times)
    assert tuple(times) == names  # (a dict keeps its order)
    for name, value in times.items():
        if name.endswith("_ms"):
            assert math.isfinite(value) and value >= 0.0, name
    assert times["upload_ms"] + times["download_ms"] > 0.0
    plain = calls[stage](False)
    assert type(plain) is type(result) and _bytes(plain) == _bytes(result)
