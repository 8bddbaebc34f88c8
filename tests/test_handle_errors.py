"""A HIP failure while a device object is made reaches `glh_last_error()`, and the object it leaves behind is closed.

The four handle-based objects (`_lib.Orient`, `Calib`, `Matcher`, `Sift`) are made by one template (csrc/glh_stage.h:
create_object) and held by one Python base (`_lib._Handle`).  Where no device is present the first HIP call of a valid
create, hipSetDevice, fails: each must raise GLH_E_HIP with that call, the runtime's words and its own stage file's name and
line in the message, as tests/test_stage_errors.py asks of the stateless stages.  Skipped where a device is present: there
the calls succeed (the GPU tests of each object cover its life cycle).
"""
import re

import numpy as np
import pytest

from tests.test_stage_errors import GLH_E_HIP, _no_device

GLH_E_STATE = -4

# object -> (its stage file, its smallest legal arguments, a call that needs an open handle)
OBJECTS = {
    "Orient": ("glh_orient.hip",  # 1 image, 0 pairs
               lambda: (1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros((0, 2)), np.zeros((0, 2))),
               lambda obj: obj.eval(np.eye(3)[None], np.zeros((1, 3, 3, 3)))),
    "Calib": ("glh_calib.hip",  # 1 camera, 0 controls
              lambda: (1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                       np.zeros(1, np.int64), np.zeros((0, 2)), np.zeros((0, 3))),
              lambda obj: obj.eval(np.zeros((1, 1, 24)), np.eye(3)[None, None], [], [])),
    "Matcher": ("glh_match.hip", lambda: (), lambda obj: obj.put(0, np.zeros((1, 4), np.uint8))),
    "Sift": ("glh_sift.hip", lambda: (), lambda obj: obj.counts()),
}


@pytest.mark.parametrize("name", list(OBJECTS))
def test_a_failed_create_is_reported_from_the_stage_file_and_leaves_a_closed_object(name):
    from glimpse_amd import _lib

    if not _no_device():
        pytest.skip("a device is present: the HIP calls succeed")
    source, arguments, method = OBJECTS[name]
    cls = getattr(_lib, name)
    obj = object.__new__(cls)  # (kept, so that what a failed __init__ leaves behind can be looked at)
    with pytest.raises(_lib.GlhError) as info:
        obj.__init__(*arguments())
    message = _lib.load().glh_last_error().decode()
    print(name, info.value.code, message)
    assert info.value.code == GLH_E_HIP
    found = re.fullmatch(r"(hip\w+)\(.*\) failed: (.+) \((.+):(\d+)\)", message)
    assert found, message
    assert found.group(3).endswith(source) and int(found.group(4)) > 0
    assert message in str(info.value)
    assert not obj._h
    obj.close()
    obj.close()
    assert not obj._h
    with pytest.raises(_lib.GlhError, match="the handle is closed") as closed:
        method(obj)
    assert closed.value.code == _lib.E_STATE == GLH_E_STATE
