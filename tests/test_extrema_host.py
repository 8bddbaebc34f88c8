"""The joint extrema reduction of the fused step's phase A on the CPU: glh_math.h's wave_max4_joint -- the schedule the
kernel runs -- with its lane operations restated on arrays (tests/hostcheck/extrema_hostcheck.cpp), against four plain
min / max reductions over the wave.  Test-only: the product never runs this code on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "extrema_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "libextrema_hostcheck.so")


@pytest.fixture(scope="module")
def hc():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "glimpse_amd", "csrc", "glh_math.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", OUT, SRC], check=True)
    return C.CDLL(OUT)


def _reduce(hc, lanes):
    """lanes [4][64] (min u, min v, max u, max v per lane) -> the four extrema as the kernel stores them: the first lane of
    row k holds value k, the minima negated; every lane of a row must hold the same value."""
    lanes = np.ascontiguousarray(lanes, dtype=np.float64)
    out = np.empty(64)
    hc.hc_extrema4(lanes.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    rows = out.reshape(4, 16)
    assert (rows == rows[:, :1]).all(), "a row of the wave does not end with one value in all its lanes"
    return np.array([-rows[0, 0], -rows[1, 0], rows[2, 0], rows[3, 0]])


def _plain(lanes):
    return np.array([lanes[0].min(), lanes[1].min(), lanes[2].max(), lanes[3].max()])


def test_joint_reduction_equals_four_plain_reductions(hc):
    rng = np.random.default_rng(11)
    for trial in range(400):
        scale = 10.0 ** rng.integers(-3, 5)
        lanes = rng.standard_normal((4, 64)) * scale + rng.uniform(-2000, 2000)
        np.testing.assert_array_equal(_reduce(hc, lanes), _plain(lanes))


def test_the_extremum_is_found_in_every_lane(hc):
    """One outlier per value, in every lane in turn (each lane's path through the two swaps and the four row exchanges)."""
    base = np.tile(np.array([[5.0], [6.0], [-5.0], [-6.0]]), (1, 64))
    for lane in range(64):
        lanes = base.copy()
        lanes[0, lane], lanes[1, (lane + 17) % 64] = -1.0, -2.0
        lanes[2, (lane + 32) % 64], lanes[3, 63 - lane] = 1.0, 2.0
        np.testing.assert_array_equal(_reduce(hc, lanes), [-1.0, -2.0, 1.0, 2.0])


def test_idle_lanes_and_infinities(hc):
    """A lane without a particle holds the identities (+inf for a minimum, -inf for a maximum); a wave of idle lanes
    returns them; equal values and values differing in the last place are told apart exactly."""
    rng = np.random.default_rng(12)
    ident = np.array([np.inf, np.inf, -np.inf, -np.inf])
    lanes = np.tile(ident[:, None], (1, 64))
    np.testing.assert_array_equal(_reduce(hc, lanes), ident)
    for live in (1, 6, 31, 33, 63):
        lanes = np.tile(ident[:, None], (1, 64))
        at = rng.choice(64, live, replace=False)
        lanes[:, at] = rng.uniform(100, 1900, (4, live))
        np.testing.assert_array_equal(_reduce(hc, lanes), _plain(lanes))
    x = 1234.5678
    lanes = np.full((4, 64), x)
    lanes[0, 40], lanes[2, 9] = np.nextafter(x, -np.inf), np.nextafter(x, np.inf)
    np.testing.assert_array_equal(_reduce(hc, lanes), [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf), x])
