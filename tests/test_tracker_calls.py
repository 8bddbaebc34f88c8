"""The Python driver of a run (`glimpse_amd/tracker.py`) without a device: `_lib.Context` is replaced by a stub that
records every call it receives -- method, arguments, arrays as (shape, dtype, CRC32 of their bytes), so masks, parameter
tables and host draws are pinned exactly -- and answers the getters with scripted arrays.  The expected traces and result
digests are in tests/golden/tracker_calls.json; they were recorded from the driver as it was before it was restructured
into plan -> batch run -> assembly (commit 731d611) with

    python tests/test_tracker_calls.py --record

and what the driver asks of the device, call for call, and what it returns must not move.

Every scenario: 5 time steps, 3 tracks of 8 particles, 7 x 7 tiles, 2 observers of 64 x 48 uint8 frames, the second
covering time steps 2 to 4 only -- its template starts mid-sequence and splits the common frames into two runs."""
import datetime
import json
import os
import sys
import zlib

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import glimpse_amd
from glimpse_amd import _lib
from glimpse_amd import tracker as tracker_module

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracker_calls.json")
T0 = datetime.datetime(2020, 1, 1)
DAY = datetime.timedelta(days=1)
T, P, N, TILE = 5, 3, 8, (7, 7)


def abbreviate(x):
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return f"<{'x'.join(map(str, a.shape))} {a.dtype} {zlib.crc32(a.tobytes()):08x}>"
    if isinstance(x, (list, tuple)):
        return "[" + ", ".join(abbreviate(v) for v in x) + "]"
    if isinstance(x, np.dtype):
        return str(x)
    if isinstance(x, np.generic):
        x = x.item()
    if x is None or isinstance(x, (bool, int, float, str)):
        return repr(x)
    return type(x).__name__


class Recorder:
    """The call log all stub contexts of one scenario write into, and the script their getters answer from."""

    def __init__(self):
        self.calls = []
        self.contexts = []
        self.obs_status = {}        # (frame, observer, point) -> status word
        self.first_context_only = False  # the observer statuses are scripted for the first context made only
        self.point_status = {}      # point -> (status bits, error frame)

    def note(self, ctx, name, args, kwargs):
        text = ", ".join([abbreviate(a) for a in args] + [f"{k}={abbreviate(v)}" for k, v in kwargs.items()])
        self.calls.append(f"{ctx} {name}({text})")

    def names(self, ctx=None):
        return [c.split(" ", 1)[1].split("(")[0] for c in self.calls if ctx is None or c.startswith(f"{ctx} ")]


def stub_context(rec):
    class Context:
        def __init__(self, max_points, max_particles, n_observers=1, **kw):
            self.index = len(rec.contexts)
            rec.contexts.append(self)
            rec.note(self.index, "Context", (max_points, max_particles, n_observers), kw)
            self.handle, self.O, self.P, self.N, self.frame = 1, n_observers, 0, 0, 0

        def __getattr__(self, name):  # (every call that returns nothing)
            if name.startswith("_"):
                raise AttributeError(name)

            def call(*args, **kwargs):
                rec.note(self.index, name, args, kwargs)
            return call

        def close(self):
            rec.note(self.index, "close", (), {})
            self.handle = None

        def begin_sequence(self, n_points, n_particles, tile_size):
            rec.note(self.index, "begin_sequence", (n_points, n_particles, tile_size), {})
            self.P, self.N = n_points, n_particles

        def set_frame(self, frame):
            rec.note(self.index, "set_frame", (frame,), {})
            self.frame = frame

        def step(self, frame, *args, **kwargs):
            rec.note(self.index, "step", (frame,) + args, kwargs)
            self.frame = frame

        def _statuses(self, frame0, n_frames):
            out = np.zeros((n_frames, self.O, self.P), dtype=np.int32)
            if not rec.first_context_only or self.index == 0:
                for (f, o, p), word in rec.obs_status.items():
                    if frame0 <= f < frame0 + n_frames:
                        out[f - frame0, o, p] = word
            return out

        def observer_status(self):
            rec.note(self.index, "observer_status", (), {})
            return self._statuses(self.frame, 1)[0]

        def observer_status_frames(self, frame0, n_frames):
            rec.note(self.index, "observer_status_frames", (frame0, n_frames), {})
            return self._statuses(frame0, n_frames)

        def point_status(self):
            rec.note(self.index, "point_status", (), {})
            out = np.zeros(self.P, dtype=np.uint32)
            for p, (bits, _) in rec.point_status.items():
                out[p] = bits
            return out

        def point_error_frame(self):
            rec.note(self.index, "point_error_frame", (), {})
            out = np.zeros(self.P, dtype=np.int32)
            for p, (_, frame) in rec.point_status.items():
                out[p] = frame
            return out

        def get_tracks(self, frame0, n_frames):
            rec.note(self.index, "get_tracks", (frame0, n_frames), {})
            means = np.arange(self.P * n_frames * 6, dtype=float).reshape(self.P, n_frames, 6)
            return means, means + 0.5

        def get_covariances(self, frame0, n_frames):
            rec.note(self.index, "get_covariances", (frame0, n_frames), {})
            return np.arange(n_frames * self.P * 36, dtype=float).reshape(n_frames, self.P, 6, 6)

        def get_particles(self):
            rec.note(self.index, "get_particles", (), {})
            return 100.0 * self.frame + np.arange(self.P * self.N * 6, dtype=float).reshape(self.P, self.N, 6)

        def get_weights(self):
            rec.note(self.index, "get_weights", (), {})
            return 10.0 * self.frame + np.arange(self.P * self.N, dtype=float).reshape(self.P, self.N)

        def get_point_state(self, point):
            rec.note(self.index, "get_point_state", (point,), {})
            return self.get_particles()[point], self.get_weights()[point]

        def upload_done(self, ticket, wait=False):
            rec.note(self.index, "upload_done", (ticket,), dict(wait=wait))
            return True

    return Context


class Env:
    """One scenario's tracker module with the stubs in place (pytest's monkeypatch, or `Patches` when recording)."""

    def __init__(self, patch):
        self.rec = rec = Recorder()
        self.kinds = {}
        patch.setattr(_lib, "Context", stub_context(rec))

        def no_device(*a, **k):
            raise RuntimeError("no device")

        def project(cam, xyz, device_id=0, directions=False):
            rec.note("-", "stage_project", (cam, xyz), {})
            uv = np.tile([32.0, 24.0], (len(xyz), 1))
            uv[len(xyz) // 4:] += 3.0  # (the prior's spread: three pixels)
            return uv

        patch.setattr(_lib, "device_memory", no_device)
        patch.setattr(_lib, "stage_project", project)
        real = tracker_module.Tracks

        def tracks(**kw):  # (what the driver hands to the container: arrays or lists of rows)
            self.kinds = {k: type(kw.get(k)).__name__ for k in ("means", "sigmas", "covariances", "particles", "weights",
                                                                 "errors", "warnings")}
            return real(**kw)

        patch.setattr(tracker_module, "Tracks", tracks)

    def tracker(self, **kw):
        kw.setdefault("max_search_dim", 64)
        cam = glimpse_amd.Camera(imgsz=(64, 48), f=(100, 100))
        rng = np.random.default_rng(7)
        observers = []
        for steps in (range(0, T), range(2, T)):
            images = [glimpse_amd.Image("synthetic", cam=cam, datetime=T0 + i * DAY,
                                        array=rng.integers(0, 256, size=(48, 64), dtype=np.uint8)) for i in steps]
            observers.append(glimpse_amd.Observer(images, sigma=0.3))
        return glimpse_amd.Tracker(observers, **kw)

    @staticmethod
    def models(counts=(N,) * P):
        return [glimpse_amd.CartesianMotion(xy=(10.0 + p, 20.0 - p), time_unit=DAY, dem=0.0, dem_sigma=0.1, n=n)
                for p, n in enumerate(counts)]

    def digest(self, tracks):
        out = {k: abbreviate(getattr(tracks, k)) for k in ("means", "sigmas", "covariances", "particles", "weights")}
        out["errors"] = [None if e is None else f"{type(e).__name__}: {e}" for e in tracks.errors]
        out["warnings"] = [None if w is None else [f"{type(x).__name__}: {x}" for x in w] for w in tracks.warnings]
        out["kinds"] = self.kinds
        return dict(calls=self.rec.calls, result=out)


def stub_tracks(n_frames=T, n_points=P):
    means = np.arange(n_points * n_frames * 6, dtype=float).reshape(n_points, n_frames, 6)
    return means, means + 0.5


# ---- the scenarios ---------------------------------------------------------------------------------------------------
def philox_uniform(env):
    t = env.tracker().track(env.models(), tile_size=TILE, rng="philox", seed=3)
    names = [n for n in env.rec.names() if n in ("track", "step", "evolve", "update_weights", "observer_status_frames")]
    assert names == ["track", "evolve", "update_weights", "track", "observer_status_frames", "observer_status_frames"]
    tracks = [c for c in env.rec.calls if c.startswith("0 track(")]
    assert tracks[0].startswith("0 track([1], ") and tracks[1].startswith("0 track([3, 4], ")
    return env.digest(t)


def philox_late_track(env):
    t = env.tracker().track(env.models(), tile_size=TILE, rng="philox", observer_mask=[[1, 1], [1, 0], [0, 1]])
    names = env.rec.names()
    assert "track" not in names and "step" not in names and names.count("record_moments") == T
    return env.digest(t)


def numpy_stream(env):
    np.random.seed(11)
    t = env.tracker().track(env.models(), tile_size=TILE)
    assert env.rec.names().count("step") == 3 and all("normals=<3x8x3" in c for c in env.rec.calls if " step(" in c)
    return env.digest(t)


def numpy_stream_covariances(env):
    np.random.seed(11)
    t = env.tracker().track(env.models(), tile_size=TILE, return_covariances=True)
    assert env.rec.names().count("record_covariances") == T and t.sigmas is None and t.covariances.shape == (P, T, 6, 6)
    return env.digest(t)


def philox_particles(env):
    t = env.tracker().track(env.models(), tile_size=TILE, rng="philox", return_particles=True)
    names = env.rec.names()
    assert "track" not in names and names.count("step") == 3 and names.count("get_particles") == T
    assert names.count("get_weights") == T and t.particles.shape == (P, T, N, 6) and t.weights.shape == (P, T, N)
    return env.digest(t)


def philox_stratified(env):
    t = env.tracker(resample_method="stratified").track(env.models(), tile_size=TILE, rng="philox")
    names = env.rec.names()
    assert "track" not in names and "step" not in names and names.count("resample") == T - 1
    return env.digest(t)


def deferred_out_of_bounds(env):
    env.rec.obs_status[(3, 0, 1)] = _lib.OBS_OUT_OF_BOUNDS
    t = env.tracker().track(env.models(), tile_size=TILE, rng="philox")
    w = t.warnings
    assert w[0] is None and w[2] is None and len(w[1]) == 1 and type(w[1][0]) is UserWarning
    assert str(w[1][0]) == "Particles too close to or beyond image bounds, skipping image"
    return env.digest(t)


def tile_too_large_fixed(env):
    env.rec.obs_status[(3, 0, 1)] = _lib.OBS_TILE_TOO_LARGE
    t = env.tracker().track(env.models(), tile_size=TILE, rng="philox")
    assert env.rec.names().count("begin_sequence") == 1 and len(env.rec.contexts) == 1
    assert type(t.warnings[1][0]) is RuntimeWarning
    assert str(t.warnings[1][0]) == "search tile exceeds max_search_dim=64; observer 0 skipped"
    return env.digest(t)


def tile_too_large_grows(env):
    env.rec.obs_status[(3, 0, 1)] = _lib.OBS_TILE_TOO_LARGE
    env.rec.first_context_only = True
    t = env.tracker(max_search_dim=None).track(env.models(), tile_size=TILE, rng="philox")
    made = [c for c in env.rec.calls if " Context(" in c or " close(" in c]
    # (three offsets of 3 pixels: a spread of sqrt(27) = 5.2 pixels; 7 + 10 * 5.2 + 8 = 67 -> 80, doubled: 160; the larger
    # context exists before the one in use is closed)
    assert len(made) == 3 and "max_search_dim=80" in made[0] and "max_search_dim=160" in made[1] and made[2] == "0 close()"
    assert env.rec.names().count("begin_sequence") == 2 and all(w is None for w in t.warnings)
    return env.digest(t)


def point_failure(env):
    env.rec.point_status[1] = (_lib.PT_NAN, 3)
    t = env.tracker().track(env.models(), tile_size=TILE, rng="philox")
    means, sigmas = stub_tracks()
    assert type(t.errors[1]) is ValueError and str(t.errors[1]) == "Some particles have missing (NaN) values"
    assert t.errors[0] is None and t.errors[2] is None
    assert np.isnan(t.means[1, 3:]).all() and np.isnan(t.sigmas[1, 3:]).all()
    np.testing.assert_array_equal(t.means[1, :3], means[1, :3])
    np.testing.assert_array_equal(t.means[[0, 2]], means[[0, 2]])
    np.testing.assert_array_equal(t.sigmas[[0, 2]], sigmas[[0, 2]])
    return env.digest(t)


def point_failure_single_track(env):
    env.rec.point_status[0] = (_lib.PT_NAN, 3)
    with pytest.raises(ValueError, match=r"Some particles have missing \(NaN\) values"):
        env.tracker().track(env.models((N,)), tile_size=TILE, rng="philox")
    return dict(calls=env.rec.calls, result=None)


def numpy_replay(env):
    env.rec.point_status[1] = (_lib.PT_NAN, 3)
    np.random.seed(11)
    t = env.tracker().track(env.models(), tile_size=TILE)
    assert env.rec.names().count("begin_sequence") == 2
    # (track 1 stops drawing at the frame where it failed: the draws of track 2 move up the stream)
    steps = [c for c in env.rec.calls if " step(4, " in c]
    assert len(steps) == 2 and steps[0] != steps[1]
    return env.digest(t)


def two_particle_counts(env):
    t = env.tracker().track(env.models((N, N, 6)), tile_size=TILE, rng="philox")
    offsets = [c for c in env.rec.calls if " set_point_offset(" in c]
    assert offsets == ["0 set_point_offset(0)", "1 set_point_offset(2)"]
    assert env.kinds["means"] == "list" and env.kinds["sigmas"] == "list" and t.means.shape == (P, T, 6)
    return env.digest(t)


SCENARIOS = [philox_uniform, philox_late_track, numpy_stream, numpy_stream_covariances, philox_particles,
             philox_stratified, deferred_out_of_bounds, tile_too_large_fixed, tile_too_large_grows, point_failure,
             point_failure_single_track, numpy_replay, two_particle_counts]


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda s: s.__name__)
def test_trace(scenario, expected, monkeypatch):
    got = json.loads(json.dumps(scenario(Env(monkeypatch))))
    want = expected[scenario.__name__]
    assert got["calls"] == want["calls"]
    assert got["result"] == want["result"]


# ---- the plan --------------------------------------------------------------------------------------------------------
def random_plans(count=200):
    rng = np.random.default_rng(5)
    for k in range(count):
        n_times, n_obs, n_tracks = int(rng.integers(2, 9)), int(rng.integers(1, 4)), int(rng.integers(1, 5))
        if k % 4 == 0:  # (the uniform runs a random draw rarely makes: every observer from some step on, full mask)
            has = np.arange(n_times)[:, None] >= rng.integers(0, 3, size=n_obs)[None, :]
            mask = np.ones((n_tracks, n_obs), dtype=bool)
        else:
            has = rng.random((n_times, n_obs)) < 0.7
            mask = rng.random((n_tracks, n_obs)) < 0.8
        method = "systematic" if k % 8 else "stratified"
        yield has, mask, has.argmax(axis=0), method


def test_plan_matches_the_formula():
    for has, mask, template_indices, method in random_plans():
        plan = tracker_module._Plan(has, mask, template_indices, method)
        n_times, first, last = len(has), [], []
        for p in range(len(mask)):
            seen = [i for i in range(n_times) if (has[i] & mask[p]).any()]
            first.append(seen[0] if seen else 0)
            last.append(seen[-1] if seen else -1)
        np.testing.assert_array_equal(plan.first, first)
        np.testing.assert_array_equal(plan.last, last)
        np.testing.assert_array_equal(plan.empty, [b < a for a, b in zip(first, last)])
        first, last = np.array(first), np.array(last)
        uniform = bool(mask.all()) and bool((first == first[0]).all()) and bool((last == last[0]).all())
        assert plan.uniform == uniform and (plan.lo, plan.hi) == (
            int(first[~plan.empty].min()) if (~plan.empty).any() else 0, int(last.max()))
        for i in range(n_times):
            common = (uniform and method == "systematic" and bool(((first < i) & (i <= last)).all())
                      and not (template_indices == i).any())
            assert bool(plan.common[i]) == common
            np.testing.assert_array_equal(plan.starting(i), (first == i) & ~plan.empty)
            np.testing.assert_array_equal(plan.running(i), (first < i) & (i <= last))


def test_plan_run_end_stops_at_the_first_other_frame():
    seen = 0
    for has, mask, template_indices, method in random_plans():
        plan = tracker_module._Plan(has, mask, template_indices, method)
        for i in np.nonzero(plan.common)[0]:
            for through in range(int(i), len(has) + 1):
                j = plan.run_end(int(i), through)
                assert i <= j <= max(i, min(plan.hi, through)) and plan.common[i:j + 1].all()
                assert j == min(plan.hi, through) or j == i > min(plan.hi, through) or not plan.common[j + 1]
                seen += 1
    assert seen > 100  # (the cases do reach common frames)


# ---- the merge of parts ----------------------------------------------------------------------------------------------
def test_merge_parts():
    merge = glimpse_amd.tracks.merge_parts
    a, b = np.zeros((2, 5, 6)), np.ones((1, 5, 6))
    out = merge([a, b])
    assert isinstance(out, np.ndarray) and out.shape == (3, 5, 6) and (out[2] == 1).all()
    rows = merge([a, b], rows=True)  # (runs of several batches always hand lists over)
    assert isinstance(rows, list) and len(rows) == 3 and rows[2] is not None and rows[2].shape == (5, 6)
    ragged = merge([a, np.ones((1, 4, 6))])
    assert isinstance(ragged, list) and [r.shape for r in ragged] == [(5, 6), (5, 6), (4, 6)]
    mixed = merge([a, [np.ones((5, 6))]])
    assert isinstance(mixed, list) and len(mixed) == 3
    assert merge([None, a]) is None and merge([None, None], rows=True) is None
    assert merge([[None, "e"], [None]]) == [None, "e", None]


if __name__ == "__main__":
    class Patches:  # (monkeypatch's setattr, kept for the life of the process)
        @staticmethod
        def setattr(target, name, value):
            setattr(target, name, value)

    assert sys.argv[1:] == ["--record"], __doc__
    recorded = {}
    real_context, real_tracks = _lib.Context, tracker_module.Tracks
    for scenario in SCENARIOS:
        _lib.Context, tracker_module.Tracks = real_context, real_tracks
        recorded[scenario.__name__] = scenario(Env(Patches))
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=0)
        f.write("\n")
    print({k: len(v["calls"]) for k, v in recorded.items()})
