"""`ransac_pairs(samples="device")` on the GPU (INPUTS.md, "Device samples: the rule"): the draw kernel alone
(`glh_stage_ransac_samples`) and the whole call against tests/ransac_draw_restated.py in every number; the fits of a call
that draws against the same call given those samples as arrays -- the path tests/test_gpu_ransac_pairs.py holds to the host
-- byte for byte; chunking, seeds, `np.random`, short and enumerated pairs, and the matcher method."""
import datetime
import functools
import math

import numpy as np
import pytest

from tests import ransac_draw_restated as rd
from tests import ransac_pair_cases as pc

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE0012345678
SCENES = ("mixed_rows", "kinds_px", "weights", "six_parameters")
INFO = ("values", "status", "consensus", "refit_values", "refit_status", "mean_errors", "winner", "hyp_offset")
WORKGROUP = 256  # csrc/glh_calib.h: CAL_TB, the draw kernel's


def run(name, **changes):
    """One call of ransac_pairs on fresh objects of scene `name`."""
    from glimpse_amd import optimize

    cams, matches, d = pc.scene(name)
    results, info = optimize.ransac_pairs(matches, return_info=True, **{**pc.call(name, d), **changes})
    return dict(matches=matches, results=results, info=info)


@functools.lru_cache(maxsize=None)
def drawn(name):
    return run(name, samples="device", seed=SEED)


def same(a, b):
    """Every number of two calls: the per-hypothesis and per-pair arrays, the samples, and each pair's result."""
    if not all(a["info"][key].tobytes() == b["info"][key].tobytes() for key in INFO):
        return False
    for x, y in zip(a["info"]["samples"], b["info"]["samples"]):
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            return False
    for x, y in zip(a["results"], b["results"]):
        if (x is None) != (y is None) or (x is not None and (x[0].tobytes() != y[0].tobytes() or not np.array_equal(x[1], y[1]))):
            return False
    return len(a["results"]) == len(b["results"])


@pytest.mark.parametrize("n", [1, 4, 5, 12, 65])
def test_the_draw_kernel_equals_the_restatement(n):
    """Groups of n + 1, 63, 64, 65, 257 and 2^20 rows (those above n) in one call; more hypotheses than one workgroup of the
    draw kernel holds and no multiple of it; ids neither from 0 nor in order."""
    from glimpse_amd import _lib

    groups = [(s, count, k) for s, count, k in ((n + 1, 100, 9), (63, 37, 0), (64, 64, 2 ** 24 - 1), (65, 1, 3), (257, 150, 70000),
                                                (2 ** 20, 77, 5)) if s > n]
    rows, counts, ids = (np.array(v) for v in zip(*groups))
    offset = np.concatenate(([0], np.cumsum(counts)))
    assert offset[-1] > WORKGROUP and offset[-1] % WORKGROUP
    got, times = _lib.stage_ransac_samples(0, rows, ids, offset, n, rd.seed_words(SEED), return_times=True)
    print("n", n, "hypotheses", offset[-1], "times_ms", times)
    assert got.shape == (offset[-1], n) and got.dtype == np.int64
    for g, (s, count, k) in enumerate(groups):
        assert np.array_equal(got[offset[g]:offset[g + 1]], rd.drawn(SEED, k, s, n, np.arange(count))), (n, s)
    # a group's samples are its own: the last group alone, under its id, and from a later hypothesis on
    s, count, k = groups[-1]
    alone = _lib.stage_ransac_samples(0, [s], [k], [0, count], n, rd.seed_words(SEED))
    assert np.array_equal(alone, got[offset[-2]:])
    other = _lib.stage_ransac_samples(0, [s], [k], [0, count], n, rd.seed_words(SEED + 1))
    assert not np.array_equal(other, alone)


def test_the_stage_refuses_what_it_cannot_draw():
    from glimpse_amd import _lib

    good = dict(rows=[13, 64], group_id=[0, 1], hyp_offset=[0, 3, 5], n=12, seed=(1, 2))
    assert _lib.stage_ransac_samples(0, **good).shape == (5, 12)
    for change in (dict(rows=[12, 64]), dict(rows=[13, 2 ** 31]), dict(group_id=[0, -1]), dict(hyp_offset=[1, 3, 5]),
                   dict(hyp_offset=[0, 3, 2]), dict(n=0)):
        with pytest.raises(_lib.GlhError, match="ransac samples"):
            _lib.stage_ransac_samples(0, **{**good, **change})
    assert _lib.stage_ransac_samples(0, [], [], [0], 3, (1, 2)).shape == (0, 3)
    hyps, enumerated = _lib.ransac_hypotheses([2, 4, 5, 13, 2 ** 31 - 1], 2, 9)
    assert list(hyps) == [0, 6, 9, 9, 9] and list(enumerated) == [False, True, False, False, False]
    assert _lib.ransac_combinations(4, 2, 6).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    for bad in ((4, 2, 7), (1, 2, 1), (4, 0, 1), (2 ** 31, 2, 1)):
        with pytest.raises(_lib.GlhError, match="ransac combinations"):
            _lib.ransac_combinations(*bad)
    with pytest.raises(_lib.GlhError, match="ransac hypotheses"):
        _lib.ransac_hypotheses([5], 0, 9)


@pytest.mark.parametrize("name", SCENES)
def test_the_samples_are_the_rules_and_the_fits_those_of_the_same_samples_given(name):
    got = drawn(name)
    call = pc.call(name)
    sizes = [m.size for m in got["matches"].values()]
    assert got["info"]["seed"] == SEED and "draw" in got["info"]["times_ms"]
    for k, s in enumerate(sizes):
        want = rd.samples(SEED, k, s, call["n"], call["iterations"])
        assert want is not None and np.array_equal(got["info"]["samples"][k], want), (name, k)
        assert got["info"]["samples"][k].dtype == np.int64
        assert got["info"]["hyp_offset"][k + 1] - got["info"]["hyp_offset"][k] == len(want)
    given = run(name, samples=got["info"]["samples"])
    assert "seed" not in given["info"] and "draw" not in given["info"]["times_ms"]
    assert same(got, given)
    assert any(r is not None for r in got["results"])
    print(name, "times_ms", got["info"]["times_ms"])


@pytest.mark.parametrize("name", SCENES)
def test_chunks_and_seeds(name):
    got = drawn(name)
    pairs = len(got["matches"])
    split = run(name, samples="device", seed=SEED, budget=1)  # (no two pairs fit one byte: a chunk each)
    assert got["info"]["chunks"] == 1 and split["info"]["chunks"] == pairs and same(got, split)
    if name == "mixed_rows":  # chunks of more than one pair as well: tests/test_gpu_ransac_pairs.py's budget
        some = run(name, samples="device", seed=SEED, budget=800)
        assert 1 < some["info"]["chunks"] < pairs and same(got, some)
    assert same(got, run(name, samples="device", seed=SEED))
    other = run(name, samples="device", seed=SEED ^ 1 << 40)
    assert not any(np.array_equal(a, b) for a, b in zip(got["info"]["samples"], other["info"]["samples"]))


@pytest.mark.parametrize("name", SCENES)
def test_without_a_seed_np_random_gives_it_in_one_call(name):
    np.random.seed(7)
    words = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
    after = np.random.get_state()
    seed = int(words[0]) | int(words[1]) << 32
    runs = []
    for _ in range(2):
        np.random.seed(7)
        runs.append(run(name, samples="device"))
        assert all(np.array_equal(a, b) for a, b in zip(after, np.random.get_state()))
        assert runs[-1]["info"]["seed"] == seed
    assert same(runs[0], runs[1]) and same(runs[0], run(name, samples="device", seed=seed))


def test_short_enumerated_and_smallest_drawn_pairs():
    """n = 2, iterations = 9: a pair of 2 rows (None), of 4 (C = 6 < 9: every combination, in order), of 5 (C = 10 =
    iterations + 1: the smallest drawn pair) and of 65, cut from the pairs of mixed_rows; then the same places with other
    neighbours."""
    from glimpse_amd import optimize

    cams, matches, d = pc.scene("mixed_rows")
    call = {**pc.call("mixed_rows", d), "iterations": 9, "min_inliers": 1, "samples": "device", "seed": SEED}
    source = list(matches.values())

    def cut(q, rows):
        m = source[q]
        return optimize.Matches(cams=m.cams, uvs=[m.uvs[0][:rows], m.uvs[1][:rows]])

    first = [cut(0, 2), cut(1, 4), cut(2, 5), cut(3, 65)]
    second = [cut(3, 63), cut(1, 13), cut(2, 5), cut(0, 2)]
    assert math.comb(4, 2) < 9 and math.comb(5, 2) == 9 + 1
    out = []
    for pairs in (first, second):
        results, info = optimize.ransac_pairs({(q, q + 1): m for q, m in enumerate(pairs)}, return_info=True, **call)
        for k, m in enumerate(pairs):
            want = rd.samples(SEED, k, m.size, 2, 9)
            if want is None:
                assert info["samples"][k] is None and results[k] is None and info["winner"][k] == -1
                assert info["hyp_offset"][k] == info["hyp_offset"][k + 1]
            else:
                assert np.array_equal(info["samples"][k], want), k
        out.append((results, info))
    (results, info), (results2, info2) = out
    assert info["samples"][1].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert len(info["samples"][2]) == 9 and len(info["samples"][3]) == 9
    assert info["chunks"] == 1 and info["seed"] == SEED
    # the pair of 5 rows is pair 2 of both calls: the same samples, fits and result, whatever stands beside it
    a, b = info["hyp_offset"][2:4], info2["hyp_offset"][2:4]
    assert np.array_equal(info["samples"][2], info2["samples"][2])
    for key in INFO[:6]:
        assert info[key][a[0]:a[1]].tobytes() == info2[key][b[0]:b[1]].tobytes(), key
    assert info["winner"][2] == info2["winner"][2]
    assert (results[2] is None) == (results2[2] is None)
    if results[2] is not None:
        assert results[2][0].tobytes() == results2[2][0].tobytes() and np.array_equal(results[2][1], results2[2][1])
    # the enumerated pair against the same samples given
    given = optimize.ransac_pairs({(0, 1): first[1]}, return_info=True, **{**call, "samples": [info["samples"][1]], "seed": None})[1]
    b = info["hyp_offset"][1:3]
    for key in INFO[:6]:
        assert info[key][b[0]:b[1]].tobytes() == given[key].tobytes(), key


def test_fifty_iterations_find_a_winner_for_every_pair():
    got = run("mixed_rows", samples="device", seed=SEED, iterations=50)
    sizes = [m.size for m in got["matches"].values()]
    assert all(s > 2 for s in sizes)
    assert list(np.diff(got["info"]["hyp_offset"])) == [50] * len(sizes)
    assert (got["info"]["winner"] >= 0).all() and all(r is not None for r in got["results"])
    print("inliers", [len(r[1]) for r in got["results"]], "of", sizes)


def test_the_matcher_filters_the_rows_ransac_pairs_keeps():
    import glimpse_amd
    from glimpse_amd import optimize

    cams, matches, d = pc.scene("mixed_rows")
    call = pc.call("mixed_rows", d)
    want = optimize.ransac_pairs(matches, samples="device", seed=SEED, **call)
    cams, matches, d = pc.scene("mixed_rows")
    images = [glimpse_amd.Image(cam=cam, array=np.zeros((2, 2), np.uint8), datetime=datetime.datetime(2020, 1, 1, 0, k))
              for k, cam in enumerate(cams)]
    data = list(matches.values())
    before = [(m.uvs[0].copy(), m.uvs[1].copy()) for m in data]
    matcher = optimize.KeypointMatcher(images)
    matcher.matches = optimize.PairMatches(data, [i for i, _ in matches], [j for _, j in matches], (len(images), len(images)))
    counts = matcher.ransac_matches(samples="device", seed=SEED, **call)
    assert list(counts) == [-1 if r is None else len(r[1]) for r in want] and (counts > 0).any()
    for m, r, (uv0, uv1) in zip(data, want, before):
        keep = np.zeros(len(uv0), dtype=bool)
        if r is not None:
            keep[r[1]] = True
        assert np.array_equal(m.uvs[0], uv0[keep]) and np.array_equal(m.uvs[1], uv1[keep])
    assert sum(len(uv0) for uv0, _ in before) > sum(m.size for m in data)
