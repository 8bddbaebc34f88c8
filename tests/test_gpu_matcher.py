"""The descriptor search on the device (glh_match_knn2, glimpse_amd/csrc/glh_match.hip) against its NumPy restatement
(tests/matcher_restated.py): idx and d2 exactly, np.array_equal, on both paths; the handle's life cycle; and
optimize.match_keypoints / KeypointMatcher.build_matches on the GPU against what the reference returned with the
brute-force stand-in (tools/make_golden_matcher.py).

The integer kernel takes T in tiles of 128 rows (subtiles of 32 for the matrix instruction, whose accumulator gives lane
half h rows 8 g + 4 h + r), the float kernel in tiles of 32; with few queries every tile is a range of its own and the
merge kernel folds them: that is so for every shape up to test_middle_size.  The workgroups of the integer kernel sweep
several tiles each -- the register prefetch, the barriers between tiles, the per-tile best two pushed into the running best
two -- only when there are more than 8 query blocks of 128 per tile; test_integer_kernel_sweeps_several_tiles has those
shapes, with a merge and without one."""
import contextlib
import io

import numpy as np
import pytest

from tests import matcher_cases as mc
from tests import matcher_restated as mr

pytestmark = pytest.mark.gpu

N_Q = (1, 2, 31, 33, 97)
N_T = (1, 2, 31, 32, 33, 65, 257)


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    _lib.load()
    return _lib


def same(found, expected, what):
    idx, d2 = found[:2]
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == expected[0].shape, what
    assert np.array_equal(idx, expected[0]), what
    assert np.array_equal(d2, expected[1]), what  # (inf == inf; no NaN is made here)


def integer_pools(dim, seed):
    """Q (97, dim) and T (257, dim) uint8, unrelated to each other (a swapped row / column map cannot pass), with all-0
    and all-255 rows on both sides: the largest d2, and the two ends of the shift to int8."""
    rng = np.random.default_rng(seed)
    q, t = rng.integers(0, 256, (97, dim), dtype=np.uint8), rng.integers(0, 256, (257, dim), dtype=np.uint8)
    q[1], q[30], q[96] = 0, 255, 255
    t[0], t[1], t[32], t[256] = 255, 0, 255, 0
    return q, t


def sweep(lib, q_pool, t_pool, path, what):
    with lib.Matcher() as m:
        for a, n_q in enumerate(N_Q):
            assert m.put(a, q_pool[:n_q], path=path) == what
        for n_t in N_T:
            assert m.put(100, t_pool[:n_t], path=path) == what
            for a, n_q in enumerate(N_Q):
                same(m.knn2(a, 100), mr.knn2(q_pool[:n_q], t_pool[:n_t], path), (what, q_pool.shape[1], n_q, n_t))


@pytest.mark.parametrize("dim", (128, 64, 36, 1, 256, 200))  # K steps 4, 2, 2, 1 and, for 129 .. 256, 8
def test_integer_path_edge_shapes(lib, dim):
    q, t = integer_pools(dim, 100 + dim)
    sweep(lib, q, t, None, "integer")
    # the largest distance there is: dim * 255^2, exact in int32 and in float32
    expected = mr.knn2(q[:97], t[:2])
    assert expected[1][1, 0] == 0 and expected[1][30].tolist() == [0.0, dim * 255.0 ** 2]


@pytest.mark.parametrize("dim", (128, 64, 36, 1, 257))
def test_float_path_edge_shapes(lib, dim):
    rng = np.random.default_rng(200 + dim)
    q = (rng.normal(0, 1, (97, dim)) * np.exp(rng.normal(0, 2, (97, 1)))).astype(np.float32)
    t = (rng.normal(0, 1, (257, dim)) * np.exp(rng.normal(0, 2, (257, 1)))).astype(np.float32)
    t[40] = t[7]  # an exact tie at any dim
    sweep(lib, q, t, None, "float")
    # root-SIFT: unit rows of square roots, distances close together
    d = np.sqrt(rng.dirichlet(np.full(dim, 0.3), 97 + 257)).astype(np.float32)
    # (at dim 1 every row is [1.]: integer values, which the host sends down the integer path; the same bits either way)
    sweep(lib, d[:97], d[97:], None, "integer" if dim == 1 else "float")


@pytest.mark.parametrize("dim", (128, 36, 1))
def test_float_path_on_integers_equals_the_integer_path(lib, dim):
    q, t = integer_pools(dim, 300 + dim)
    sweep(lib, q, t, "float", "float")
    with lib.Matcher() as m:
        assert m.put(0, q) == "integer" and m.put(1, t) == "integer"
        assert m.put(2, q.astype(np.float64)) == "integer" and m.put(3, t.astype(np.float32), path="float") == "float"
        assert m.put(4, q, path="float") == "float"
        by_integer, by_float = m.knn2(0, 1), m.knn2(4, 3)
        same(by_float, by_integer, dim)
        same(m.knn2(2, 1), by_integer, dim)
        same(by_integer, mr.knn2(q, t), dim)


PLANTS = {  # name -> the train rows that hold the nearest and the second nearest of query 0, n_t = 300
    "one subtile, one lane half": (1, 3),
    "one subtile, both lane halves": (2, 5),
    "both lane halves, second first": (13, 10),
    "one tile of the integer kernel, two of the float kernel": (3, 117),
    "different tiles": (5, 200),
    "different tiles, the nearer one later": (260, 5),
    "the last, partial tile": (290, 299),
    "the last row and the first": (299, 0),
}


@pytest.mark.parametrize("path", (None, "float"))
def test_planted_neighbours(lib, path):
    rng = np.random.default_rng(5)
    far = rng.integers(128, 256, (300, 128), dtype=np.uint8)
    q = rng.integers(0, 64, (40, 128), dtype=np.uint8)  # 40 queries: both lane halves of a wave hold real ones
    with lib.Matcher() as m:
        m.put(0, q, path=path)
        for name, (first, second) in PLANTS.items():
            t = far.copy()
            t[first], t[second] = q[0], q[0]
            t[first, 0] += 1   # d2 1
            t[second, 1] += 2  # d2 4
            m.put(1, t, path=path)
            idx, d2 = m.knn2(0, 1)
            assert idx[0].tolist() == [first, second] and d2[0].tolist() == [1.0, 4.0], name
            same((idx, d2), mr.knn2(q, t, path), name)
        # exact duplicates of queries at a lower and at a higher train index: in one subtile, across tiles and ranges
        for name, rows in (("one subtile", (10, 20)), ("across subtiles", (31, 32)), ("across tiles", (10, 150)),
                           ("three copies", (260, 127, 128)), ("into the last tile", (0, 299))):
            t = far.copy()
            for r in rows:
                t[r] = q[7]
            t[rows[0] + 2] = q[39]
            m.put(1, t, path=path)
            idx, d2 = m.knn2(0, 1)
            assert idx[7].tolist() == sorted(rows)[:2] and d2[7].tolist() == [0.0, 0.0], name
            assert idx[39, 0] == rows[0] + 2 and d2[39, 0] == 0, name
            same((idx, d2), mr.knn2(q, t, path), name)


def test_middle_size_splits_t_over_workgroups_and_merges(lib):
    rng = np.random.default_rng(6)
    base = np.minimum(rng.gamma(0.6, 40.0, (4000, 128)), 255)
    q = np.clip(base[rng.integers(0, 4000, 3000)] + rng.integers(-6, 7, (3000, 128)), 0, 255).astype(np.uint8)
    t = np.clip(base[rng.integers(0, 4000, 5000)] + rng.integers(-6, 7, (5000, 128)), 0, 255).astype(np.uint8)
    t[4999], t[17] = q[2999], q[2999]
    with lib.Matcher() as m:
        m.put(0, q)
        m.put(1, t)
        idx, d2, times = m.knn2(0, 1, return_times=True)
        assert times["merge"] > 0 and times["search"] > 0, times  # 24 query blocks: T in 40 ranges
        assert idx[2999].tolist() == [17, 4999]
        same((idx, d2), mr.knn2(q, t), "3000 x 5000 x 128")
        # the float kernel with several tiles to a range and a merge: 12 query blocks, 79 ranges of 2 tiles
        m.put(2, q[:1500], path="float")
        m.put(3, t[:5000], path="float")
        found = m.knn2(2, 3)
        same(found, (idx[:1500], d2[:1500]), "float 1500 x 5000 x 128")


def plant(q, t, plants, copies):
    """`t` with neighbours planted for queries of `q`: plants {query: (nearest row, second row)} at d2 1 and 4, copies
    {query: rows} exact duplicates of the query."""
    for query, (first, second) in plants.items():
        t[first], t[second] = q[query], q[query]
        t[first, 0] += 1
        t[second, 1 % t.shape[1]] += 2
    for query, rows in copies.items():
        for r in rows:
            t[r] = q[query]
    return t


def several_tiles_case(n_q, n_t, dim, tiles):
    """(q, t, plants, copies): far rows (128 .. 255) against near queries (0 .. 63), so the planted rows are the answer."""
    rng = np.random.default_rng(n_q)
    q = rng.integers(0, 64, (n_q, dim), dtype=np.uint8)
    t = rng.integers(128, 256, (n_t, dim), dtype=np.uint8)
    span, last = min(128 * tiles, n_t), n_t - 1  # the rows of the first range; the last row
    plants = {0: (span - 3, 5), 1: (6, span - 4), n_q - 1: (last, 130), 77: (129, last - 1), 4097: (127, 128)}
    copies = {7: (10, 140, span - 6), 130: (last - 7, 3), n_q - 2: (255, 256), 200: (span // 2 + 20, last - 9)}
    taken = [r for rows in (*plants.values(), *copies.values()) for r in rows] + [50]
    assert len(set(taken)) == len(taken) and max(taken) < n_t
    t = plant(q, t, plants, copies)
    q[300], t[50] = 0, 255  # the largest distance there is at this dim, beside the planted ones
    return q, t, plants, copies


@pytest.mark.parametrize("n_q,n_t,dim,tiles,ranges", ((16384, 2100, 128, 3, 6), (12000, 2500, 256, 2, 10),
                                                     (65537, 300, 36, 3, 1), (65700, 1000, 200, 8, 1)))
def test_integer_kernel_sweeps_several_tiles(lib, n_q, n_t, dim, tiles, ranges):
    """`tiles` tiles of 128 train rows to a workgroup, T in `ranges` ranges (1: no merge, the search kernel writes the
    result itself).  Planted: the nearer row in a later tile of the same range than the second and the other way round,
    in the last partial tile, in another range, either side of a tile's edge; exact copies at a lower and a higher index
    in the tiles of one range and across ranges."""
    blocks, n_tiles = -(-n_q // 128), -(-n_t // 128)  # (the library's own split, glh_match.hip: match_knn2)
    want = max(1, min(1024 // blocks, n_tiles))
    assert (-(-n_tiles // want), -(-n_tiles // -(-n_tiles // want))) == (tiles, ranges)
    q, t, plants, copies = several_tiles_case(n_q, n_t, dim, tiles)
    with lib.Matcher() as m:
        assert m.put(0, q) == "integer" and m.put(1, t) == "integer"
        idx, d2, times = m.knn2(0, 1, return_times=True)
    assert (times["merge"] > 0) == (ranges > 1), times
    for query, rows in plants.items():
        assert idx[query].tolist() == list(rows) and d2[query].tolist() == [1.0, 4.0], query
    for query, rows in copies.items():
        assert idx[query].tolist() == sorted(rows)[:2] and d2[query].tolist() == [0.0, 0.0], query
    same((idx, d2), mr.knn2_large(q, t), (n_q, n_t, dim))


def test_handle_life_cycle(lib):
    rng = np.random.default_rng(7)
    sets = [rng.integers(0, 256, (int(n), 64), dtype=np.uint8) for n in rng.integers(1, 200, 48)]
    with lib.Matcher() as m:
        for slot, d in enumerate(sets):  # many sets resident at once
            m.put(slot, d)
        assert m.slots() == list(range(48))
        for a, b in ((0, 47), (47, 0), (13, 13), (20, 31)):
            same(m.knn2(a, b), mr.knn2(sets[a], sets[b]), (a, b))
        m.drop(13)
        assert 13 not in m.slots()
        with pytest.raises(lib.GlhError, match="unknown slot 13"):
            m.knn2(13, 0)
        with pytest.raises(lib.GlhError, match="unknown slot 13"):
            m.drop(13)
        m.put(13, sets[5])  # the same slot again, another set
        same(m.knn2(13, 20), mr.knn2(sets[5], sets[20]), "put again")
        m.put(20, sets[6])  # in the place of a resident set
        same(m.knn2(13, 20), mr.knn2(sets[5], sets[6]), "replaced")
        with pytest.raises(lib.GlhError, match="unknown slot 99"):
            m.knn2(0, 99)
        m.put(60, rng.integers(0, 256, (5, 32), dtype=np.uint8))
        with pytest.raises(lib.GlhError, match="dim mismatch: slot 0 has 64, slot 60 has 32"):
            m.knn2(0, 60)
        m.put(61, rng.normal(0, 1, (5, 64)))
        with pytest.raises(lib.GlhError, match="mixed kinds: slot 0 is uint8, slot 61 is float32"):
            m.knn2(0, 61)
        with pytest.raises(lib.GlhError, match="n == 0"):
            m.put(62, np.zeros((0, 64), np.uint8))
        with pytest.raises(lib.GlhError, match="slot -1"):
            m.put(-1, sets[0])
        with pytest.raises(ValueError, match="descriptors"):
            m.put(62, np.zeros(64, np.uint8))
        assert m.put(63, rng.integers(0, 256, (3, 300), dtype=np.uint8)) == "float"  # dim > 256: no integer path
        same(m.knn2(0, 47), mr.knn2(sets[0], sets[47]), "after the errors")
    for call in (lambda: m.knn2(0, 47), lambda: m.put(0, sets[0]), lambda: m.drop(0)):
        with pytest.raises(lib.GlhError, match="the handle is closed"):
            call()
    m.close()  # twice is nothing
    load = lib.load()
    assert load.glh_match_destroy(None) == 0 and load.glh_match_create(0, None) == -1
    with pytest.raises(lib.GlhError):
        lib.Matcher(device_id=1 << 20)


@pytest.mark.parametrize("c,r,d,w", mc.OPTIONS)
def test_match_keypoints_on_the_gpu(lib, golden, c, r, d, w):
    from glimpse_amd import optimize

    g = golden("matcher_pairs.npz")
    ka, kb = (g["pts_a"], g["desc_a"]), (g["pts_b"], g["desc_b"])
    kwargs = mc.option_kwargs(g, c, r, d, w)
    found = optimize.match_keypoints(ka, kb, **kwargs)
    mc.same(found, mc.expected(g, c, r, d, w))
    mc.same(found, optimize.match_keypoints(ka, kb, matcher=mr.BruteForceMatcher(), **kwargs))
    # float descriptors with integer values take the integer path, root-like ones the float path: the same logic
    mc.same(optimize.match_keypoints((ka[0], ka[1].astype(np.float32)), kb, **kwargs), mc.expected(g, c, r, d, w))
    fa, fb = (ka[0], np.sqrt(ka[1] / 7.0).astype(np.float32)), (kb[0], np.sqrt(kb[1] / 7.0).astype(np.float32))
    mc.same(optimize.match_keypoints(fa, fb, **kwargs), optimize.match_keypoints(fa, fb, matcher=mr.BruteForceMatcher(), **kwargs))


def test_match_keypoints_edges_on_the_gpu(lib, golden):
    from glimpse_amd import optimize

    g = golden("matcher_pairs.npz")
    ka, kb = (g["pts_a"], g["desc_a"]), (g["pts_b"], g["desc_b"])
    mc.same(optimize.match_keypoints((ka[0][:1], ka[1][:1]), kb, return_ratios=True), [g[f"empty_few_{k}"] for k in range(3)])
    mc.same(optimize.match_keypoints((ka[0][:180], ka[1][:180]), kb, max_ratio=1e-9), [g[f"empty_none_plain_{k}"] for k in range(2)])
    mc.same(optimize.match_keypoints(ka, (kb[0][:1], kb[1][:1])), [g["single_uva"], g["single_uvb"]])
    with pytest.raises(ZeroDivisionError):
        optimize.match_keypoints((ka[0][:3], g["zd_a"]), (kb[0][:4], g["zd_b"]), max_ratio=float(g["max_ratio"]))


def test_build_matches_and_fit_on_the_gpu(lib, golden, tmp_path):
    import glimpse_amd
    from glimpse_amd import optimize

    g = golden("matcher_sequence.npz")
    ratio = float(g["max_ratio"])
    model = mc.sequence_matcher(g)
    with contextlib.redirect_stdout(io.StringIO()):
        model.build_matches(max_ratio=ratio, weights=True, path=tmp_path / "m", parallel=4)
    mc.assert_pairs_equal_golden(model.matches, g)
    with contextlib.redirect_stdout(io.StringIO()):  # cross-check: the same kernel with the slots swapped
        crossed = mc.sequence_matcher(g)
        crossed.build_matches(max_ratio=ratio, cross_check=True, **mc.setting_kwargs("seq12"))
        by_host = mc.sequence_matcher(g)
        by_host.build_matches(max_ratio=ratio, cross_check=True, matcher=mr.BruteForceMatcher(), **mc.setting_kwargs("seq12"))
    assert np.array_equal(np.column_stack([crossed.matches.row, crossed.matches.col]), g["pairs_seq12"])
    for a, b in zip(crossed.matches.data, by_host.matches.data):
        assert a.size > 0 and np.array_equal(a.uvs[0], b.uvs[0]) and np.array_equal(a.uvs[1], b.uvs[1])
    # convert_matches makes the camera coordinates on the device: the tolerance of tests/test_optimize_gpu.py for them
    model.filter_matches(min_weight=float(g["min_weight"]), clear_weights=True)
    model.convert_matches(optimize.RotationMatchesXYZ, clear_uvs=True)
    assert all(type(m) is optimize.RotationMatchesXYZ and m.uvs is None for m in model.matches.data)
    np.testing.assert_allclose(np.vstack([m.xys[0] for m in model.matches.data]), g["converted_xy_a"], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(np.vstack([m.xys[1] for m in model.matches.data]), g["converted_xy_b"], rtol=1e-11, atol=1e-12)
    # ObserverCameras with a matcher: build_matches, then fit on those matches
    matcher = mc.sequence_matcher(g)
    observer = optimize.ObserverCameras(glimpse_amd.Observer(list(matcher.images)))
    observer.matcher = matcher
    with contextlib.redirect_stdout(io.StringIO()):
        observer.build_matches(max_ratio=ratio, max_distance=None, seq=(1, 2))
        assert observer.matches is matcher.matches and len(observer.matches.data) == len(g["pairs_seq12"])
        assert all(type(m) is optimize.RotationMatchesXYZ for m in observer.matches.data)
        start = np.array([img.cam.viewdir for img in matcher.images])
        result = observer.fit(options={"maxiter": 3})
        with observer.upload() as handle:
            at_start, _ = observer.evaluate(handle, start)
    x = np.asarray(result.x).reshape(-1, 3)
    assert x.shape == (6, 3) and np.isfinite(x).all() and result.nit >= 1
    assert result.fun < at_start and np.abs(x - start).max() > 0  # the line search only accepts a smaller objective
