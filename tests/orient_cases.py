"""What tests/test_optimize_host.py and tests/test_optimize_gpu.py share: the fixtures of tools/make_golden_orient.py
(tests/golden/orient_sequence.npz, orient_chunks.npz) as the restatement's pairs and as glimpse_amd objects."""
import datetime
import functools

import numpy as np

FIXTURES = ("orient_sequence.npz", "orient_chunks.npz")
U = 2.0 ** -53


# The seeded sequences (`synthetic`): what tests/test_optimize_host.py asserts of each and tests/test_optimize_gpu.py runs.
SYNTHETIC = (256, 257, 300, 600)  # images: 1, 2, 2 and 3 workgroups of k_orient_reduce's image part
SYNTHETIC_SEED = 7
PAIR_SIZES = (0, 1, 255, 256, 257, 4095, 4096, 4097, 8193)  # either side of a lane turn (256) and of one and two chunks
HUB, HUB_PARTNERS = 100, 150  # the hub image and its pairs per side


def synthetic_isolated(n_images):
    """The images in no pair: 200, and one past the first workgroup's 256 where there is one (280, or the last image)."""
    return [200] + ([280] if n_images > 281 else [n_images - 1] if n_images > 256 else [])


def synthetic_viewdirs(n_images, seed=SYNTHETIC_SEED):
    """View directions (n, 3) spread over +-20 degrees of yaw and pitch and +-5 of roll."""
    rng = np.random.default_rng([seed, n_images])
    return rng.uniform(-1.0, 1.0, (n_images, 3)) * (20.0, 20.0, 5.0)


def synthetic_pair_list(n_images):
    """[(i, j)] of `synthetic` in COO order (by i, then j): the chain (i, i + 1), (i, i + 2) without the ISOLATED images,
    and the HUB image with HUB_PARTNERS images as i and as many as j (other images where there are enough of them, else
    some of the same images both ways round).  Image 0 is only ever i and the last image in a pair only ever j."""
    isolated = synthetic_isolated(n_images)
    pairs = {(i, i + d) for i in range(n_images) for d in (1, 2) if i + d < n_images}
    last = max(m for m in range(n_images) if m not in isolated)
    free = [m for m in range(1, last) if m != HUB and m not in isolated]
    as_i = free[-HUB_PARTNERS:]  # (HUB, m)
    rest = [m for m in free if m not in as_i]
    as_j = (rest if len(rest) >= HUB_PARTNERS else free)[:HUB_PARTNERS]  # (m, HUB)
    pairs |= {(HUB, m) for m in as_i} | {(m, HUB) for m in as_j}
    return sorted((i, j) for i, j in pairs if i not in isolated and j not in isolated)


def synthetic_sizes(n_pairs, rng):
    """Matches per pair: PAIR_SIZES at pairs 3 .. 11 and again from pair 260 (a lane's second turn), else 5 .. 35."""
    sizes = rng.integers(5, 36, n_pairs)
    sizes[3:3 + len(PAIR_SIZES)] = PAIR_SIZES
    sizes[260:260 + len(PAIR_SIZES)] = PAIR_SIZES
    return sizes


def synthetic(n_images, seed=SYNTHETIC_SEED, with_viewdirs=False):
    """(pairs, R, Rprime) of a seeded sequence of `n_images`: pairs = [(i, j, xy_i, xy_j)] of `synthetic_pair_list` with
    camera coordinates uniform in +-0.4 and noise of 0.01 (standard deviation) on the second side; R and Rprime are
    glimpse_amd.camera.rotations of `synthetic_viewdirs`."""
    from glimpse_amd.camera import rotations

    viewdirs = synthetic_viewdirs(n_images, seed)
    rng = np.random.default_rng([seed, n_images, 1])
    listed = synthetic_pair_list(n_images)
    pairs = []
    for (i, j), m in zip(listed, synthetic_sizes(len(listed), rng)):
        xy_i = rng.uniform(-0.4, 0.4, (m, 2))
        pairs.append((i, j, xy_i, xy_i + 0.01 * rng.standard_normal((m, 2))))
    R, Rprime = rotations(viewdirs)
    return (pairs, R, Rprime, viewdirs) if with_viewdirs else (pairs, R, Rprime)


def synthetic_probe(viewdirs, seed=SYNTHETIC_SEED):
    """View directions up to half a degree off `viewdirs`: a point at which the anchors' terms are not zero."""
    return viewdirs + np.random.default_rng([seed, len(viewdirs), 2]).uniform(-0.5, 0.5, viewdirs.shape)


def synthetic_observer(n_images, anchors=(0, 130)):
    """(ObserverCameras, pairs) of `synthetic(n_images)`, the matches as a dict of RotationMatchesXYZ (no device is needed
    to build them)."""
    import glimpse_amd
    from glimpse_amd import optimize

    case = synthetic_case(n_images)
    cams = [glimpse_amd.Camera(imgsz=(100, 80), f=(120, 120), viewdir=v) for v in case["viewdirs"]]
    images = [glimpse_amd.Image(cam=cam, array=np.zeros((2, 2), np.uint8),
                                datetime=datetime.datetime(2020, 1, 1) + datetime.timedelta(hours=n))
              for n, cam in enumerate(cams)]
    matches = {(i, j): optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], xys=[xy_i, xy_j]) for i, j, xy_i, xy_j in case["pairs"]}
    return optimize.ObserverCameras(glimpse_amd.Observer(images), matches=matches, anchors=list(anchors)), case["pairs"]


def flat(pairs):
    """(pair_i, pair_j, offsets, xy_i, xy_j) as `_lib.Orient` takes them."""
    offsets = np.concatenate(([0], np.cumsum([len(p[2]) for p in pairs]))).astype(np.int64)
    return ([p[0] for p in pairs], [p[1] for p in pairs], offsets,
            np.concatenate([np.empty((0, 2))] + [p[2] for p in pairs]), np.concatenate([np.empty((0, 2))] + [p[3] for p in pairs]))


def longdouble_evaluate(n_images, pairs, R, Rprime):
    """The objective and gradient of `pairs` with plain matrix products and plain sums in np.longdouble: no chunk, lane
    or wave in it.  Returns (objective, gradient (n, 3), addends (n, 3): how many match addends feed each entry)."""
    L = np.longdouble
    objective, gradient, addends = L(0), np.zeros((n_images, 3), L), np.zeros((n_images, 3), np.int64)
    for i, j, xy_i, xy_j in pairs:
        if not len(xy_i):
            continue
        a = np.column_stack((xy_i, np.ones(len(xy_i)))).astype(L)
        b = np.column_stack((xy_j, np.ones(len(xy_j)))).astype(L)
        di, dj = a @ R[i].astype(L), b @ R[j].astype(L)  # rows: R^T [x, y, 1]
        di, dj = di / np.sqrt((di * di).sum(axis=1))[:, None], dj / np.sqrt((dj * dj).sum(axis=1))[:, None]
        d = di - dj
        objective = objective + np.abs(d).sum()
        g = np.einsum("mr,rwk,mk->w", np.sign(d), Rprime[i].astype(L), a)
        gradient[i] += g
        gradient[j] -= g
        addends[i] += len(xy_i)
        addends[j] += len(xy_i)
    return objective, gradient, addends


def longdouble_bounds(details, addends):
    """(objective's, gradient's (n, 3)) bound on |float64 evaluation - longdouble_evaluate|, u = 2^-53:
    u (n_adds sum |addend| + 32 matches) with n_adds = matches the number of match addends that feed the output.  The
    first term is the bound of recursive summation in any order; the second allows 32 u for the evaluation of an addend
    (ray components of magnitude <= 1 from about ten roundings each, three of them per addend)."""
    M = details["matches"]
    return U * (M * details["abs_objective"] + 32 * M), U * (addends * details["abs_gradient"] + 32 * addends)


def longdouble_ratios(found, exact, details):
    """The errors of `found` = (objective, gradient) against `exact` of longdouble_evaluate, and the largest of them as a
    multiple of u sum |addend|: (error, ratio) of the objective, (errors (n, 3), largest ratio) of the gradient."""
    err_o = abs(float(np.longdouble(found[0]) - exact[0]))
    err_g = np.abs((found[1].astype(np.longdouble) - exact[1]).astype(np.float64))
    some = details["abs_gradient"] > 0
    return (err_o, err_o / (U * details["abs_objective"])), (err_g, float((err_g[some] / (U * details["abs_gradient"][some])).max()))


@functools.lru_cache(maxsize=None)
def synthetic_case(n_images):
    """`synthetic(n_images)` with its view directions, the restatement's result and details and the longdouble result,
    computed once a session (shared: read, never written)."""
    from tests import orient_restated as rs

    pairs, R, Rprime, viewdirs = synthetic(n_images, with_viewdirs=True)
    details = {}
    want = rs.evaluate(n_images, pairs, R, Rprime, details)
    exact = longdouble_evaluate(n_images, pairs, R, Rprime)
    return dict(pairs=pairs, R=R, Rprime=Rprime, viewdirs=viewdirs, want=want, details=details, exact=exact)


def internals(g):
    v = g["internals"]
    return dict(imgsz=v[0:2], f=v[2:4], c=v[4:6], k=v[6:12], p=v[12:14])


def pairs_of(g):
    """[(i, j, xy_i, xy_j)] in COO order, on the reference's camera coordinates."""
    off = g["offsets"]
    return [(int(i), int(j), g["xy_i"][off[p]:off[p + 1]], g["xy_j"][off[p]:off[p + 1]])
            for p, (i, j) in enumerate(zip(g["pair_i"], g["pair_j"]))]


def observer_of(g):
    """(ObserverCameras, its cameras) at the fixture's start view directions, the matches as a dict of
    RotationMatchesXYZ built from the reference's camera coordinates (no device is needed to build them)."""
    import glimpse_amd
    from glimpse_amd import optimize

    cams = [glimpse_amd.Camera(viewdir=v, **internals(g)) for v in g["viewdirs_start"]]
    images = [glimpse_amd.Image(cam=cam, array=np.zeros((2, 2), np.uint8),
                                datetime=datetime.datetime(2020, 1, 1) + datetime.timedelta(hours=n))
              for n, cam in enumerate(cams)]
    matches = {(i, j): optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], xys=[xy_i, xy_j])
               for i, j, xy_i, xy_j in pairs_of(g)}
    model = optimize.ObserverCameras(glimpse_amd.Observer(images), matches=matches, anchors=[int(a) for a in g["anchors"]])
    return model, cams
