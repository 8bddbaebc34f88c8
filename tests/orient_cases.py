"""What tests/test_optimize_host.py and tests/test_optimize_gpu.py share: the fixtures of tools/make_golden_orient.py
(tests/golden/orient_sequence.npz, orient_chunks.npz) as the restatement's pairs and as glimpse_amd objects."""
import datetime

import numpy as np

FIXTURES = ("orient_sequence.npz", "orient_chunks.npz")
U = 2.0 ** -53


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
