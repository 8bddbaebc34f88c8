"""What tests/test_calib_host.py and tests/test_gpu_calib.py share of the calibration whose row jobs are wider than a
workgroup of k_calib_rows (256 threads): a seeded model of three cameras with every kind of control, and `predicted` of a
control by the formulas of oracle/camera.py (float64 NumPy, none of the package's kernels).  No device is needed to build
the model: the rotation kinds are given camera coordinates, their image coordinates are made on the host."""
import functools

import numpy as np

from oracle import camera as oc

SEED = 11
POSITION = (10.0, 20.0, 30.0)  # of all three: the match kinds need one position
INTERNALS = dict(imgsz=(400, 300), f=(500, 505), c=(3, -2), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.003), p=(0.001, -0.002))
VIEWDIRS = ((5.0, 2.0, 1.0), (9.0, -1.0, -2.0), (81.0, 3.0, 0.5))  # camera 2 looks 72 degrees past camera 1
# (kind, cameras, rows) in control order: the Points, the match kinds and the Lines control interleave, so the workgroup
# lists of the three kernels do and no multi-workgroup job starts at row 0 of the output
CONTROLS = (("points", (0,), 1), ("matches", (1, 2), 257), ("points", (1,), 255), ("lines", (0,), 300),
            ("rotation", (0, 1), 1000), ("points", (2,), 256), ("rotation_xy", (0, 1), 257), ("points", (0,), 257),
            ("matches", (1, 2), 1000), ("rotation", (0, 1), 257), ("points", (1,), 600), ("rotation_xy", (0, 1), 1000))
BEHIND = {2: (3,), 7: (256,), 10: (255, 256, 300, 511, 512, 599)}  # control -> rows of Points behind the camera
FAR = {4: (5, 256, 700, 999), 6: (256,), 9: (100, 256), 11: (255, 256, 512, 768, 999)}  # control -> rows of far rays
TB = 256


def oracle_vectors():
    return [oc.make_camera(xyz=POSITION, viewdir=v, **INTERNALS) for v in VIEWDIRS]


def _rays(vector, xy):
    """World ray directions of camera coordinates: R^T [x, y, 1]."""
    return np.column_stack((xy, np.ones(len(xy)))) @ oc.rotation_matrix(vector[3:6])


def _far_side(vectors, target, other, x=40.0):
    """+1 or -1: the side of camera `other`'s x axis on which the ray (x, 0.1) (x = 40: 88.6 degrees off the axis) is
    behind camera `target`."""
    for s in (1.0, -1.0):
        if np.isnan(oracle_predicted("rotation_xy", vectors, (target, other), [None, np.array([[s * x, 0.1]])], 0)).all():
            return s
    raise AssertionError("no far ray of the other camera is behind the target")


def oracle_predicted(kind, vectors, cams, data, side=0):
    """`predicted` of a control by oracle/camera.py.  `data`: (xyz,) of Points; the two sides' image coordinates of
    Matches, camera coordinates of the rotation kinds.  `side`: which of the two cameras predicts."""
    if kind == "points":
        return oc.xyz_to_uv(vectors[cams[0]], data[0])
    target, other = vectors[cams[side]].copy(), vectors[cams[1 - side]]
    target[0:3] = 0  # (ray directions: nothing to subtract)
    rays = oc.uv_to_xyz(other, data[1 - side]) if kind == "matches" else _rays(other, data[1 - side])
    return oc.xyz_to_xy(target, rays) if kind == "rotation_xy" else oc.xyz_to_uv(target, rays)


@functools.lru_cache(maxsize=None)
def data():
    """[per control: the arrays `oracle_predicted` takes (Lines: (uv, world polyline))], seeded."""
    rng = np.random.default_rng(SEED)
    vectors = oracle_vectors()
    out = []
    for n, (kind, cams, rows) in enumerate(CONTROLS):
        if kind == "points":
            depth = rng.uniform(100.0, 1000.0, rows)
            depth[list(BEHIND.get(n, ()))] *= -1.0
            xyz = np.asarray(POSITION) + depth[:, None] * _rays(vectors[cams[0]], rng.uniform(-0.4, 0.4, (rows, 2)))
            out.append((xyz,))
        elif kind == "lines":
            x = np.linspace(-0.37, 0.36, 9)
            line = np.asarray(POSITION) + 1000.0 * _rays(vectors[cams[0]], np.column_stack((x, 0.03 * np.cos(7 * x) - 0.01)))
            out.append((np.column_stack((rng.uniform(20, 380, rows), rng.uniform(100, 200, rows))), line))
        else:
            xy = [rng.uniform(-0.38, 0.38, (rows, 2)), rng.uniform(-0.38, 0.38, (rows, 2))]
            if kind == "matches":  # image coordinates; a fifteenth of camera 2's field is behind camera 1, and the reverse
                xy[1][-1] = (_far_side(vectors, cams[0], cams[1], 0.375) * 0.375, 0.1)  # (the last row for certain)
                xy[0][-1] = (_far_side(vectors, cams[1], cams[0], 0.375) * 0.375, 0.1)
                xy = [oc.distort(vectors[c], p) * vectors[c][8:10] + (vectors[c][6:8] / 2 + vectors[c][10:12]) for c, p in zip(cams, xy)]
            else:  # camera coordinates; a few rays so far out that they are behind the other camera
                far = list(FAR[n])
                xy[1][far] = (_far_side(vectors, cams[0], cams[1]) * 40.0, 0.1)
                xy[0][far] = (_far_side(vectors, cams[1], cams[0]) * 40.0, 0.1)
            out.append(tuple(xy))
    for arrays in out:
        for a in arrays:
            a.setflags(write=False)
    return out


def model():
    """(Cameras with the view directions of all three cameras as parameters, its cameras): a new one every call."""
    import glimpse_amd
    from glimpse_amd import optimize

    cams = [glimpse_amd.Camera(xyz=POSITION, viewdir=v, **INTERNALS) for v in VIEWDIRS]
    rng = np.random.default_rng(SEED + 1)
    controls = []
    for (kind, members, rows), arrays in zip(CONTROLS, data()):
        if kind == "points":
            uv = rng.uniform(0, 400, (rows, 2))  # (the observed side plays no part in `predicted`)
            controls.append(optimize.Points(cams[members[0]], uv=uv, xyz=arrays[0]))
        elif kind == "lines":
            controls.append(optimize.Lines(cams[members[0]], uvs=[arrays[0]], xyzs=[arrays[1]]))
        elif kind == "matches":
            controls.append(optimize.Matches(cams=[cams[c] for c in members], uvs=list(arrays)))
        else:
            mtype = optimize.RotationMatches if kind == "rotation" else optimize.RotationMatchesXY
            controls.append(mtype(cams=[cams[c] for c in members], xys=list(arrays)))
    return optimize.Cameras(cams, controls, cam_params=[{"viewdir": True}] * 3), cams
