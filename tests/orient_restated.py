"""The arithmetic of `glh_orient_eval` (glimpse_amd/csrc/glh_orient.hip) restated in NumPy, operation by operation and sum
by sum in the kernel's order, so that the device must equal it in every bit; and the callback of
`optimize.ObserverCameras.fit` built on it.  Products and sums are written out element by element (no matmul, whose BLAS
may contract or reassociate).

Order of the sums ("Sequence orientation"):
  * a pair's matches are cut into chunks of CHUNK; in a chunk, lane t of 256 adds the addends of matches t, t + 256, ...
    in order to a sum that starts at +0;
  * the 256 sums are added by `block_sum`: within each wave of 64 a butterfly (lane ^ 32, 16, 8, 4, 2, 1), then
    ((w0 + w1) + w2) + w3 over the waves;
  * a pair is the sum of its chunks in order from +0; an image's gradient walks the pairs in COO order, + where the image
    is i and - where it is j, from +0; the objective is lane t's sum over pairs t, t + 256, ... followed by `block_sum`.
"""
import numpy as np

CHUNK = 4096
TB = 256
WAVE = 64
_LANE = np.arange(WAVE)


def block_sum(v):
    """The workgroup's sum of `v` (256,) as thread 0 ends up with it."""
    w = np.asarray(v, dtype=np.float64).reshape(TB // WAVE, WAVE)
    off = WAVE // 2
    while off:
        w = w + w[:, _LANE ^ off]
        off //= 2
    total = w[0, 0]
    for k in range(1, TB // WAVE):
        total = total + w[k, 0]
    return total


def lane_sums(addends):
    """`addends` (m,), m <= CHUNK, of one chunk -> the 256 lanes' running sums (missing matches add nothing: +0)."""
    rounds = -(-len(addends) // TB) if len(addends) else 0
    padded = np.zeros(rounds * TB)
    padded[:len(addends)] = addends
    acc = np.zeros(TB)
    for r in range(rounds):
        acc = acc + padded[r * TB:(r + 1) * TB]
    return acc


def rays(R, xy):
    """Unit ray directions (m, 3) of camera coordinates `xy` (m, 2): R^T [x, y, 1] times 1 / sqrt((a^2 + b^2) + c^2)."""
    x, y = xy[:, 0], xy[:, 1]
    d = [(R[0, k] * x + R[1, k] * y) + R[2, k] for k in range(3)]
    inv = 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return [d[k] * inv for k in range(3)]


def match_addends(Ri, Rj, Rprime_i, xy_i, xy_j):
    """Per match of a pair: the objective's addend (m,), the gradient's (3, m), and d_i - d_j (3, m)."""
    di, dj = rays(Ri, xy_i), rays(Rj, xy_j)
    dxyz = [di[r] - dj[r] for r in range(3)]
    objective = (np.abs(dxyz[0]) + np.abs(dxyz[1])) + np.abs(dxyz[2])
    sign = [np.sign(v) for v in dxyz]
    x, y = xy_i[:, 0], xy_i[:, 1]
    gradient = []
    for w in range(3):
        t = [sign[r] * ((Rprime_i[r, w, 0] * x + Rprime_i[r, w, 1] * y) + Rprime_i[r, w, 2]) for r in range(3)]
        gradient.append((t[0] + t[1]) + t[2])
    return objective, np.array(gradient).reshape(3, -1), np.array(dxyz).reshape(3, -1)


def evaluate(n_images, pairs, R, Rprime, details=None):
    """(objective, gradient (n_images, 3)) of `pairs` = [(i, j, xy_i (m, 2), xy_j (m, 2))] in COO order at the rotation
    matrices `R` (n, 3, 3) and derivatives `Rprime` (n, 3, 3, 3).  `details` (a dict) receives what the bounds of the
    tests are made of: sum |addend| of the objective and of the gradient, the number of matches and min |d_i - d_j|."""
    sums = []
    abs_objective, abs_gradient, smallest, total = 0.0, np.zeros((n_images, 3)), np.inf, 0
    for i, j, xy_i, xy_j in pairs:
        xy_i, xy_j = np.asarray(xy_i, dtype=np.float64).reshape(-1, 2), np.asarray(xy_j, dtype=np.float64).reshape(-1, 2)
        pair = np.zeros(4)
        if len(xy_i):
            o, g, dxyz = match_addends(R[i], R[j], Rprime[i], xy_i, xy_j)
            rows = np.vstack((o[None], g))
            for start in range(0, len(xy_i), CHUNK):
                part = np.array([block_sum(lane_sums(rows[q, start:start + CHUNK])) for q in range(4)])
                pair = pair + part
            abs_objective += float(np.sum(np.abs(o)))
            abs_gradient[i] += np.sum(np.abs(g), axis=1)
            abs_gradient[j] += np.sum(np.abs(g), axis=1)
            smallest = min(smallest, float(np.min(np.abs(dxyz))))
            total += len(xy_i)
        sums.append(pair)
    gradient = np.zeros((n_images, 3))
    for (i, j, _, _), pair in zip(pairs, sums):
        gradient[i] = gradient[i] + pair[1:]
        gradient[j] = gradient[j] - pair[1:]
    lanes = np.zeros(TB)
    for p, pair in enumerate(sums):
        lanes[p % TB] = lanes[p % TB] + pair[0]
    if details is not None:
        details.update(abs_objective=abs_objective, abs_gradient=abs_gradient, min_abs_dxyz=smallest, matches=total)
    return block_sum(lanes), gradient


def anchor_terms(viewdirs, viewdirs_0, anchors, anchor_weight):
    """The anchors' part of the objective and gradient, as optimize.py:2052-2056 forms it."""
    objective = 0
    gradients = np.zeros(viewdirs.shape)
    for i in anchors:
        objective += (anchor_weight / 2.0) * np.sum((viewdirs[i] - viewdirs_0[i]) ** 2)
        gradients[i] += anchor_weight * (viewdirs[i] - viewdirs_0[i])
    return objective, gradients


def callback(viewdirs, viewdirs_0, anchors, anchor_weight, pairs, rotations, details=None):
    """(objective, gradient (n, 3)) of ObserverCameras.fit's callback at `viewdirs` (n, 3): the anchor terms first, then
    the matches.  `rotations`: viewdirs -> (R, Rprime) (glimpse_amd.camera.rotations)."""
    viewdirs = np.asarray(viewdirs, dtype=np.float64).reshape(-1, 3)
    a_objective, a_gradient = anchor_terms(viewdirs, viewdirs_0, anchors, anchor_weight)
    R, Rprime = rotations(viewdirs)
    m_objective, m_gradient = evaluate(len(viewdirs), pairs, R, Rprime, details)
    if details is not None:
        details.update(anchor_objective=a_objective, anchor_gradient=a_gradient, match_objective=m_objective,
                       match_gradient=m_gradient)
    return a_objective + m_objective, a_gradient + m_gradient


def fit(viewdirs_start, viewdirs_0, anchors, anchor_weight, pairs, rotations, method="bfgs", **kwargs):
    """scipy.optimize.minimize driven by `callback`, as ObserverCameras.fit drives it by the device."""
    import scipy.optimize

    def fun(x):
        objective, gradient = callback(x, viewdirs_0, anchors, anchor_weight, pairs, rotations)
        return objective, gradient.ravel()

    return scipy.optimize.minimize(fun=fun, x0=np.asarray(viewdirs_start, dtype=np.float64).ravel(), jac=True,
                                   method=method, **kwargs)
