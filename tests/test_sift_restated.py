"""The SIFT rule itself (INPUTS.md, "SIFT: the rule"), held to account on its NumPy restatement (tests/sift_restated.py),
since cv2 is not there to compare with: a blob is found where it is and at its scale, the orientation turns with the image,
the descriptor recognises a turned image, and the host-side steps do what the rule says.  No GPU."""
import numpy as np
import pytest

from tests import sift_cases as sc
from tests import sift_restated as sr


@pytest.mark.parametrize("s", [2, 3, 4, 6])
def test_blob_is_found_at_its_place_and_scale(s):
    kps, desc = sr.detect(sc.blob(s))
    k = kps[np.argmax(kps[:, 4])]
    print(s, k.tolist())
    assert np.hypot(k[0] - 40.3, k[1] - 37.6) < 1.0
    ratio = k[2] / 2.0 / (0.9 * s)
    assert 2.0 ** (-1.0 / 3.0) < ratio < 2.0 ** (1.0 / 3.0)
    assert desc.dtype == np.uint8 and desc.shape == (len(kps), 128)


def _strongest_angles(img):
    kps, _ = sr.detect(img)
    return sorted(kps[kps[:, 4] == kps[:, 4].max()][:, 3].tolist())


def test_orientation_turns_with_the_image():
    """A fainter blob (half the amplitude) 6 px from the blob in the direction theta.  The pair is mirror-symmetric about
    its axis, so the strongest keypoint's histogram has TWO peaks of near-equal height, mirror images of each other, and
    both become keypoints (>= 0.8 max); which of them is the taller rests on the blob's sub-pixel centre, which does not
    turn with theta.  So every orientation of the strongest keypoint is compared: each must be an orientation at theta = 0
    turned by theta, within one histogram bin (10 degrees), and the other way round.  A wrong sign, a swapped axis or a
    missing `360 -` turns the set the other way or mirrors it, which this bound does not let through: the two peaks are
    about 95 and 262 degrees at theta = 0, not 180 apart."""
    def angles(theta):
        dx, dy = 6.0 * np.cos(np.radians(theta)), 6.0 * np.sin(np.radians(theta))
        return _strongest_angles(sc.blob(3, second=(dx, dy, 90.0)))

    def gap(a, b):
        return abs((a - b + 180.0) % 360.0 - 180.0)

    first = angles(0)
    assert len(first) == 2 and gap(first[0] + 180.0, first[1]) > 10.0
    for theta in (0, 90, 180, 270):
        found = angles(theta)
        print(theta, found)
        assert len(found) == len(first)
        for a in found:
            assert min(gap(a, b + theta) for b in first) <= 10.0
        for b in first:
            assert min(gap(a, b + theta) for a in found) <= 10.0
    # the turn has a sign: turned the other way, the orientations at 90 degrees do not fit
    assert max(min(gap(a, b - 90.0) for b in first) for a in angles(90)) > 10.0


def test_descriptor_recognises_a_turned_image():
    img = sc.texture(96, 96, seed=3)
    turned = np.rot90(img)  # turned[i, j] = img[j, 95 - i]
    ka, da = sr.detect(img)
    kb, db = sr.detect(turned)
    ka, da = ka[(ka[:, 5].astype(int) & 255) == 255], da[(ka[:, 5].astype(int) & 255) == 255]
    kb, db = kb[(kb[:, 5].astype(int) & 255) == 255], db[(kb[:, 5].astype(int) & 255) == 255]
    # a point (x, y) of img is at (y, 95 - x) of turned, in the coordinates of the doubled image's cells (pt = cell / 2)
    # at (y, 95.5 - x): the cell grid is half a pixel off the pixel grid
    back = np.stack([95.5 - kb[:, 1], kb[:, 0]], axis=1)
    d2 = ((da[:, None, :].astype(np.int64) - db[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
    nearest = d2.argmin(axis=1)
    pairs = hits = 0
    for i in range(len(ka)):
        near = np.hypot(back[:, 0] - ka[i, 0], back[:, 1] - ka[i, 1]) < 1.0
        near &= (kb[:, 2] / ka[i, 2] < 2.0 ** (1.0 / 3.0)) & (ka[i, 2] / kb[:, 2] < 2.0 ** (1.0 / 3.0))
        if near.any():
            pairs += 1
            hits += bool(near[nearest[i]])
    print(f"{hits} of {pairs} pairs ({len(ka)}, {len(kb)} keypoints): {hits / max(pairs, 1):.3f}")
    assert pairs >= 20
    assert hits >= pairs / 2


def test_order_duplicates_and_octave_packing():
    st = sc.stages("61x47")
    cells, kps = st["cells"], st["keypoints"]
    keys = [tuple(c) for c in cells.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    octave = kps[:, 5].astype(np.int64)
    assert np.array_equal(((octave & 255) + 1) & 255, cells[:, 0]) and np.array_equal((octave >> 8) & 255, cells[:, 1])
    assert np.all((octave >> 16) >= 0) and np.all((octave >> 16) <= 255)
    assert sr.pack_octave(0, 2, 0.25) == 255 | (2 << 8) | (191 << 16) and sr.pack_octave(3, 1, -0.5) == 2 | (1 << 8)
    # a keypoint equal to its predecessor in pt, size and angle is dropped (and only that one)
    twice = np.concatenate([kps[:3], kps[2:3], kps[3:]])
    desc = np.concatenate([st["descriptors"][:3], st["descriptors"][2:3], st["descriptors"][3:]])
    k, d = sr.finish(twice, desc)
    k0, d0 = sr.finish(kps, st["descriptors"])
    assert np.array_equal(k, k0) and np.array_equal(d, d0) and len(k0) == len(kps)


def test_mask_nfeatures_and_empty():
    st = sc.stages("61x47")
    kps, desc = st["keypoints"], st["descriptors"]
    mask = sc.mask_of("61x47")
    k, d = sr.finish(kps, desc, mask=mask)
    inside = np.array([mask[int(v + 0.5), int(u + 0.5)] != 0 for u, v in kps[:, :2]])
    assert 0 < inside.sum() < len(kps)
    assert np.array_equal(k, kps[inside]) and np.array_equal(d, desc[inside])
    k, d = sr.finish(kps, desc, nfeatures=10)
    assert len(k) == 10 and np.all(np.diff([np.flatnonzero((kps == row).all(axis=1))[0] for row in k]) > 0)
    assert k[:, 4].min() >= np.sort(kps[:, 4])[-10]
    tie = kps.copy()
    tie[:, 4] = 1.0
    assert np.array_equal(sr.finish(tie, desc, nfeatures=4)[0], tie[:4])
    assert sr.detect(np.zeros((5, 5), np.uint8)) == (None, None)
    assert sr.octave_sizes(5, 5) == [] and sr.octave_sizes(6, 6) == [(12, 12)]


def test_root_descriptors():
    """root-SIFT (Arandjelovic & Zisserman 2012): the square root of the L1-normalised descriptor, in float32."""
    desc = sc.stages("61x47")["descriptors"]
    block = np.concatenate([desc[:12], np.zeros((1, 128), np.uint8)])
    root = sr.root_descriptors(block)
    assert root.dtype == np.float32 and root.shape == block.shape
    assert np.all(root[block == 0] == 0.0) and np.all(root[block > 0] > 0.0) and np.all(root[-1] == 0.0)
    # unit L2 norm (the L1 norm of the squares is 1): float32 rounding of 128 terms, and 1e-7 against sums of ~2000
    assert np.allclose((root[:-1].astype(np.float64) ** 2).sum(axis=1), 1.0, rtol=0, atol=128 * 2.0 ** -23)
    # the order of the elements of a row is kept: a larger integer gives a root at least as large
    for row, r in zip(block[:-1], root[:-1]):
        order = np.argsort(row, kind="stable")
        assert np.all(np.diff(r[order]) >= 0.0)
        assert np.all(r[order][np.diff(row[order], prepend=row[order][0]) > 0] > 0.0)
    # against the expression itself in float64 (float32 result: half an ulp of each operation)
    exact = np.sqrt(block[:-1] / (block[:-1].sum(axis=1, keepdims=True) + 1e-7))
    assert np.allclose(root[:-1], exact, rtol=4 * 2.0 ** -24, atol=0)


def test_the_images_of_the_gpu_test_meet_its_conditions():
    """What tests/test_gpu_sift.py asserts before it compares, checked here without a device."""
    for name in sc.FULL:
        st = sc.stages(name)
        trace = st["trace"]
        print(name, len(st["candidates"]), len(st["keypoints"]), trace)
        assert len(st["keypoints"]) >= 30 and len(trace["octaves"]) >= 3
        for what in ("moved", "contrast", "edge", "border", "two_orientations", "clipped"):
            assert trace[what] >= 1, (name, what)


def test_the_large_image_overflows_a_fresh_candidate_list_and_the_others_do_not():
    """ "300x400" is there for the second attempt of the device's candidate list (sc.LIST_SLOTS slots on a fresh handle);
    "61x47", which the reuse test runs before and after it, must fit the first."""
    st = sc.stages("300x400")
    print("300x400:", len(st["candidates"]), "candidates,", len(st["keypoints"]), "keypoints")
    assert sc.LIST_SLOTS == 4096 and len(st["candidates"]) > 4096
    assert (len(st["candidates"]), len(st["keypoints"])) == (4446, 1608)  # (the figures of INPUTS.md)
    assert len(st["keypoints"]) <= 2 * len(st["candidates"]) + 64  # (the keypoint list's own second attempt is not reached)
    for name in ("61x47", "47x61", "256x192", "strip"):
        assert len(sc.stages(name)["candidates"]) < sc.LIST_SLOTS, name


def test_the_ends_of_the_layer_range_meet_the_conditions_of_the_gpu_test():
    """nOctaveLayers 1 and 8 on the images tests/test_gpu_sift.py runs them on: enough keypoints for the sweep's floor,
    keypoints of the last layer (8) and of more than one octave, all S + 3 tables, and the radii that fold the strip's
    reflection more than once."""
    for name in ("61x47", "47x61"):
        for params in ({"nOctaveLayers": 1}, {"nOctaveLayers": 8}, {"nOctaveLayers": 8, "sigma": 2.4}):
            st = sc.stages(name, **params)
            kept = sr.finish(st["keypoints"], st["descriptors"])[0]
            print(name, params, len(st["candidates"]), "candidates,", len(kept), "keypoints")
            assert len(kept) >= 5
            layers = set(st["cells"][:, 1].tolist())
            assert layers == {1} if params["nOctaveLayers"] == 1 else (8 in layers and len(layers) >= 7)
            assert np.array_equal((st["keypoints"][:, 5].astype(np.int64) >> 8) & 255, st["cells"][:, 1])
    assert len(sr.finish(*[sc.stages("47x61", nOctaveLayers=8)[k] for k in ("keypoints", "descriptors")])[0]) == 64
    assert len(sr.finish(*[sc.stages("47x61", nOctaveLayers=1)[k] for k in ("keypoints", "descriptors")])[0]) == 16
    for name, layers in (("47x61", 8), ("strip", 8), ("strip", 1)):
        st = sc.stages(name, nOctaveLayers=layers)
        assert all(len(g) == layers + 3 and len(d) == layers + 2 for g, d in zip(st["gauss"], st["dog"]))
        assert len(st["gauss"]) >= 2 and len(st["candidates"]) >= 1
        assert layers == 1 or (len(st["candidates"]) >= 5 and len(st["keypoints"]) >= 1)  # (one layer: for the pyramid)
    assert len(sr.tables(8, 1.6)) == 11 and [r for r, _ in sr.tables(1, 1.6)] == [5, 11, 22, 45]
    assert sc.stages("strip", nOctaveLayers=1)["gauss"][1][0].shape == (40, 12)  # radius 45 over 12 cells: four folds
    assert max(r for r, _ in sr.tables(8, 1.6)) == 6  # (with eight layers the blurs are narrow: no fold past the first)


def test_elementary_functions_are_close_to_the_library():
    """They are the rule's own (determinism is what counts), but they must still be the functions they are named for."""
    x = np.linspace(-60.0, 3.0, 2001)
    assert np.allclose(sr.exp_own(x), np.exp(x), rtol=1e-14, atol=0)
    assert sr.exp_own(-800.0) == 0.0
    t = np.radians(np.arange(0.0, 360.0, 0.5))
    got = sr.atan2_own(np.sin(t), np.cos(t))
    assert np.max(np.abs((got - np.degrees(t) + 180.0) % 360.0 - 180.0)) < 0.02  # (the polynomial's own error)
    for deg in np.arange(0.0, 360.5, 0.5):
        s, c = sr.sincos_own(float(deg))
        assert abs(s - np.sin(np.radians(deg))) < 1e-15 and abs(c - np.cos(np.radians(deg))) < 1e-15
