"""The opt-in surface of optimize.SIFT that needs no device: what is refused and how, and the KeyPoint tuple."""
import numpy as np
import pytest

from glimpse_amd import helpers, optimize


def test_default_method_still_refuses():
    with pytest.raises(NotImplementedError, match="keypoint detection .SIFT of cv2. is not served.*method=optimize.SIFT"):
        optimize.detect_keypoints(np.zeros((8, 8)))
    with pytest.raises(NotImplementedError, match="keypoint detection .SIFT of cv2. is not served"):
        optimize.detect_keypoints(np.zeros((64, 64)), method=None, nOctaveLayers=2)


def test_unknown_keyword_and_method():
    with pytest.raises(TypeError):
        optimize.SIFT.create(nOctaves=4)
    with pytest.raises(TypeError):
        optimize.detect_keypoints(np.zeros((64, 64)), method=optimize.SIFT, blur=2)

    class ORB:
        @classmethod
        def create(cls, **kwargs):
            raise AssertionError("not reached")

    with pytest.raises(NotImplementedError, match="ORB.*is not served"):
        optimize.detect_keypoints(np.zeros((64, 64)), method=ORB)


def test_colour_array_is_refused():
    with pytest.raises(NotImplementedError, match="two-dimensional"):
        optimize.detect_keypoints(np.zeros((32, 32, 3)), method=optimize.SIFT)


def test_an_image_without_an_octave_is_empty_without_a_device():
    assert optimize.detect_keypoints(np.zeros((5, 5)), method=optimize.SIFT) == ([], None)
    assert optimize.detect_keypoints(np.zeros((5, 40)), method=optimize.SIFT, root=True) == ([], None)


def test_keypoint_pickles_and_points(tmp_path):
    kp = optimize.KeyPoint((12.5, 7.25), 3.2, 271.0, 0.03, 255 | (2 << 8) | (130 << 16), -1)
    assert kp.pt == (12.5, 7.25) and kp.size == 3.2 and kp.angle == 271.0 and kp.octave & 255 == 255 and kp.class_id == -1
    assert optimize._point(kp) == (12.5, 7.25)
    desc = np.arange(256, dtype=np.uint8).reshape(2, 128)
    helpers.write_pickle(([kp, kp._replace(pt=(1.0, 2.0))], desc), path=tmp_path / "k.pkl")
    kps, d = helpers.read_pickle(tmp_path / "k.pkl")
    assert kps[0] == kp and type(kps[0]) is optimize.KeyPoint and kps[1].pt == (1.0, 2.0) and np.array_equal(d, desc)


def test_create_keeps_its_arguments():
    s = optimize.SIFT.create(10, 2, 0.08, 5, 1.2)
    assert (s.nfeatures, s.nOctaveLayers, s.contrastThreshold, s.edgeThreshold, s.sigma) == (10, 2, 0.08, 5.0, 1.2)


def test_close_without_a_handle_and_context_manager():
    with optimize.SIFT.create() as s:
        assert s._handle is None
    s.close()
    s.close()
