"""The few functions of the reference's src/glimpse/helpers.py that the host-side raster logic needs, restated."""
import numpy as np


def intersect_boxes(boxes):
    """Intersection of boxes, each (xmin, ..., xmax, ...) (helpers.py:1264-1291); NaN entries are ignored."""
    boxes = np.asarray(boxes)
    if boxes.shape[1] % 2 != 0:
        raise ValueError("Box lengths are not divisible by 2")
    ndim = boxes.shape[1] // 2
    boxmin = np.nanmax(boxes[:, 0:ndim], axis=0)
    boxmax = np.nanmin(boxes[:, ndim:], axis=0)
    if any(boxmax - boxmin <= 0):
        raise ValueError("Boxes do not intersect")
    return np.hstack((boxmin, boxmax))
