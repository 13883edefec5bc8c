"""The level table the description kernels take by value (orbx_device.hpp: DescLevels, filled by makeDescLevels where installGeometry fills the
device's LevelGeom table) against that LevelGeom table, field by field, for the geometries tests/test_describe_chain.py runs on the GPU.  CPU only:
orbx_debug_describe_levels builds both on the host."""
import numpy as np
import pytest

import extractorb_amd as X

INT_MAX = 2 ** 31 - 1
GEOMETRIES = [(1, 63, 84), (2, 75, 100), (3, 90, 120), (8, 222, 296), (9, 267, 356), (16, 948, 1264), (8, 480, 640), (8, 1080, 1920), (12, 600, 800)]


@pytest.mark.parametrize("nlevels,rows,cols", GEOMETRIES)
@pytest.mark.parametrize("max_batch", [1, 3, 512])
def test_the_table_by_value_equals_the_level_geometry(nlevels, rows, cols, max_batch):
    n, desc, geom = X.describe_levels(rows, cols, 200, 1.2, nlevels, max_batch)
    assert n == nlevels
    for r, name in enumerate(X.DESCRIBE_LEVEL_FIELDS):
        assert desc[r, :nlevels].tolist() == geom[r, :nlevels].tolist(), name
    # what the kernel relies on: first slots ascending from 0 and even (the two keypoints of a wave share a level), INT_MAX behind the last level
    first = desc[0, :nlevels]
    assert first[0] == 0 and (np.diff(first) > 0).all() and (first % 2 == 0).all()
    assert (desc[0, nlevels:] == INT_MAX).all() and (desc[1:, nlevels:] == 0).all() and (geom[:, nlevels:] == 0).all()
    # widths, heights and strides of the reference's level sizes; the arena offsets of consecutive levels leave room for max_batch frames
    sizes = X.compute_level_sizes(rows, cols, 1.2, nlevels)
    assert [(int(w), int(h)) for w, h in zip(desc[1, :nlevels], desc[2, :nlevels])] == sizes
    assert (desc[3, :nlevels] % 64 == 0).all() and (desc[4, :nlevels] % 64 == 0).all()
    for off, per in ((5, 6), (7, 8)):
        assert (desc[off, 1:nlevels] >= desc[off, :nlevels - 1] + max_batch * desc[per, :nlevels - 1]).all()
    scale = desc[9, :nlevels].astype(np.uint32).view(np.float32)
    assert np.array_equal(scale, X.compute_tables(200, 1.2, nlevels)["scale_factors"])


@pytest.mark.parametrize("nlevels,rows,cols", GEOMETRIES[:6])
def test_the_smallest_frame_of_a_depth(nlevels, rows, cols):
    """the frames of tests/test_describe_chain.py are the smallest 4 : 3 frames (columns a multiple of 4) the geometry accepts for their depth"""
    assert rows == cols * 3 // 4
    with pytest.raises(X.OrbxError):
        X.describe_levels((cols - 4) * 3 // 4, cols - 4, 200, 1.2, nlevels, 1)


def test_bad_arguments():
    L = X.load_library()
    buf = np.zeros((11, 16), np.int64)
    import ctypes as C
    n = C.c_int()
    assert L.orbx_debug_describe_levels(200, 1.2, 0, 480, 640, 1, C.byref(n), buf.ctypes.data, buf.ctypes.data) == -2
    assert L.orbx_debug_describe_levels(200, 1.2, 17, 480, 640, 1, C.byref(n), buf.ctypes.data, buf.ctypes.data) == -2
    assert L.orbx_debug_describe_levels(200, 1.2, 8, 480, 640, 0, C.byref(n), buf.ctypes.data, buf.ctypes.data) == -2
    assert L.orbx_debug_describe_levels(200, 1.2, 8, 480, 640, 1, C.byref(n), None, buf.ctypes.data) == -2
    assert L.orbx_debug_describe_levels(200, 1.2, 8, 60, 80, 1, C.byref(n), buf.ctypes.data, buf.ctypes.data) == -5      # (too small: ORBX_ERR_IMAGE_TOO_SMALL)
