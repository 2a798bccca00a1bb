"""savsr_amd.frames.plane_table: where the byte matrices of every frame kind lie.  Every layout x depth at the sizes where chroma
rounding and block alignment go wrong (odd heights and widths), against yuv.frame_bytes, yuv.chroma_hw and active.block_of; and the
packed table.  CPU only."""
import pytest

from savsr_amd import active, yuv
from savsr_amd.frames import Plane, detector_side, plane_table

FORMAT_OF = {"400": "y400", "420": "i420", "422": "i422", "444": "i444"}
SIZES = [(2, 2), (5, 3), (3, 5)]


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("layout", ["400", "420", "422", "444"])
def test_planar_tables_are_contiguous_and_sized_by_the_layout(layout, depth, h, w):
    side, size = detector_side(FORMAT_OF[layout], (h, w), depth)
    assert side.layout == layout and size == (h, w)
    tab = plane_table(side, size)
    s = 1 if depth == 8 else 2
    assert tab.sample == s and tab.stride == yuv.frame_bytes(h, w, depth, layout) == side.frame_bytes(h, w)
    assert len(tab.planes) == (1 if layout == "400" else 3)
    assert tab.planes[0] == Plane(0, h, w * s, 1, 1)                                  # the Y matrix
    end = 0
    for p in tab.planes:                                                              # in order, nothing between them
        assert p.offset == end and p.rows >= 1 and p.row_bytes >= s
        end += p.rows * p.row_bytes
    assert end == yuv.frame_bytes(h, w, depth, layout)                                # the last plane ends the frame
    for p in tab.planes[1:]:                                                          # U, V
        assert (p.rows, p.row_bytes // s) == yuv.chroma_hw(h, w, layout) and p.row_bytes % s == 0
        assert (p.bv, p.bh) == active.block_of(layout)
    assert plane_table(side, size, 3, 99, 99) == tab                                  # c, h, w are not read for planar frames


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("c", [1, 2, 3])
def test_packed_table_is_one_matrix(c, h, w):
    side, size = detector_side("rgb", None, 8)
    assert size is None and side.layout is None
    tab = plane_table(side, size, c, h, w)
    assert tab == (h * w * c, 1, (Plane(0, h, w * c, 1, 1),))
    assert (tab.planes[0].bv, tab.planes[0].bh) == active.block_of(None)
