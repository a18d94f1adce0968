"""The velocity planes' layout (tgnh_topology.cpp) on host-only handles: the planes hold the MASSIVE slots only, packed
in slot order wave tile by wave tile, every tile's segment beginning on a 128-byte line (16 words of 8 bytes: the planes exist in
mixed and double precision only).  A slot's word is at  base[tile] + offset[pattern][lane]  of each plane; topology(17) answers
the stride, the bases and the offsets, and everything here restates them in numpy from the descriptor's masses.

What the kernels rely on, and what is asserted: no two massive slots share a word, every word lies inside the stride (the planes
are allocated 3 x stride words), a tile's words lie in lines no other tile touches."""
import numpy as np
import pytest

from openmm_drudenose_amd import DrudeTGNHIntegrator, HostTopology
from massive_planes_boxes import NAMES, box, plane_layout

LINE = 16            # words of a 128-byte line


def layout_of(name, com=True):
    s, g, ng = box(name)
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, com)
    for _ in range(ng):
        it.addTempGroup()
    it._particleTempGroup = np.ascontiguousarray(g, np.int32)
    t = HostTopology(s, it, mode="TGNH")
    try:
        assert int(t.topology(16)[0]) == 1, "the box must qualify for the planes"
        wt = t.topology(9).reshape(-1, 2)[:, 0].astype(np.int64)
        wpat = t.topology(12).view(np.uint32)
        stride, bases, offsets = plane_layout(t)
        return s, wt, wpat, stride, bases, offsets
    finally:
        t.close()


@pytest.mark.parametrize("com", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_bases_offsets_and_stride(name, com):
    s, wt, wpat, stride, bases, offsets = layout_of(name, com)
    nw = len(wt) - 1
    massive = s.mass != 0.0
    assert len(bases) == nw + 1 and offsets.shape == (int((wpat >> 8).max()) + 1, 64)
    count = np.array([int(massive[wt[k]:wt[k + 1]].sum()) for k in range(nw)], np.int64)
    # every tile base a multiple of a line, and at least the previous base plus the previous tile's massive slots
    assert np.all(bases % LINE == 0) and bases[0] >= 0
    assert np.all(bases[1:] >= bases[:-1] + count)
    # the stride covers the last tile, is what the table's last entry says, and keeps the three planes line-aligned
    assert stride == bases[nw] and stride >= bases[nw - 1] + count[nw - 1] and stride % LINE == 0
    # ... and wastes less than a line per tile
    assert np.all(bases[1:] - bases[:-1] - count < LINE)
    # a lane's offset: the massive slots of its tile before it
    words = np.full(len(s.mass), -1, np.int64)
    for k in range(nw):
        ws, m = int(wt[k]), int(wt[k + 1] - wt[k])
        assert 0 < m <= 64 and int(wpat[k] & 255) > 0
        before = np.concatenate([[0], np.cumsum(massive[ws:ws + m])[:-1]])
        assert np.array_equal(offsets[int(wpat[k] >> 8)][:m], before), (name, k)
        words[ws:ws + m] = np.where(massive[ws:ws + m], bases[k] + before, -1)
    # no two massive slots share a word; every word inside the stride; slot order kept
    used = words[massive]
    assert len(used) == int(massive.sum()) and np.all(np.diff(used) > 0) and used[0] >= 0 and used[-1] < stride
    if massive.all():                                        # the compact layout is the identity inside a tile
        assert np.array_equal(offsets[:, :], np.tile(np.arange(64), (len(offsets), 1)))


def test_a_water_tile_is_three_lines_of_a_plane():
    """60 slots, 48 of them massive: 48 x 8 B = three 128-byte lines exactly, no padding between full tiles; the stride of the
    1001-molecule box is 83 x 48 + 32 (its last tile: 5 molecules = 20 massive slots, padded to two lines)"""
    s, wt, wpat, stride, bases, offsets = layout_of("water1001")
    assert np.array_equal(bases[:84], 48 * np.arange(84)) and stride == 83 * 48 + 32
    assert np.array_equal(offsets[0][:10], [0, 1, 2, 3, 4, 4, 5, 6, 7, 8])      # O, D, H1, H2, M | O ...


def test_the_massless_slot_fourth_of_five():
    s, wt, wpat, stride, bases, offsets = layout_of("nacl-order")
    assert np.array_equal(offsets[0][:10], [0, 1, 2, 3, 3, 4, 5, 6, 7, 7])      # O, H1, H2, M, D | O ...: not lane - lane div 5


def test_a_box_that_does_not_qualify_has_no_layout():
    from helpers import water_row
    s, g, ng = water_row("heavy-odd", 48)
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
    t = HostTopology(s, it, mode="dualNH")
    try:
        assert int(t.topology(16)[0]) == 0
        stride, bases, offsets = plane_layout(t)
        assert stride == 0 and len(bases) == 0 and offsets.shape == (0, 64)
    finally:
        t.close()
