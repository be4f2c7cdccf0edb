"""tests/wino_walk.py, the host mirror of wino_pc.hpp's tile list (pc_tile_share, pc_decode), by itself: the walks partition the list,
grid_for() meets the preconditions of the walking tests on 256 CUs, which tile fields can change along a walk for which workgroup
counts, and that a dropped next-tile book hand-over is visible in the words a second tile reads.  No GPU."""
import pytest

import wino_walk as ww

GRIDS = [8, 32, 38, 256, 304]
NTILES = [1, 7, 8, 9, 37, 56, 255, 256, 257, 400, 511, 512, 560, 616, 672, 900, 1001, 2431]

# (name, ncg, kd, dil, H, W) of the walking launches of test_gpu_wino_pc_walk.py
LAUNCHES = [("64 columns", 1, 1, 1, 50, 120), ("128 -> 128", 2, 1, 1, 50, 120), ("deconv", 4, 1, 1, 50, 120),
            ("dilation 2, 128 -> 128", 2, 1, 2, 50, 120), ("dilation 2, 64 columns", 1, 1, 2, 50, 120), ("kd = 3", 1, 3, 1, 38, 70)]


@pytest.mark.parametrize("G", GRIDS)
def test_walks_cover_the_tile_list_exactly_once(G):
    for ntiles in NTILES:
        ws = ww.walks(ntiles, G)
        assert len(ws) == min(ntiles, G)
        seen = sorted(t for w in ws for t in w)
        assert seen == list(range(ntiles)), (G, ntiles)
        for b, w in enumerate(ws):      # a walk is what (first, step, end) says, in ascending order
            first, step, end = ww.share(ntiles, min(ntiles, G), b)
            assert w == list(range(first, end, step)) and step > 0


def test_share_is_the_xcd_split_only_for_multiples_of_8():
    assert ww.share(616, 256, 0) == (0, 32, 77) and ww.share(616, 256, 9) == (78, 32, 154) and ww.share(616, 256, 255) == (539 + 31, 32, 616)
    assert ww.share(616, 38, 5) == (5, 38, 616) and ww.share(616, 304, 303) == (539 + 37, 38, 616)
    assert ww.share(5, 5, 3) == (3, 5, 5)


def test_decode_fields():
    N, H, W = 3, 50, 120                                          # 7 x 8 tiles: the last row and the last column cross the edge
    assert ww.plane_tiles(H, W) == (7, 8) and ww.spatial_tiles(N, H, W) == 168
    t = ww.decode(2 * (56 + 8 * 6 + 7) + 1, N, H, W, 2)           # sample 1, tile row 6, tile column 7, column group 1
    assert t == ww.Tile(1, 48, 112, 0, 0, 1, 111, False)
    assert ww.decode(0, N, H, W, 1).inside and not ww.decode(7, N, H, W, 1).inside and not ww.decode(48, N, H, W, 1).inside
    assert ww.plane_tiles(H, W, 2) == (4, 4) and ww.spatial_tiles(N, H, W, 2) == 192
    t = ww.decode(2 * (64 + 4 * (4 * 1 + 2) + 3) + 0, N, H, W, 2, 1, 2)   # sample 1, tile (1, 2), parity (1, 1), column group 0
    assert t == ww.Tile(1, 16, 64, 1, 1, 0, 91, True)
    # dilation 2: an interior test per parity (a tile whose odd lattice ends beyond the image takes the edge body, its even one not)
    assert ww.decode(4 * (4 * 3 + 0) + 0, 1, 63, 120, 1, 1, 2).inside and not ww.decode(4 * (4 * 3 + 0) + 2, 1, 63, 120, 1, 1, 2).inside
    t = ww.decode(5 + 7 * (3 + 5 * 2), 7, 38, 70, 1, 3, 1)        # kd = 3: depth fastest; slice 5, tile (2, 3)
    assert t == ww.Tile(5, 16, 48, 0, 0, 0, 96, True)


@pytest.mark.parametrize("name,ncg,kd,dil,H,W", LAUNCHES)
def test_grid_for_meets_its_preconditions_on_256_cus(name, ncg, kd, dil, H, W):
    n = ww.grid_for(256, ncg, kd, dil, H, W)
    pre = ww.preconditions(256, n, H, W, ncg, kd, dil)
    assert all(pre.values()), (name, n, pre)
    assert n == 1 or not all(ww.preconditions(256, n - 1, H, W, ncg, kd, dil).values())      # the smallest one
    lens = [len(w) for w in ww.walks(ww.launch_tiles(n, H, W, ncg, dil), 256)]
    assert min(lens) == 2 and max(lens) == 3, (name, n)
    if kd != 3:
        assert ww.launch_tiles(1, H, W, ncg, dil) <= 256          # a launch per sample: one tile per workgroup


def test_grid_for_values_on_256_cus():
    """The grids the walking tests run on an MI355X (256 CUs), pinned so that a change of the mirror shows."""
    got = {name: ww.grid_for(256, ncg, kd, dil, H, W) for name, ncg, kd, dil, H, W in LAUNCHES}
    assert got == {"64 columns": 10, "128 -> 128": 5, "deconv": 3, "dilation 2, 128 -> 128": 5, "dilation 2, 64 columns": 9, "kd = 3": 21}
    assert ww.launch_tiles(10, 50, 120, 1) == 560 and ww.launch_tiles(5, 50, 120, 2) == 560 and ww.launch_tiles(3, 50, 120, 4) == 672
    assert ww.launch_tiles(5, 50, 120, 2, 2) == 640 and ww.launch_tiles(21, 38, 70, 1) == 525


def test_kd3_plane_of_20_tiles_never_walks_from_an_edge_tile_to_an_interior_one():
    """Why the kd = 3 walking test does not use a 30 x 70 plane (4 x 5 tiles): depth runs fastest, so a walk leaves an edge tile for an
    interior one only at the end of a tile row, position 5 j D of the list — and with 20 D tiles the XCD eighths end at the multiples
    of 2.5 D: every such position is the end of a share.  No depth makes that launch meet the preconditions."""
    for D in range(1, 120):
        assert not ww.preconditions(256, D, 30, 70, 1, 3, 1)["edge_in"], D
    with pytest.raises(ValueError):
        ww.grid_for(256, 1, 3, 1, 30, 70, limit=120)


def _fields_that_change(G, ntiles, N, H, W, ncg, kd, dil):
    out = set()
    for w in ww.walks(ntiles, G):
        for a, b in zip(w, w[1:]):
            ta, tb = ww.decode(a, N, H, W, ncg, kd, dil), ww.decode(b, N, H, W, ncg, kd, dil)
            out |= {f for f in ("cg", "py", "px") if getattr(ta, f) != getattr(tb, f)}
    return out


@pytest.mark.parametrize("G", GRIDS)
def test_which_fields_change_along_a_walk(G):
    """The column group (1, 2 or 4 per tile; the deconv form's phase is the column group of its four) changes along a walk exactly when
    the stride is no multiple of the group count, the dilation parity (above the column group in the list index) exactly when it is no
    multiple of 4 ncg.  G % 32 == 0: the stride G / 8 is a multiple of 4, so column group and phase are the same all along every walk —
    a weight stream of another column group behind a tile's last stage, and nph != PH in pc_dc_tile, are never executed; the parity
    still changes for 32 workgroups with two column groups, not for 256.  G = 38 and G = 304 (stride 38) change phase and parity."""
    H, W = 50, 120
    for ncg, dil, N in ((1, 1, 11), (2, 1, 6), (4, 1, 3), (1, 2, 9), (2, 2, 5)):
        ntiles = ww.launch_tiles(N, H, W, ncg, dil)
        assert ntiles > G
        changed = _fields_that_change(G, ntiles, N, H, W, ncg, 1, dil)
        step = ww.share(ntiles, G, 0)[1]
        assert step == (G // 8 if G % 8 == 0 else G)
        assert ("cg" in changed) == (step % ncg != 0), (G, ncg, dil, changed)
        assert bool(changed & {"py", "px"}) == (dil == 2 and step % (4 * ncg) != 0), (G, ncg, dil, changed)
        if G % 32 == 0:
            assert step % 4 == 0 and "cg" not in changed
        if G == 256:        # this device: a walking launch has one workgroup per CU and keeps column group, phase and parity
            assert not changed, (ncg, dil, changed)
    if G in (38, 304):
        assert "cg" in _fields_that_change(G, 672, 3, H, W, 4, 1, 1)                      # the deconv form's phase
        assert _fields_that_change(G, 640, 5, H, W, 2, 1, 2) & {"py", "px"}               # the dilation parity
    if G == 32:
        assert _fields_that_change(G, 640, 5, H, W, 2, 1, 2) & {"py", "px"}


@pytest.mark.parametrize("name,ncg,kd,dil,H,W", LAUNCHES)
def test_a_dropped_book_hand_over_changes_the_words_a_second_tile_reads(name, ncg, kd, dil, H, W):
    """The producers' last two stages of a tile load the NEXT tile's first two stages from the next tile's book.  Keeping the current
    tile's offsets there makes the second tile of a walk convolve (for its first two 16-channel stages) the wrong pixels: in the
    mirror, the words of consecutive tiles of a walk differ for every hand-over of these launches — none of them would go unnoticed
    by a comparison of the output with a reference, and none exists in a launch of one tile per workgroup."""
    N = ww.grid_for(256, ncg, kd, dil, H, W)
    ntiles = ww.launch_tiles(N, H, W, ncg, dil)
    handovers = 0
    for w in ww.walks(ntiles, 256):
        for a, b in zip(w, w[1:]):
            ta, tb = ww.decode(a, N, H, W, ncg, kd, dil), ww.decode(b, N, H, W, ncg, kd, dil)
            assert ww.halo_words(ta, N, H, W, kd, dil) != ww.halo_words(tb, N, H, W, kd, dil), (name, a, b)
            handovers += 1
    assert handovers == ntiles - 256
    for w in ww.walks(ww.launch_tiles(1, H, W, ncg, dil), 256) if kd != 3 else []:
        assert len(w) == 1
