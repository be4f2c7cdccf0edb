"""Host mirror of the persistent Winograd kernel's tile list (csrc/wino_pc.hpp: pc_tile_share, pc_decode; the epilogue choice of
csrc/wino_pc.hip: pc_epilogue / pc_dc_tile).  Plain Python, no GPU: the walking tests (test_gpu_wino_pc_walk.py) take their grids
from it and assert from it that a launch really makes workgroups hand one tile over to the next.

KEEP IN STEP with pc_tile_share and pc_decode in neuralrgbd_amd/csrc/wino_pc.hpp (a comment there names this file): a change of
the tile order or of the split on one side without the other makes the preconditions of the walking tests describe another kernel."""
from collections import namedtuple

TH, TW = 8, 16            # kPcTH, kPcTW: output pixels of a tile, in units of the dilation lattice

Tile = namedtuple("Tile", "n y0 x0 py px cg row inside")


def ceil_div(a, b):
    return (a + b - 1) // b


def plane_tiles(H, W, dil=1):
    """(tiles_y, tiles_x) of one plane."""
    return ceil_div(H, TH * dil), ceil_div(W, TW * dil)


def spatial_tiles(N, H, W, dil=1):
    """nrgbd_conv_wino_tiles: statistics rows of the full form."""
    ty, tx = plane_tiles(H, W, dil)
    return N * ty * tx * dil * dil


def share(ntiles, G, b):
    """pc_tile_share: (first, step, end) of workgroup b of G.  XCD x = b % 8 owns the x-th contiguous eighth of the list and its
    workgroups walk it interleaved; a grid that is no multiple of 8 walks the whole list with stride G."""
    if G % 8 == 0:
        xc = b & 7
        return ((ntiles * xc) >> 3) + (b >> 3), G >> 3, (ntiles * (xc + 1)) >> 3
    return b, G, ntiles


def decode(t, N, H, W, ncg, kd=1, dil=1):
    """pc_decode<KD, DIL>: list index -> tile.  ncg = column groups of the launch ((Cout + 63) >> 6; 4 = the deconv form's phases, cg
    = phase 2a + b).  n is the depth slice when kd = 3 (depth fastest).  inside: the tile takes the interior epilogue (else the edge
    body) — the test of pc_epilogue and, with dil = 1, of pc_dc_tile."""
    tiles_y, tiles_x = plane_tiles(H, W, dil)
    row = t // ncg
    cg = t - row * ncg
    t, n, par = row, 0, 0
    if kd == 3:
        n, t = t % N, t // N
    if dil > 1:
        par, t = t % (dil * dil), t // (dil * dil)
    tx, t = t % tiles_x, t // tiles_x
    ty = t
    if kd != 3:
        ty, n = t % tiles_y, t // tiles_y
    py = par // dil
    px = par - py * dil
    y0, x0 = ty * TH * dil, tx * TW * dil
    inside = y0 + py + dil * (TH - 1) < H and x0 + px + dil * (TW - 1) < W
    return Tile(n, y0, x0, py, px, cg, row, inside)


def walks(ntiles, ncu):
    """The tile sequence of every workgroup of a launch: G = min(ntiles, ncu) workgroups (pc_workgroups)."""
    G = min(ntiles, ncu)
    out = []
    for b in range(G):
        first, step, end = share(ntiles, G, b)
        out.append(list(range(first, end, step)))
    return out


def launch_tiles(N, H, W, ncg, dil=1):
    return spatial_tiles(N, H, W, dil) * ncg


def preconditions(ncu, N, H, W, ncg, kd=1, dil=1):
    """What a walking test needs of its launch, each as a bool (conditions, not measurements):
      walk2     every workgroup walks at least 2 tiles
      walk3     at least one walks 3
      in_edge   some walk goes from an interior-epilogue tile to an edge-epilogue tile
      edge_in   ... and some the other way
      crosses   some walk goes on to another sample (depth slice when kd = 3)
      sample    2-D only: one sample's tile list is no longer than the CU count, so a launch per sample does not walk"""
    nt = launch_tiles(N, H, W, ncg, dil)
    ws = walks(nt, ncu)
    steps = [(decode(a, N, H, W, ncg, kd, dil), decode(b, N, H, W, ncg, kd, dil)) for w in ws for a, b in zip(w, w[1:])]
    return {
        "walk2": min(len(w) for w in ws) >= 2,
        "walk3": max(len(w) for w in ws) >= 3,
        "in_edge": any(a.inside and not b.inside for a, b in steps),
        "edge_in": any(b.inside and not a.inside for a, b in steps),
        "crosses": any(a.n != b.n for a, b in steps),
        "sample": kd == 3 or launch_tiles(1, H, W, ncg, dil) <= ncu,
    }


def grid_for(ncu, ncg, kd, dil, H, W, limit=4096):
    """The smallest N (depth D when kd = 3) at which a launch on ncu CUs meets every one of preconditions()."""
    for N in range(1, limit + 1):
        if all(preconditions(ncu, N, H, W, ncg, kd, dil).values()):
            return N
    raise ValueError("no N <= %d makes a %dx%d plane (ncg %d, kd %d, dil %d) walk on %d CUs" % (limit, H, W, ncg, kd, dil, ncu))


def halo_words(tile, N, H, W, kd=1, dil=1):
    """The input pixels (slice, y, x) inside the image that pc_book makes the producers load for a tile (10 x 18 halo; kd = 3: of the
    three slices n - 1 .. n + 1 that exist).  What a wrong book hand-over changes."""
    out = set()
    for z in ([tile.n] if kd != 3 else [z for z in (tile.n - 1, tile.n, tile.n + 1) if 0 <= z < N]):
        for hy in range(TH + 2):
            for hx in range(TW + 2):
                gy, gx = tile.y0 + tile.py + dil * (hy - 1), tile.x0 + tile.px + dil * (hx - 1)
                if 0 <= gy < H and 0 <= gx < W:
                    out.add((z, gy, gx))
    return out
