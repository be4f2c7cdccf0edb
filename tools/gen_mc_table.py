"""The 256-case triangle table of the TSDF mesh extraction (csrc/tsdf_mesh.hip), derived from a rule and written as
neuralrgbd_amd/csrc/tsdf_mc_table.hpp.  Nothing is read from anywhere: the table is what the rule below gives.

    python tools/gen_mc_table.py            # rewrites the header
    python tools/gen_mc_table.py --check    # exit status 1 when the committed header differs

Numbering.  Corner c = cx + 2 cy + 4 cz of a cell whose lowest lattice point is (ix, iy, iz); bit c of the case is set iff T_c < 0
("inside").  Edge e = 4 a + p + 2 q runs along axis a (0, 1, 2 = x, y, z) from the corner whose coordinates on the two OTHER axes, in
ascending axis order, are (p, q) and whose coordinate on a is 0: edges 0-3 along x from (0, p, q), 4-7 along y from (p, 0, q), 8-11
along z from (p, q, 0).  The vertex of edge e is the crossing (lattice point of the low corner, axis a) of nrgbd_tsdf_extract_points.

The rule.
  * Face segments: the four corners of each of the six faces are walked counter-clockwise as seen from outside the cube; every
    maximal run of inside corners is cut off by one segment, directed from the sign-changing edge at which the walk enters the run to
    the one at which it leaves it.  A face with four sign changes gets two segments, each around one INSIDE corner.  Only the face's
    four signs enter, so the two cells that share a face agree.
  * Loops: a sign-changing edge lies on two faces, which walk it in opposite directions, so it starts exactly one segment and ends
    exactly one: the segments link into closed, consistently directed loops.  Loops are taken in the order of their lowest edge.
  * Triangulation: a loop of n edges becomes the fan (L0, Li, Li+1), i = 1 .. n - 2, of the first rotation L of the loop, counted
    from its lowest edge, none of whose diagonals (L0, Li), i = 2 .. n - 2, joins two edges of one cube face: a diagonal inside a face
    is a mesh edge the neighbouring cell can produce too.
  * Winding: with the segment direction above every triangle's right-hand normal points to positive T, free space.

This is a topologically consistent table (a closed manifold on any sign field), not MC33: inside an ambiguous cell it does not follow
the topology of the trilinear interpolant."""
import os
import sys

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neuralrgbd_amd", "csrc", "tsdf_mc_table.hpp")
SLOTS = 16                      # edge slots per case: at most 5 triangles and a terminating -1


def corner(cx, cy, cz):
    return cx + 2 * cy + 4 * cz


def edge_low_corner(e):
    """(cx, cy, cz) of the low corner of edge e."""
    a, p, q = e >> 2, e & 1, (e >> 1) & 1
    lo = [0, 0, 0]
    others = [k for k in range(3) if k != a]
    lo[others[0]], lo[others[1]] = p, q
    return tuple(lo)


def edge_corners(e):
    c0 = corner(*edge_low_corner(e))
    return c0, c0 | (1 << (e >> 2))


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def face_walks():
    """The six faces as four corners each, counter-clockwise seen from outside: axis d, side s; (u, v, d) is right-handed."""
    walks = []
    for d in range(3):
        u, v = (d + 1) % 3, (d + 2) % 3
        for s in (0, 1):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)]
            if s == 0:
                ring.reverse()
            walk = []
            for cu, cv in ring:
                c = [0, 0, 0]
                c[d], c[u], c[v] = s, cu, cv
                walk.append(corner(*c))
            walks.append(walk)
    return walks


FACES = face_walks()
EDGE_FACES = [frozenset(f for f, w in enumerate(FACES) if set(edge_corners(e)) <= set(w)) for e in range(12)]


def on_common_face(a, b):
    return bool(EDGE_FACES[a] & EDGE_FACES[b])


def segments(case):
    """{entering edge: leaving edge} over the six faces."""
    nxt = {}
    for walk in FACES:
        ins = [(case >> c) & 1 for c in walk]
        for i in range(4):
            if ins[i] and not ins[i - 1]:
                j = i
                while ins[(j + 1) % 4]:
                    j += 1
                start = EDGE_OF[frozenset((walk[i - 1], walk[i]))]
                end = EDGE_OF[frozenset((walk[j % 4], walk[(j + 1) % 4]))]
                assert start not in nxt
                nxt[start] = end
    return nxt


def loops(case):
    nxt = segments(case)
    changing = [e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1]
    assert sorted(nxt) == changing == sorted(nxt.values())
    out, seen = [], set()
    for e in changing:
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        out.append(loop)
    return out


def fan(loop):
    n = len(loop)
    for r in range(n):
        L = loop[r:] + loop[:r]
        if not any(on_common_face(L[0], L[i]) for i in range(2, n - 1)):
            return [(L[0], L[i], L[i + 1]) for i in range(1, n - 1)]
    raise AssertionError("no valid apex for loop %s" % (loop,))


def triangles(case):
    return [t for loop in loops(case) for t in fan(loop)]


def table():
    """[256] lists of (e0, e1, e2)."""
    tab = [triangles(case) for case in range(256)]
    assert tab[1] == [(0, 4, 8)]            # the corner at the origin inside: the normal of (x, y, z) points to (1, 1, 1), outside
    return tab


def render():
    tab = table()
    assert max(len(t) for t in tab) * 3 < SLOTS
    lines = [
        "// tsdf_mc_table.hpp: the triangle table of the TSDF mesh extraction (tsdf_mesh.hip).  GENERATED by tools/gen_mc_table.py from",
        "// the rule written out there; do not edit: tests/test_tsdf_mesh_host.py regenerates it and compares.",
        "//",
        "// Corner c = cx + 2 cy + 4 cz of the cell whose lowest lattice point is (ix, iy, iz); bit c of the case is set iff T_c < 0.",
        "// Edge e = 4 a + p + 2 q runs along axis a from the corner with coordinate 0 on a and (p, q) on the two other axes in ascending",
        "// axis order: 0-3 along x from (0, p, q), 4-7 along y from (p, 0, q), 8-11 along z from (p, q, 0).  Its vertex is the crossing",
        "// (lattice point of that corner, axis a) of nrgbd_tsdf_extract_points.",
        "// kMcTriangles[case]: three edges per triangle, the right-hand normal towards positive T (free space), then -1 to the end;",
        "// kMcCount[case]: the number of triangles (at most kMcMaxTriangles; %d over the 256 cases)." % sum(len(t) for t in tab),
        "// The table is topologically consistent: face segments depend on the face's four signs alone (a face with four sign changes",
        "// separates its two INSIDE corners), and no fan diagonal lies in a cube face, so the mesh of any sign field is a closed",
        "// manifold.  It is not MC33: inside an ambiguous cell it does not follow the topology of the trilinear interpolant.",
        "#pragma once",
        "",
        "namespace nrgbd {",
        "",
        "constexpr int kMcMaxTriangles = %d;" % max(len(t) for t in tab),
        "",
        "alignas(16) static __constant__ const signed char kMcTriangles[256][%d] = {" % SLOTS,
    ]
    for case, tris in enumerate(tab):
        flat = [e for t in tris for e in t]
        flat += [-1] * (SLOTS - len(flat))
        lines.append("    {%s},  // %d" % (", ".join("%2d" % e for e in flat), case))
    lines += ["};", "", "alignas(16) static __constant__ const unsigned char kMcCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    %s," % ", ".join("%d" % len(t) for t in tab[r:r + 32]))
    lines += ["};", "", "}  // namespace nrgbd", ""]
    return "\n".join(lines)


def main(argv):
    text = render()
    if "--check" in argv:
        same = os.path.isfile(HEADER) and open(HEADER).read() == text
        print("tsdf_mc_table.hpp %s" % ("is up to date" if same else "DIFFERS from the generator's output"))
        return 0 if same else 1
    with open(HEADER, "w") as fh:
        fh.write(text)
    tab = table()
    print("%s: %d triangles over 256 cases, at most %d per case" % (HEADER, sum(len(t) for t in tab), max(len(t) for t in tab)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
