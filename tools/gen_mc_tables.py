"""Generates fast-learning-nerf_amd/csrc/mc_tables.h: the 256-case marching-cubes edge and triangle tables.

Corner and edge numbering are the classic ones (corner n at (x, y, z) = (i, j, k) offsets CORNERS[n]; edge e joins
EDGES[e]).  The triangles are not copied from the classic table: they are derived here from one face rule, so that the
surface is closed for every field, ambiguous faces included.

- Face rule: on a face with two diagonal inside corners and two diagonal outside corners, the two segments cut off
  the inside corners ("separate the inside corners").  Both cells that share the face see the same four values, so
  they pair the same four edge vertices.
- Each segment is directed by which side of it the inside corner lies on, seen from outside the cell.  The neighbour
  sees the face from the other side and runs the segment the other way, so the surface is consistently oriented.
- Segments chain into closed loops on the cube's boundary.  Each loop is triangulated with diagonals whose two
  endpoints do not share a cube face.  Such a diagonal belongs to this cell alone, so every mesh edge lies in
  exactly two triangles.
- The winding makes (v1-v0) x (v2-v0) point from inside (value > threshold) to outside.

Run: python tools/gen_mc_tables.py  (rewrites the header; the output is deterministic)."""
import os
import sys

import numpy as np

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]   # lower corner first
# faces: four corners in cyclic order, outward normal
FACES = [((0, 1, 2, 3), (0, 0, -1)), ((4, 5, 6, 7), (0, 0, 1)), ((0, 1, 5, 4), (0, -1, 0)),
         ((3, 2, 6, 7), (0, 1, 0)), ((0, 3, 7, 4), (-1, 0, 0)), ((1, 2, 6, 5), (1, 0, 0))]
MAX_TRI = 5


def edge_of(a, b):
    for e, (p, q) in enumerate(EDGES):
        if {p, q} == {a, b}:
            return e
    raise KeyError((a, b))


def edge_faces(e):
    a, b = EDGES[e]
    return {f for f, (cs, _) in enumerate(FACES) if a in cs and b in cs}


def mid(e):
    a, b = EDGES[e]
    return (np.array(CORNERS[a], float) + np.array(CORNERS[b], float)) / 2


def segments(case):
    inside = [(case >> n) & 1 for n in range(8)]
    segs = []
    for cs, normal in FACES:
        fe = [edge_of(cs[m], cs[(m + 1) % 4]) for m in range(4)]
        cross = [m for m in range(4) if inside[cs[m]] != inside[cs[(m + 1) % 4]]]
        pairs = []
        if len(cross) == 2:
            pairs = [(fe[cross[0]], fe[cross[1]])]
        elif len(cross) == 4:
            pairs = [(fe[(m - 1) % 4], fe[m]) for m in range(4) if inside[cs[m]]]   # cut off each inside corner
        for a, b in pairs:
            ia = [c for c in EDGES[a] if inside[c]][0]
            s = np.dot(np.cross(mid(b) - mid(a), np.array(CORNERS[ia], float) - mid(a)), normal)
            assert s != 0
            segs.append((a, b) if s > 0 else (b, a))
    return segs


def loops(case):
    nxt = {}
    for a, b in segments(case):
        assert a not in nxt, (case, 'two segments leave one vertex')
        nxt[a] = b
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        lp, v = [], start
        while v not in seen:
            seen.add(v)
            lp.append(v)
            v = nxt[v]
        assert v == start
        out.append(lp)
    return out


def triangulate(orig):
    """Triangles (in loop orientation) of polygon `orig` whose diagonals join edges without a common face."""
    m = len(orig)

    def attempt(lp):
        def ok(i, j):   # chord between lp[i] and lp[j]: a loop side, or an allowed diagonal
            return (j - i) % m in (1, m - 1) or not (edge_faces(lp[i]) & edge_faces(lp[j]))

        memo = {}

        def rec(i, j):   # triangulate the chain i..j closed by chord (i, j)
            if j - i < 2:
                return []
            if (i, j) not in memo:
                res = None
                for k in range(i + 1, j):
                    if ok(i, k) and ok(k, j):
                        a, b = rec(i, k), rec(k, j)
                        if a is not None and b is not None:
                            res = a + [(lp[i], lp[k], lp[j])] + b
                            break
                memo[(i, j)] = res
            return memo[(i, j)]
        return rec(0, m - 1)
    for r in range(m):   # first rotation that admits such a triangulation
        t = attempt(orig[r:] + orig[:r])
        if t is not None:
            return t
    raise RuntimeError('no face-safe triangulation of loop %r' % (orig,))


def tables():
    tri = np.full((256, 3 * MAX_TRI + 1), -1, np.int8)
    edge = np.zeros(256, np.uint16)
    for case in range(256):
        inside = [(case >> n) & 1 for n in range(8)]
        for e, (a, b) in enumerate(EDGES):
            if inside[a] != inside[b]:
                edge[case] |= 1 << e
        ts = [t for lp in loops(case) for t in triangulate(lp)]
        assert len(ts) <= MAX_TRI, (case, len(ts))
        flat = [e for t in ts for e in t]
        tri[case, :len(flat)] = flat
    return tri, edge


def orientation_signs(tri):
    """Signs of (sum of a case's triangle normals) . (outside centroid - inside centroid) over the cases where it is not 0."""
    signs = set()
    for case in range(1, 255):
        inside = [(case >> n) & 1 for n in range(8)]
        c_in = np.mean([CORNERS[n] for n in range(8) if inside[n]], 0)
        c_out = np.mean([CORNERS[n] for n in range(8) if not inside[n]], 0)
        n_sum = np.zeros(3)
        row = tri[case]
        for t in range(MAX_TRI):
            if row[3 * t] < 0:
                break
            p = [mid(int(row[3 * t + q])) for q in range(3)]
            n_sum += np.cross(p[1] - p[0], p[2] - p[0])
        s = np.dot(n_sum, c_out - c_in)
        if abs(s) > 1e-9:
            signs.add(int(np.sign(s)))
    return signs


def header(tri, edge):
    axis = [int(np.argmax(np.array(CORNERS[b]) - np.array(CORNERS[a]))) for a, b in EDGES]
    ntri = [int((tri[c] >= 0).sum()) // 3 for c in range(256)]
    lines = ['// mc_tables.h -- marching-cubes tables, GENERATED by tools/gen_mc_tables.py (do not edit by hand).',
             '// Classic corner / edge numbering; triangles derived from one face rule (ambiguous faces separate the inside',
             '// corners), so meshes are closed and consistently oriented for every field.  Winding: (v1-v0)x(v2-v0) points',
             '// from inside (value > threshold) to outside.  Bit n of a case = corner n is inside.',
             '// The initialisers are macros so that one copy of the numbers serves the host arrays and __constant__ memory.',
             '#pragma once',
             '#define MC_MAX_TRI %d' % MAX_TRI,
             '#define MC_TRI_STRIDE %d   // int8 entries per case: up to MC_MAX_TRI triangles, -1 terminated' % (3 * MAX_TRI + 1),
             '// corner n sits at (i, j, k) offset MC_CORNER[n]; edge e runs from corner MC_EDGE_LO[e] along axis MC_EDGE_AXIS[e]',
             '// (0 = i, 1 = j, 2 = k)',
             '#define MC_CORNER_INIT {%s}' % ', '.join('{%d, %d, %d}' % c for c in CORNERS),
             '#define MC_EDGE_LO_INIT {%s}' % ', '.join(str(a) for a, _ in EDGES),
             '#define MC_EDGE_AXIS_INIT {%s}' % ', '.join(str(a) for a in axis),
             '#define MC_EDGE_TABLE_INIT { \\']
    for r in range(0, 256, 16):
        lines.append('  ' + ', '.join('0x%03x' % int(v) for v in edge[r:r + 16]) + ', \\')
    lines.append('}')
    lines.append('#define MC_NTRI_INIT { \\')
    for r in range(0, 256, 32):
        lines.append('  ' + ', '.join(str(v) for v in ntri[r:r + 32]) + ', \\')
    lines.append('}')
    lines.append('#define MC_TRI_TABLE_INIT { \\')
    for case in range(256):
        lines.append('  {' + ', '.join('%d' % int(v) for v in tri[case]) + '}, \\')
    lines.append('}')
    return '\n'.join(lines) + '\n'


def main():
    tri, edge = tables()
    if orientation_signs(tri) == {-1}:   # the segment direction convention came out reversed: flip every triangle
        for case in range(256):
            for t in range(MAX_TRI):
                if tri[case, 3 * t] >= 0:
                    tri[case, 3 * t + 1], tri[case, 3 * t + 2] = tri[case, 3 * t + 2], tri[case, 3 * t + 1]
    signs = orientation_signs(tri)
    assert signs == {1}, signs
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fast-learning-nerf_amd', 'csrc', 'mc_tables.h')
    with open(out, 'w') as f:
        f.write(header(tri, edge))
    n = [int((tri[c] >= 0).sum()) // 3 for c in range(256)]
    print(out, 'max triangles per case', max(n), file=sys.stderr)


if __name__ == '__main__':
    main()
