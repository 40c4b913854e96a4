"""CPU-only: the marching-cubes case table of xs_extract_mesh (xs_mesh_case_table, host code) for all 256 cases — only and all
sign-changing edges, consistent orientation, normals away from the negative side, and a face rule that depends on the face's signs alone
(so that neighbouring cubes meet without cracks)."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def capi():
    # imported when a test runs, not when the module is collected: a GPU run of the suite loads torch's HIP runtime first
    return importlib.import_module("x-slam_amd.capi")


def corner(c):   # the numbering documented with xs_mesh_case_table in include/xslam_amd.h
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_ends(e):
    a, j = divmod(e, 4)
    others = [k for k in range(3) if k != a]
    lo = np.zeros(3, int)
    lo[others[0]], lo[others[1]] = j & 1, (j >> 1) & 1
    hi = lo.copy()
    hi[a] = 1
    return lo, hi


def idx(p):
    return int(p[0] | (p[1] << 1) | (p[2] << 2))


def sign_change(case, e):
    lo, hi = edge_ends(e)
    return bool(case >> idx(lo) & 1) != bool(case >> idx(hi) & 1)


def mid(e):
    lo, hi = edge_ends(e)
    return (lo + hi) / 2.0


def directed_edges(tris):
    return [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]


@functools.lru_cache(maxsize=None)
def table():
    return {c: capi().mesh_case_table(c) for c in range(256)}


def test_every_case_uses_only_and_all_crossing_edges():
    for case, tris in table().items():
        used = {e for t in tris for e in t}
        crossing = {e for e in range(12) if sign_change(case, e)}
        assert used == crossing, case
        assert len(tris) <= 5
        assert (case in (0, 255)) == (not tris)


def test_orientation_is_consistent_inside_each_case():
    for case, tris in table().items():
        d = directed_edges(tris)
        assert len(set(d)) == len(d), case                 # no directed edge twice
        for u, v in d:
            if (v, u) not in d:                             # used once: a boundary segment, on a face of the cube
                shared = [k for k in range(3) if mid(u)[k] == mid(v)[k] and mid(u)[k] in (0.0, 1.0)]
                assert shared, (case, u, v)


def test_single_negative_corner_normals_point_away():
    for c in range(8):
        for case in (1 << c, 255 ^ (1 << c)):
            (t,) = table()[case]
            p = [mid(e) for e in t]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            centre = sum(p) / 3
            toward_neg = (corner(c) - centre) if case == 1 << c else (centre - corner(c))   # negative side
            assert np.dot(n, toward_neg) < 0, case


def boundary_segments_on_face(case, axis, side):
    """Unordered boundary segments of the case that lie on face (axis, side), as sets of edge midpoints in the face's own 2-D coords."""
    d = directed_edges(table()[case])
    out = set()
    for u, v in d:
        if (v, u) in d:
            continue
        if mid(u)[axis] == side and mid(v)[axis] == side:
            others = [k for k in range(3) if k != axis]
            out.add(frozenset((tuple(mid(u)[others]), tuple(mid(v)[others]))))
    return out


def test_face_pairing_depends_only_on_the_face():
    """For every face and every sign pattern of its corners: the lower cube (face at side 1) and the upper cube (face at side 0) cut the
    shared face into the same segments, whatever their other four corners are."""
    for axis in range(3):
        for pattern in range(16):
            seen = set()
            for other in range(16):
                for side in (0, 1):
                    case = 0
                    face_i = other_i = 0
                    for c in range(8):
                        if corner(c)[axis] == side:
                            bit = pattern >> face_i & 1
                            face_i += 1
                        else:
                            bit = other >> other_i & 1
                            other_i += 1
                        case |= bit << c
                    seen.add(frozenset(boundary_segments_on_face(case, axis, side)))
            assert len(seen) == 1, (axis, pattern, seen)


def test_generated_table_is_committed():
    """csrc/xs_mesh_table.h is what csrc/gen_mesh_table.py writes."""
    csrc = os.path.join(ROOT, "x-slam_amd", "csrc")
    out = subprocess.run([sys.executable, os.path.join(csrc, "gen_mesh_table.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(csrc, "xs_mesh_table.h")).read()


def test_bad_case_is_refused():
    with pytest.raises(capi().XsError):
        capi().mesh_case_table(256)
