"""ppp_set_cloud_mesh / the STL codec: a triangle mesh sampled on the device into the resident cloud.

The yardstick is sample_mesh() below: the rule of include/ppp_hip.h restated in numpy float64 on the RESIDENT vertices, which
the tests read back from a handle (ppp_set_cloud + ppp_get_cloud), so that nothing here depends on how the conversion is
written.  Samples, tri_index and stats are compared for exact equality.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, FRONT = 0, 1


# ---------------------------------------------------------------- the rule, restated
def sample_mesh(rv, tris, pitch, facing=ALL, vp=(0.0, 0.0, 0.0), detail=False):
    """rv: resident vertices float32 [n_verts, 3]; tris int [n_tris, 3] or None (a soup).  pitch as the ABI holds it: a float32.
    Returns (samples float32 [n, 3], tri_index int32 [n], stats); detail=True adds per-sample (t, w) and per-row M."""
    rv = np.asarray(rv, np.float32)
    nv = rv.shape[0]
    if tris is None:
        tris = np.arange(nv, dtype=np.int64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    pitch = np.float64(np.float32(pitch))
    v = np.asarray(vp, np.float32).astype(np.float64)
    P = rv.astype(np.float64)
    out, idx, ts, ws, Ms = [], [], [], [], []
    st = dict(triangles=len(tris), sampled=0, degenerate=0, culled=0, rows=0, samples=0)
    with np.errstate(all="ignore"):
        for f, tri in enumerate(tris):
            if ((tri < 0) | (tri >= nv)).any():
                st["degenerate"] += 1
                continue
            a, b, c = P[tri[0]], P[tri[1]], P[tri[2]]
            if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
                st["degenerate"] += 1
                continue

            def len2(p, q):
                d = q - p
                return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            ab, bc, ca = len2(a, b), len2(b, c), len2(c, a)
            if ab >= bc and ab >= ca:
                p0, p1, p2, longest = a, b, c, ab
            elif bc >= ca:
                p0, p1, p2, longest = b, c, a, bc
            else:
                p0, p1, p2, longest = c, a, b, ca
            e1, e2 = p1 - p0, p2 - p0
            n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            A2 = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if not (A2 > 0.0) or not np.isfinite(A2):
                st["degenerate"] += 1
                continue
            if facing == FRONT:
                d = v - p0
                if not (((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) > 0.0):
                    st["culled"] += 1
                    continue
            L = np.sqrt(longest)
            hgt = A2 / L
            R = int(max(1.0, np.ceil(hgt / pitch)))
            r = np.arange(R, dtype=np.float64)
            t = (r + 0.5) / np.float64(R)
            ln = L * (1.0 - t)
            M = np.maximum(1.0, np.ceil(ln / pitch)).astype(np.int64)
            row = np.repeat(np.arange(R), M)
            first = np.concatenate([[0], np.cumsum(M)[:-1]])
            k = (np.arange(M.sum()) - first[row]).astype(np.float64)
            tt = t[row]
            s = (k + 0.5) / M[row].astype(np.float64)
            w = s * (1.0 - tt)
            pts = (p0[None, :] + e2[None, :] * tt[:, None]) + e1[None, :] * w[:, None]
            out.append(pts.astype(np.float32))
            idx.append(np.full(len(pts), f, np.int32))
            ts.append(tt); ws.append(w); Ms.append(M)
            st["sampled"] += 1
            st["rows"] += R
            st["samples"] += len(pts)
    samples = np.concatenate(out) if out else np.zeros((0, 3), np.float32)
    tri_index = np.concatenate(idx) if idx else np.zeros(0, np.int32)
    if detail:
        return samples, tri_index, st, (np.concatenate(ts), np.concatenate(ws), np.concatenate(Ms))
    return samples, tri_index, st


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def resident(E, verts, change_range):
    """what ppp_set_cloud makes of these vertices"""
    e = E.Engine(0, change_range=change_range)
    e.set_cloud(np.ascontiguousarray(verts, np.float32).reshape(-1, 3))
    rv = e.cloud()
    e.close()
    return rv


def check_against_numpy(E, verts, tris, pitch, change_range=0, facing=ALL, viewpoint=None, engine=None):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    rv = resident(E, verts, change_range)
    want, want_idx, want_st = sample_mesh(rv, tris, pitch, facing, (0, 0, 0) if viewpoint is None else viewpoint)
    e = engine or E.Engine(0, change_range=change_range)
    got_st = e.set_cloud_mesh(verts, tris, pitch=pitch, facing=facing, viewpoint=viewpoint, tri_index=True)
    got_idx = got_st.pop("tri_index")
    got = e.cloud()
    print("mesh: %d triangles, stats %s" % (want_st["triangles"], got_st))
    assert got_st == want_st
    assert same_bits(got_idx, want_idx)
    assert same_bits(got, want)
    if engine is None:
        e.close()
    return got, got_idx, got_st


def rand_triangles(rng, count, size, spread):
    c = rng.uniform(-spread, spread, (count, 1, 3))
    return (c + rng.uniform(-size, size, (count, 3, 3))).astype(np.float32)


# ---------------------------------------------------------------- CPU: the restatement's own properties
def test_rule_samples_lie_strictly_inside_and_counts_add_up():
    rng = np.random.default_rng(11)
    for tri in rand_triangles(rng, 40, 6.0, 50.0):
        pitch = float(rng.uniform(0.3, 1.5))
        pts, idx, st, (t, w, M) = sample_mesh(tri, None, pitch, detail=True)
        assert st["samples"] == len(pts) == int(M.sum()) and st["rows"] == len(M) and (idx == 0).all()
        # the barycentric weights of the rule itself: (1 - t - w, w, t) on (p0, p1, p2)
        assert (t > 0).all() and (t < 1).all() and (w > 0).all() and (t + w < 1).all()
        # ... and of the rounded points, solved against the triangle
        a, b, c = tri.astype(np.float64)
        B = np.linalg.lstsq(np.stack([b - a, c - a], axis=1), (pts.astype(np.float64) - a).T, rcond=None)[0]
        assert (B > 0).all() and (B.sum(axis=0) < 1).all()
        off = pts.astype(np.float64) - a - (B.T @ np.stack([b - a, c - a]))
        assert np.abs(off).max() < 1e-4                  # in the triangle's plane (float32 of coordinates below 64: 4e-6)


def probe_gap(tri, pitch, grid=48):
    """the largest distance from a point of a fine barycentric grid over the triangle to its nearest sample, and the base angles"""
    pts = sample_mesh(tri, None, pitch)[0].astype(np.float64)
    a, b, c = np.asarray(tri, np.float64)
    u, v = np.meshgrid(np.arange(grid + 1), np.arange(grid + 1), indexing="ij")
    keep = u + v <= grid
    u, v = u[keep] / grid, v[keep] / grid
    probes = a + u[:, None] * (b - a) + v[:, None] * (c - a)
    d = np.sqrt(((probes[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    return d.max()


def base_angles(tri):
    """the angles at the two ends of the longest edge (radians): the two smallest of the triangle"""
    p = np.asarray(tri, np.float64)
    ang = []
    for i in range(3):
        x, y = p[(i + 1) % 3] - p[i], p[(i + 2) % 3] - p[i]
        ang.append(np.arccos(np.clip(x @ y / np.linalg.norm(x) / np.linalg.norm(y), -1, 1)))
    return sorted(ang)[:2]


def test_rule_leaves_no_point_farther_than_the_pitch_from_a_sample():
    """No point of a triangle is farther than `pitch` from a sample, on a fine barycentric probe grid.

    Rows are at most pitch apart and a row's samples at most pitch apart, so a point between two rows is within
    sqrt(1/4 + 1/4) pitch of a sample -- except beside the two slanted edges, where the row above or below is shorter: there the
    gap grows by (row spacing / 2) cot(angle at that end of the longest edge).  The bound `pitch` therefore holds for triangles
    whose two base angles are at least atan(1 / (sqrt(3) - 1)) = 53.8 degrees and whose height is at least one pitch: those are the
    triangles drawn here (jittered equilateral ones).  On triangles drawn without that condition (vertices uniform in a cube of
    16 around a centre, pitch 0.5) the gap exceeded the pitch in 58 of 60, 3.9 pitches at worst, and the 50 x 0.05 sliver, one row
    of 50 samples over its middle half by the same rule, leaves its ends 25.5 pitches from a sample: the rule samples the area
    evenly, it does not cover corners.  What it does guarantee beside a sharper corner is the next test's bound."""
    rng = np.random.default_rng(5)
    done = 0
    while done < 25:
        side = rng.uniform(3.0, 12.0)
        tri = np.array([[0, 0, 0], [side, 0, 0], [side / 2, side * np.sqrt(3) / 2, 0]]) + rng.uniform(-0.04, 0.04, (3, 3)) * side
        rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        tri = (tri @ rot.T + rng.uniform(-30, 30, 3)).astype(np.float32)
        if min(base_angles(tri)) < np.deg2rad(54.5):
            continue
        pitch = float(rng.uniform(0.4, 1.0))
        assert probe_gap(tri, pitch) <= pitch
        done += 1


def test_rule_gap_beside_a_sharp_corner_is_bounded_by_its_angle():
    """any triangle at least one pitch high: the gap is at most sqrt(1/4 + (1 + cot a)^2 / 4) pitch, a = its smallest angle"""
    rng = np.random.default_rng(6)
    worst = 0.0
    for tri in rand_triangles(rng, 40, 8.0, 30.0):
        pitch = 0.5
        a, b, c = tri.astype(np.float64)
        area2 = np.linalg.norm(np.cross(b - a, c - a))
        longest = max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
        if area2 / longest < 2 * pitch:
            continue
        alpha = min(base_angles(tri))
        bound = np.sqrt(0.25 + 0.25 * (1 + 1 / np.tan(alpha)) ** 2) * pitch
        gap = probe_gap(tri, pitch)
        worst = max(worst, gap / pitch)
        assert gap <= bound * (1 + 1e-9)
    print("largest gap over the pitch: %.3f" % worst)


# ---------------------------------------------------------------- CPU: the STL codec
def soup(seed=3, n=37):
    v = np.random.default_rng(seed).normal(size=(n, 3, 3)).astype(np.float32) * np.float32(25)
    if n > 5:
        v[5, 1] = v[5, 0]                                # a degenerate facet: its normal is written as zeros
    return v


def test_stl_binary_roundtrip_and_normals(engine_mod, tmp_path):
    v = soup()
    p = str(tmp_path / "a.stl")
    engine_mod.save_stl(p, v)
    raw = open(p, "rb").read()
    assert len(raw) == 84 + 50 * len(v) and struct.unpack("<I", raw[80:84])[0] == len(v) and not raw.startswith(b"solid")
    rec = np.frombuffer(raw[84:], np.uint8).reshape(-1, 50)
    normals = np.ascontiguousarray(rec[:, :12]).view(np.float32).reshape(-1, 3)
    a, b, c = (v[:, i].astype(np.float64) for i in range(3))
    n = np.cross(b - a, c - a)
    # (np.cross pairs the products as the codec does; the sum's order is spelled out)
    A2 = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    want = np.zeros_like(n)
    ok = A2 > 0
    want[ok] = n[ok] / A2[ok, None]
    assert same_bits(normals, want.astype(np.float32)) and not normals[5].any()
    back = engine_mod.load_stl(p)
    assert same_bits(back, v)
    q = str(tmp_path / "b.stl")
    engine_mod.save_stl(q, back)
    assert open(q, "rb").read() == raw                   # binary -> binary


def test_stl_ascii_to_binary(engine_mod, tmp_path):
    v = soup(seed=4)
    v[0, 0] = [1e-30, -3.4e38, 0.1]                      # %.9g carries every float
    p, q, r = (str(tmp_path / n) for n in ("a.stl", "b.stl", "c.stl"))
    engine_mod.save_stl(p, v, binary=False)
    txt = open(p).read()
    assert txt.startswith("solid") and txt.rstrip().splitlines()[-1].startswith("endsolid") and txt.count("vertex") == 3 * len(v)
    back = engine_mod.load_stl(p)
    assert same_bits(back, v)
    engine_mod.save_stl(q, back)
    engine_mod.save_stl(r, v)
    assert open(q, "rb").read() == open(r, "rb").read()  # ASCII -> binary: the bytes of the direct binary file
    # case and white space, as loosely as the ASCII PCD reader: upper case, tabs, CRLF, no indentation, several tokens per line
    loose = txt.upper().replace("E+", "e+").replace("E-", "e-").replace("\n", "\r\n").replace("   VERTEX", "\tVertex\t ").replace("  OUTER LOOP\r\n", "outer loop ")
    open(p, "w", newline="").write(loose)
    assert same_bits(engine_mod.load_stl(p), v)


def test_stl_binary_whose_header_starts_with_solid(engine_mod, tmp_path):
    v = soup(seed=5, n=3)
    p = str(tmp_path / "s.stl")
    engine_mod.save_stl(p, v)
    raw = bytearray(open(p, "rb").read())
    raw[:80] = b"solid made by some exporter".ljust(80, b" ")
    raw[84:96] = struct.pack("<3f", 9, 9, 9)             # a stored normal that is wrong: ignored
    open(p, "wb").write(bytes(raw))
    assert same_bits(engine_mod.load_stl(p), v)


def test_stl_truncated_and_malformed_files_are_refused(engine_mod, tmp_path):
    v = soup(seed=6, n=9)
    p, a = str(tmp_path / "a.stl"), str(tmp_path / "t.stl")
    engine_mod.save_stl(p, v)
    raw = open(p, "rb").read()
    engine_mod.save_stl(a, v, binary=False)
    txt = open(a).read()
    cut_facet = txt[:txt.index("endfacet", len(txt) // 2) - 30]
    bad = {
        "binary cut": raw[:-7], "binary cut at a record": raw[:-50], "binary with bytes behind": raw + b"\0\0",
        "count only": raw[:84], "header cut": raw[:40], "empty": b"",
        "solid-header binary cut": b"solid x".ljust(80, b" ") + raw[80:-13],
        "ascii cut inside a facet": cut_facet.encode(), "ascii without endsolid": txt[:txt.rindex("endsolid")].encode(),
        "vertex with two numbers": txt.replace("\n  endloop", " \n  endloop", 1).replace(txt.split("vertex")[1].split()[2], "", 1).encode(),
        "vertex with a word": txt.replace(txt.split("vertex")[2].split()[0], "abc", 1).encode(),
        "four vertices": txt.replace("  endloop", "   vertex 0 0 0\n  endloop", 1).encode(),
        "two vertices": txt.replace("   vertex", "   vertx", 1).encode(),
        "not stl": b"ply\nformat ascii 1.0\n" * 8,
    }
    for what, blob in bad.items():
        open(p, "wb").write(blob)
        with pytest.raises(engine_mod.PPPError) as ex:
            engine_mod.load_stl(p)
        assert ex.value.code == engine_mod.ERR_IO, what
    with pytest.raises(engine_mod.PPPError) as ex:
        engine_mod.load_stl(str(tmp_path / "missing.stl"))
    assert ex.value.code == engine_mod.ERR_IO
    open(p, "wb").write(b"solid nothing\nendsolid nothing\n")
    assert engine_mod.load_stl(p).shape == (0, 3, 3)      # an empty solid is a file; the sampler refuses it (no triangle)


def test_examples_still_build_and_name_the_mesh_calls(engine_mod):
    """the examples compile and link against the library, api_check names the new calls (that the reference's own drivers still
    compile unchanged against include/ is tests/test_host_logic.py::test_reference_drivers_compile_unchanged)"""
    src = open(os.path.join(ROOT, "examples", "api_check.cpp")).read()
    for name in ("ppp_set_cloud_mesh", "ppp_set_cloud_stl", "ppp_load_stl", "ppp_save_stl", "ppp_default_mesh_params"):
        assert name in src, name
    engine_mod.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "-j2", "connect", "api_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for exe in ("connect", "api_check"):
        assert os.path.exists(os.path.join(ROOT, "examples", exe)), exe


# ---------------------------------------------------------------- GPU
RIGHT = np.array([[[0, 0, 0], [7.3, 0, 0.4], [0, 4.1, 0.2]]], np.float32)
SLIVER = np.array([[[1, 2, 3], [51, 2, 3], [26, 2.05, 3]]], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("change_range", [0, 1])
def test_shapes(engine_mod, change_range):
    unit = np.float32(0.001 if change_range else 1.0)    # the file's units: metres when ChangeRange scales them to mm
    pitch = 0.5
    for tri in (RIGHT, RIGHT[:, [1, 2, 0]], RIGHT[:, [2, 0, 1]]):   # the same triangle in its three cyclic orders
        check_against_numpy(engine_mod, tri * unit, None, pitch, change_range)
    got, _, st = check_against_numpy(engine_mod, SLIVER * unit, None, pitch, change_range)
    assert st["rows"] == 1 and st["samples"] <= 51      # 50 x 0.05: one row of len / pitch points, not 10 000
    # smaller than the pitch: one sample, at t = s = 0.5
    tiny = np.array([[[10, 10, 10], [10.3, 10, 10], [10, 10.2, 10.1]]], np.float32) * unit
    got, _, st = check_against_numpy(engine_mod, tiny, None, pitch, change_range)
    assert st["samples"] == 1 and st["rows"] == 1
    rv = resident(engine_mod, tiny, change_range).astype(np.float64)
    p0, p1, p2 = rv[1], rv[2], rv[0]                     # the longest edge is bc
    assert same_bits(got[0], ((p0 + (p2 - p0) * 0.5) + (p1 - p0) * 0.25).astype(np.float32))
    # exact ties of the longest edge (coordinates that are exact in float, x1000 or not): the first of ab, bc, ca wins
    iso = np.array([[[0, 0, 0], [4, 3, 0], [8, 0, 0]]], np.float32)            # ab = bc = 25 < ca = 64: no tie at the top
    tie = np.array([[[0, 0, 0], [8, 0, 0], [4, 8, 0]]], np.float32)            # bc = ca = 80 > ab = 64: bc wins
    eq = np.array([[[8, 0, 0], [0, 8, 0], [0, 0, 8]]], np.float32)             # equilateral, ab = bc = ca = 128: ab wins
    for tri in (iso, tie, eq, eq[:, [1, 2, 0]], tie[:, [2, 0, 1]]):
        got, _, _ = check_against_numpy(engine_mod, tri * unit if not change_range else (tri / np.float32(1024)), None, pitch, change_range)
    # the tie rule in the sample order: the first sample sits beside p0, the start of the winning edge
    got, _, _ = check_against_numpy(engine_mod, tie, None, pitch, 0)
    d = np.linalg.norm(got[0] - tie[0], axis=1)
    assert d.argmin() == 1                               # bc won: p0 = b
    got, _, _ = check_against_numpy(engine_mod, eq, None, pitch, 0)
    assert np.linalg.norm(got[0] - eq[0], axis=1).argmin() == 0      # ab won: p0 = a
    # an indexed mesh with shared vertices gives what its soup gives
    verts = np.array([[0, 0, 0], [9, 0, 1], [9, 6, 1], [0, 6, 0]], np.float32) * unit
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    a = check_against_numpy(engine_mod, verts, tris, 0.7, change_range)
    b = check_against_numpy(engine_mod, verts[tris.ravel()], None, 0.7, change_range)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]


@pytest.mark.gpu
def test_skipped_triangles(engine_mod):
    rng = np.random.default_rng(21)
    good = rand_triangles(rng, 6, 3.0, 20.0).reshape(-1, 3)
    verts = np.concatenate([good, [[1, 1, 1], [2, 2, 2], [3, 3, 3], [np.nan, 0, 0], [np.inf, 1, 1]]]).astype(np.float32)
    g = np.arange(18).reshape(6, 3)
    tris = np.array([g[0], [18, 19, 20],                 # collinear
                     g[1], [0, 0, 5],                    # a repeated vertex
                     g[2], [0, 21, 2],                   # a NaN coordinate
                     g[3], [3, 4, 23],                   # an index out of range
                     [-1, 4, 5], g[4], [6, 22, 7],       # a negative index, an infinite coordinate
                     g[5]], np.int32)
    got, idx, st = check_against_numpy(engine_mod, verts, tris, 0.5)
    assert st["degenerate"] == 6 and st["sampled"] == 6 and st["culled"] == 0
    assert sorted(set(idx.tolist())) == [0, 2, 4, 6, 9, 11]          # tri_index skips them
    alone, idx2, _ = check_against_numpy(engine_mod, good, None, 0.5)
    assert same_bits(got, alone)                         # the other triangles' samples are unchanged
    assert same_bits(np.searchsorted([0, 2, 4, 6, 9, 11], idx).astype(np.int32), idx2)


@pytest.mark.gpu
def test_offsets_across_scan_blocks(engine_mod):
    rng = np.random.default_rng(31)
    small = rand_triangles(rng, 3000, 1.6, 150.0)
    big = np.array([[[-100, -100, 5], [110, -95, 9], [3, 101, -4]]], np.float32)        # about 400 rows at pitch 0.5
    v = np.concatenate([small[:1500], big, small[1500:]])
    e = engine_mod.Engine(0, change_range=0)
    got, idx, st = check_against_numpy(engine_mod, v, None, 0.5, engine=e)
    big_rows = st["rows"] - sample_mesh(np.concatenate([small[:1500], small[1500:]]).reshape(-1, 3), None, 0.5)[2]["rows"]
    assert 350 <= big_rows <= 450 and 6e4 <= st["samples"] <= 2e5 and (idx == 1500).sum() > 5e4
    again = e.set_cloud_mesh(v, None, pitch=0.5, tri_index=True)
    assert same_bits(again.pop("tri_index"), idx) and again == st and same_bits(e.cloud(), got)   # called twice: identical bits
    e.close()


def box_mesh():
    """an axis-aligned closed box, 12 triangles wound outward (counter-clockwise seen from outside)"""
    x, y, z = 40.0, 30.0, 20.0
    v = np.array([[0, 0, 0], [x, 0, 0], [x, y, 0], [0, y, 0], [0, 0, z], [x, 0, z], [x, y, z], [0, y, z]], np.float32)
    t = np.array([[0, 2, 1], [0, 3, 2],      # bottom, normal -z
                  [4, 5, 6], [4, 6, 7],      # top, +z
                  [0, 1, 5], [0, 5, 4],      # y = 0, -y
                  [2, 3, 7], [2, 7, 6],      # y = y, +y
                  [1, 2, 6], [1, 6, 5],      # x = x, +x
                  [3, 0, 4], [3, 4, 7]], np.int32)   # x = 0, -x
    return v, t


@pytest.mark.gpu
def test_facing(engine_mod):
    v, t = box_mesh()
    a, b, c = (v[t[:, i]].astype(np.float64) for i in range(3))
    n = np.cross(b - a, c - a)
    centre = v.mean(axis=0)
    assert (np.einsum("ij,ij->i", n, a - centre) > 0).all()          # wound outward
    vp = np.array([20, 15, 5000], np.float32)            # far above the centre
    _, idx, st = check_against_numpy(engine_mod, v, t, 0.5, facing=FRONT, viewpoint=vp)
    assert st["culled"] == 10 and st["sampled"] == 2 and st["degenerate"] == 0 and sorted(set(idx.tolist())) == [2, 3]
    _, idx, st = check_against_numpy(engine_mod, v, t, 0.5, facing=ALL, viewpoint=vp)
    assert st["culled"] == 0 and st["sampled"] == 12 and sorted(set(idx.tolist())) == list(range(12))


def sheet_mesh(nx=60, ny=40):
    from polishpathplanning_amd import synth
    pts = synth.make_plate(nx, ny, kind="wavy", amp=8.0, seed=9, permute=False)     # metres, grid order i * ny + j
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    p = (i * ny + j).ravel()
    tris = np.concatenate([np.stack([p, p + ny, p + 1], axis=1), np.stack([p + ny, p + ny + 1, p + 1], axis=1)]).astype(np.int32)
    return pts, tris


@pytest.mark.gpu
@pytest.mark.parametrize("slices", [None, (2, 5)])
def test_handle_state_is_set_clouds(engine_mod, slices):
    """engine A takes the mesh, engine B takes A's samples through ppp_set_cloud with change_range = 0: the same bounds, the same
    plan and list, the same deviation map of a scan against either.  A slice-range pair likewise (the map of such a handle is
    ppp_get_deviation_tile's, with the handle as the scan: ppp_get_deviation refuses slice ranges)."""
    pts, tris = sheet_mesh()
    kw = dict(tool_radius=6.0, walk=1)
    if slices:
        kw.update(slice_begin=slices[0], slice_end=slices[1])
    mm = (pts * np.float32(1000)).astype(np.float32)
    A = engine_mod.Engine(0, change_range=0, **kw)
    st = A.set_cloud_mesh(mm, tris, pitch=0.5)
    samples = A.cloud()
    assert 2e4 <= st["samples"] == len(samples) <= 4e4 and st["degenerate"] == 0 and st["triangles"] == 2 * 59 * 39
    B = engine_mod.Engine(0, change_range=0, **kw)
    B.set_cloud(samples)
    assert same_bits(samples, B.cloud())
    for x, y in zip(A.minmax(), B.minmax()):
        assert same_bits(x, y)
    SA, SB = A.gen_path(), B.gen_path()
    WA, WB = A.get_path(), B.get_path()
    assert SA == SB and WA == WB and WA > 10
    # (a slice-range handle's list ends before postion_smooth: its rows are the stage in front of it)
    wp = (lambda e: e.stage(engine_mod.STAGE_WP_PRESMOOTH)) if slices else (lambda e: e.waypoints())
    assert len(wp(A)) == WA and same_bits(wp(A), wp(B))
    assert A.fast_path() == B.fast_path()
    # with ChangeRange the mesh is in metres: the same resident cloud (no second x1000), the same plan, the same sampled points
    whole = engine_mod.Engine(0, change_range=1, **kw)
    assert whole.set_cloud_mesh(pts, tris, pitch=0.5) == st and same_bits(whole.cloud(), samples)
    for x, y in zip(whole.minmax(), B.minmax()):
        assert same_bits(x, y)
    assert (whole.gen_path(), whole.get_path()) == (SB, WB)
    assert same_bits(whole.stage(engine_mod.STAGE_WP_XYZ), B.stage(engine_mod.STAGE_WP_XYZ))
    shifted = (A.cloud() + np.float32([0.21, -0.13, 0.2])).astype(np.float32)[::3]
    scan = engine_mod.Engine(0, change_range=0, tool_radius=6.0, walk=1)
    scan.set_cloud(shifted)
    if not slices:
        ra, rb = scan.deviation(A, max_dist=3.0), scan.deviation(B, max_dist=3.0)
        assert ra[5]["matched"] > 0.9 * len(shifted)
    else:
        ra, rb = A.deviation_tile(scan, 3.0, max_dist=3.0), B.deviation_tile(scan, 3.0, max_dist=3.0)
        assert ra[6]["matched"] > 100
    for x, y in zip(ra[:-1], rb[:-1]):
        assert same_bits(x, y)
    assert repr(ra[-1]) == repr(rb[-1])                  # (repr: NaN statistics compare equal to themselves)
    for e in (whole, A, B, scan):
        e.close()


@pytest.mark.gpu
def test_flat_plate_deviates_by_its_lift(engine_mod):
    rng = np.random.default_rng(8)
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    ax, ay, n = q[:, 0], q[:, 1], q[:, 2]
    c = np.array([12.0, -7.0, 20.0])
    vp = (c + 900.0 * n).astype(np.float32)              # the sensor: on the side the normal points to
    corner = lambda u, v: c + u * ax + v * ay
    verts = np.array([corner(0, 0), corner(40, 0), corner(40, 30), corner(0, 30)], np.float32)
    ref = engine_mod.Engine(0, change_range=0)
    st = ref.set_cloud_mesh(verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32), pitch=0.5, viewpoint=vp)
    assert 0.9 * 4800 <= st["samples"] <= 1.15 * 4800    # about 1 / pitch^2 per mm^2 (the last column of a row is rounded up)
    u, v = np.meshgrid(np.arange(0.35, 40, 0.7), np.arange(0.35, 30, 0.7), indexing="ij")
    u, v = u.ravel(), v.ravel()
    pts = (c + u[:, None] * ax + v[:, None] * ay + 0.3 * n).astype(np.float32)
    scan = engine_mod.Engine(0, change_range=0)
    scan.set_cloud(pts)
    dev, _, _, status, _, stats = scan.deviation(ref, max_dist=2.0)
    nr = ref.params.normal_radius
    inner = (u > nr) & (u < 40 - nr) & (v > nr) & (v < 30 - nr)
    assert (status[inner] == 0).all() and inner.sum() > 1000
    err = np.abs(dev[inner] - 0.3).max()
    print("flat plate: %d inner points, largest |deviation - 0.3| = %.3e mm" % (inner.sum(), err))
    assert err <= 1e-3
    ref.close(); scan.close()


@pytest.mark.gpu
def test_errors_leave_the_handle_as_it_was(engine_mod, tmp_path):
    import ctypes as C
    E = engine_mod
    from polishpathplanning_amd import synth
    pts, cfg = synth.make_config("tiny_5k")
    e = E.Engine(0, tool_radius=cfg["tool_radius"])
    e.set_cloud(pts)
    e.gen_path(); e.get_path()
    cloud0, wp0 = e.cloud(), e.waypoints()
    tri = RIGHT.reshape(-1, 3) * np.float32(0.001)
    L = e.L
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    v = tri.ctypes.data_as(fp)

    def unchanged():
        assert same_bits(e.cloud(), cloud0)
        e.gen_path(); e.get_path()
        assert same_bits(e.waypoints(), wp0)

    def call(verts=v, n_verts=3, tris=None, n_tris=1, pitch=0.5, facing=ALL, mp="make", stats=None):
        if mp == "make":
            mp = C.byref(E.MeshParams(pitch, facing))
        return L.ppp_set_cloud_mesh(e.h, verts, n_verts, tris, n_tris, mp, None, None, 0, stats)

    st = E.MeshStats()
    cases = dict(no_verts=dict(verts=None), no_params=dict(mp=None), pitch_zero=dict(pitch=0.0), pitch_negative=dict(pitch=-1.0),
                 pitch_nan=dict(pitch=float("nan")), pitch_inf=dict(pitch=float("inf")), facing=dict(facing=2), facing_neg=dict(facing=-1),
                 soup_count=dict(n_verts=3, n_tris=2), soup_count2=dict(n_verts=4, n_tris=1), no_triangles=dict(n_tris=0, n_verts=0))
    for name, kw in cases.items():
        assert call(**kw) == E.ERR_ARG, name
        unchanged()
    # every triangle degenerate, or culled: no sample
    flat = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 0, 0], [0, 0, 0], [5, 5, 5]], np.float32)
    assert call(verts=flat.ctypes.data_as(fp), n_verts=6, n_tris=2, stats=C.byref(st)) == E.ERR_ARG
    assert (st.triangles, st.degenerate, st.sampled, st.rows, st.samples) == (2, 2, 0, 0, 0)
    assert "no sample" in L.ppp_last_error(e.h).decode()
    unchanged()
    back = RIGHT.reshape(-1, 3) * np.float32(0.001) + np.float32([0, 0, 1])   # its normal points to +z: the origin sees its back
    assert call(verts=back.ctypes.data_as(fp), facing=FRONT, stats=C.byref(st)) == E.ERR_ARG and st.culled == 1 and st.sampled == 0
    unchanged()
    with pytest.raises(E.PPPError) as ex:
        e.set_cloud_stl(str(tmp_path / "missing.stl"))
    assert ex.value.code == E.ERR_IO
    unchanged()
    # more samples than a resident cloud holds: refused before anything is allocated for them
    huge = np.array([[0, 0, 0], [30, 0, 0], [0, 30, 0]], np.float32)                     # 30 m x 30 m at 1 um
    assert call(verts=huge.ctypes.data_as(fp), pitch=1e-3, stats=C.byref(st)) == E.ERR_CAPACITY
    unchanged()
    # cap smaller than the sample count: only cap entries are written
    idx = np.full(64, -7, np.int32)
    mp = E.MeshParams(0.5, ALL)
    two = np.concatenate([tri, tri + np.float32(0.01)])
    assert L.ppp_set_cloud_mesh(e.h, two.ctypes.data_as(fp), 6, None, 2, C.byref(mp), None, idx.ctypes.data_as(ip), 5, C.byref(st)) == 0
    assert st.samples > 60 and (idx[:5] == 0).all() and (idx[5:] == -7).all()
    full = e.set_cloud_mesh(two, None, tri_index=True)
    assert full["samples"] == st.samples and (np.diff(full["tri_index"]) >= 0).all() and full["tri_index"][-1] == 1
    e.close()
    # a part handle (ppp_set_cloud_part)
    scaled = (pts * np.float32(1000)).astype(np.float32)
    mn, mx = scaled.min(axis=0), scaled.max(axis=0)
    p = E.Engine(0, tool_radius=cfg["tool_radius"], slice_begin=2, slice_end=9)
    lo, hi, _ = p.range_interval(mn[0], mx[0])
    keep = np.nonzero((scaled[:, 0] >= lo) & (scaled[:, 0] <= hi))[0]
    p.set_cloud_part(pts[keep], keep, mn, mx, len(pts), lo, hi)
    p.gen_path(); p.get_path()
    c0, w0 = p.cloud(), p.stage(E.STAGE_WP_PRESMOOTH)     # (a slice range's list ends before postion_smooth)
    assert len(w0) > 10
    with pytest.raises(E.PPPError) as ex:
        p.set_cloud_mesh(tri)
    assert ex.value.code == E.ERR_UNSUPPORTED
    assert same_bits(p.stage(E.STAGE_WP_PRESMOOTH), w0)  # the finished pass is still there
    p.gen_path(); p.get_path()
    assert same_bits(p.cloud(), c0) and same_bits(p.stage(E.STAGE_WP_PRESMOOTH), w0)
    p.close()


@pytest.mark.gpu
def test_planner_takes_a_mesh(engine_mod, tmp_path):
    """examples/api_check with a third argument: ppp::Planner::set_mesh of the arrays and Planner::open of the .stl file"""
    from polishpathplanning_amd import synth
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "api_check"], stdout=subprocess.DEVNULL)
    pcd, stl = str(tmp_path / "c.pcd"), str(tmp_path / "plate.STL")
    engine_mod.save_pcd(pcd, synth.make_config("tiny_5k")[0])
    r = subprocess.run([os.path.join(ROOT, "examples", "api_check"), pcd, "35", stl], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    line = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("mesh ")][0]
    e = engine_mod.Engine(0)
    n = e.set_cloud_stl(stl)["samples"]
    e.close()
    assert [int(x) for x in line[1:]] == [1, 2, n, n, n, n] and n > 4000


@pytest.mark.gpu
def test_stl_on_the_device_path(engine_mod, tmp_path):
    pts, tris = sheet_mesh(24, 16)
    tris = np.ascontiguousarray(tris[:, ::-1])           # wound to face the sensor at the origin (the sheet hangs at z = 1.5 m)
    v9 = pts[tris.ravel()].reshape(-1, 9)
    vp = np.array([0, 0, 0], np.float32)
    a = engine_mod.Engine(0)
    sa = a.set_cloud_mesh(pts, tris, pitch=0.4, facing=FRONT, viewpoint=vp)
    for binary in (True, False):
        p = str(tmp_path / ("m%d.stl" % binary))
        engine_mod.save_stl(p, v9, binary=binary)
        b = engine_mod.Engine(0)
        sb = b.set_cloud_stl(p, pitch=0.4, facing=FRONT, viewpoint=vp)
        assert sb == sa and sb["samples"] > 3000 and same_bits(a.cloud(), b.cloud())
        b.close()
    a.close()
