"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_box.hpp (test harness; see clip_box_host.cpp), the cases of
the tests of radfoam.cell_geometry_in_box, and the checks the CPU and GPU tests share.  Every check takes the operator's
outputs as numpy arrays (``out``: volume, centroid, nonempty, face_area, face_vertices, wall_area, wall_vertices) and
does not care where they were computed."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_box_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_box_host.cpp"), os.path.join(_CSRC, "rf_clip_box.hpp"),
        os.path.join(_CSRC, "rf_clip.hpp")]

BAR = 1e-9      # |dV| <= BAR s^3, |dc| <= BAR s, |dA| <= BAR s^2, s = V_exact^(1/3) of the cell: clip_host's bar and unit


def build():
    if os.path.exists(_SO) and all(os.path.getmtime(s) <= os.path.getmtime(_SO) for s in _SRC):
        return _SO
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _SO, _SRC[0]],
                   check=True)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.clip_box_host_cell_box.restype = C.c_int
        _lib.clip_box_host_cell_box.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_uint32] + [C.c_void_p] * 8
    return _lib


OUT_KEYS = ("volume", "centroid", "nonempty", "face_area", "face_vertices", "wall_area", "wall_vertices")


def cell_box(points, adjacency, offsets, box, cap: int = 256) -> dict:
    """The host build of the serial cell over every cell: what cell_geometry_in_box's runner returns, as numpy, plus the
    per-cell status (0 ok, 1 a face outgrew ``cap`` vertices, 2 bad row) and ``bad``, the number of cells not ok."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    six = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
    assert six.shape == (6,)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    out = dict(volume=np.empty(n), centroid=np.empty((n, 3)), nonempty=np.empty(n, dtype=np.uint8),
               face_area=np.empty(e), face_vertices=np.empty(e, dtype=np.uint32), wall_area=np.empty((n, 6)),
               wall_vertices=np.empty((n, 6), dtype=np.uint32), status=np.empty(n, dtype=np.uint32))
    out["bad"] = lib().clip_box_host_cell_box(pts.ctypes.data, n, adj.ctypes.data, off.ctypes.data, e, bbox.ctypes.data,
                                              six.ctypes.data, cap, *(out[k].ctypes.data for k in OUT_KEYS + ("status",)))
    out["nonempty"] = out["nonempty"].astype(bool)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------

def _cube(lo, hi, shift=(0.0, 0.0, 0.0), scale=1.0):
    return tuple(scale * lo + s for s in shift) + tuple(scale * hi + s for s in shift)


HUB_BOX = (-4.5, -4.5, -4.5, 0.3, 4.5, 4.5)         # its +x wall cuts the hub cell in a 14-gon (hub58) / 15-gon (hub59)
RING_BOX = (-5.0, -5.0, -5.0, 5.0, 5.0, 0.1)        # its +z wall cuts site 1's cell in the ring's k-gon
GRID_BOXES = {"grid_between": _cube(-0.625, 0.875), "grid_sites": _cube(-0.5, 0.75), "grid_bisectors": _cube(-0.375, 0.625)}

# name -> (cloud, box, the cells the exact reference works on: a tuple, or None for pick_cells)
CASES = {
    "uniform400": ("uniform400", _cube(-1.0, 1.0), None),
    "tight": ("uniform400", (-0.6, -0.5, -0.7, 0.7, 0.6, 0.5), None),
    "wide": ("uniform400", _cube(-50.0, 50.0), None),
    "disjoint": ("uniform400", _cube(2.0, 3.0), None),
    "offset": ("offset", _cube(-1.0, 1.0, shift=(1000.0, -2000.0, 500.0)), None),
    "scaled_small": ("scaled_small", _cube(-1.0, 1.0, scale=2.0 ** -10), None),
    "scaled_large": ("scaled_large", _cube(-1.0, 1.0, scale=2.0 ** 10), None),
    "hub58": ("hub58", HUB_BOX, (0,)), "hub59": ("hub59", HUB_BOX, (0,)),
    "ring16": ("ring16", RING_BOX, (0, 1)), "ring17": ("ring17", RING_BOX, (0, 1)),
    "ring256": ("ring256", RING_BOX, (0, 1)),
    "redo_spread": ("redo_spread", _cube(-9.5, 9.5), ()),
    "grid_between": ("grid", GRID_BOXES["grid_between"], ()), "grid_sites": ("grid", GRID_BOXES["grid_sites"], ()),
    "grid_bisectors": ("grid", GRID_BOXES["grid_bisectors"], ()),
}

_CLOUDS = dict(H._CLOUDS, hub58=lambda: H.hub_cloud(58), hub59=lambda: H.hub_cloud(59))
_CSR, _HOST, _GEO = {}, {}, {}


def cloud(name: str) -> dict:
    """points, Qhull's CSR and the row of every slot of a named cloud; once per process, never modified"""
    if name not in _CSR:
        from radfoam_amd import foam

        pts = _CLOUDS[name]()
        assert pts.dtype == np.float32
        off, adj = foam.delaunay_csr(pts)
        _CSR[name] = dict(points=pts, offsets=off, adjacency=adj,
                          rows=np.repeat(np.arange(pts.shape[0]), np.diff(off.astype(np.int64))))
    return _CSR[name]


def case(name: str) -> dict:
    cl, box, _ = CASES[name]
    return dict(cloud(cl), box=np.array(box, dtype=np.float64), name=name)


def host(name: str, cap: int = 256) -> dict:
    """the host build's answer for a case, once"""
    if (name, cap) not in _HOST:
        c = case(name)
        _HOST[(name, cap)] = cell_box(c["points"], c["adjacency"], c["offsets"], c["box"], cap=cap)
    return _HOST[(name, cap)]


def write_arrays(name: str, path: str):
    """a case as the plain arrays tests/host_harness/clip_box_sanitize.cpp reads"""
    c = case(name)
    pts = np.ascontiguousarray(c["points"], dtype=np.float32)
    adj, off = c["adjacency"].astype(np.uint32), c["offsets"].astype(np.uint32)
    with open(path, "wb") as f:
        for part in (np.array([len(pts), len(adj)], dtype=np.uint32), pts, adj, off, H.bbox_of(pts), c["box"]):
            f.write(np.ascontiguousarray(part).tobytes())


def host_geometry(cloud_name: str) -> dict:
    """clip_host.cell_geometry (the unclipped cells) of a cloud, once"""
    if cloud_name not in _GEO:
        c = cloud(cloud_name)
        _GEO[cloud_name] = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])
    return _GEO[cloud_name]


def pick_cells(points: np.ndarray, box: np.ndarray) -> tuple:
    """The cells the exact reference works on where a case lists none, chosen from the sites' positions alone: the sites
    nearest to the box's 8 corners, 12 edge midpoints and 6 wall centres, the 40 sites inside the box that are nearest to
    a wall, the 12 nearest to the box's centre, and of the sites outside the box the 12 nearest to it and the 12 farthest
    from it."""
    p = points.astype(np.float64)
    lo, hi = box[:3], box[3:]
    mid = 0.5 * (lo + hi)
    picks = []
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                if (i, j, k) != (0, 0, 0):
                    target = mid + 0.5 * (hi - lo) * np.array([i, j, k])
                    picks.append(int(np.argmin(((p - target) ** 2).sum(1))))
    outside = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inside = np.nonzero(outside == 0.0)[0]
    to_wall = np.minimum(p - lo, hi - p).min(1)
    picks += inside[np.argsort(to_wall[inside])[:40]].tolist()
    picks += np.argsort(((p - mid) ** 2).sum(1))[:12].tolist()
    out = np.nonzero(outside > 0.0)[0]
    order = out[np.argsort(outside[out])]
    picks += order[:12].tolist() + order[-12:].tolist()
    return tuple(sorted(set(picks)))


def exact(name: str) -> dict:
    from tests import cell_box_ref as X

    c = case(name)
    cells = CASES[name][2]
    if cells is None:
        cells = pick_cells(c["points"], c["box"])
    return X.exact_cells_in_box(c["points"], c["offsets"], c["adjacency"], c["box"], cells)


# ---- the checks ----------------------------------------------------------------------------------------------------------

def box_volume(box) -> float:
    return float((box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]))


def wall_rectangles(box) -> np.ndarray:
    ex, ey, ez = box[3] - box[0], box[4] - box[1], box[5] - box[2]
    return np.array([ey * ez, ey * ez, ex * ez, ex * ez, ex * ey, ex * ey])


def check_shapes(c: dict, out: dict):
    n, e = len(c["points"]), len(c["adjacency"])
    assert out["volume"].shape == (n,) and out["centroid"].shape == (n, 3) and out["nonempty"].shape == (n,)
    assert out["face_area"].shape == (e,) and out["face_vertices"].shape == (e,)
    assert out["wall_area"].shape == (n, 6) and out["wall_vertices"].shape == (n, 6)
    assert out["volume"].dtype == np.float64 and out["face_area"].dtype == np.float64
    assert out["nonempty"].dtype == bool and np.array_equal(out["nonempty"], out["volume"] > 0)


def check_against_exact(name: str, out: dict, vertices: bool = True) -> tuple:
    """Check 1: on the cells the exact reference worked on, |dV| <= 1e-9 s^3, |dc| <= 1e-9 s and |dA| <= 1e-9 s^2 for the
    row's faces and the walls, s = V_exact^(1/3) of the cell; a cell that is empty in exact arithmetic (s = 0) has volume
    0, centroid NaN, every area 0 and nonempty False.  ``vertices``: every polygon has the reference's distinct-vertex
    count.  Returns the worst ratios (volume, centroid, face area, wall area)."""
    c, ref = case(name), exact(name)
    check_shapes(c, out)
    cells = np.nonzero(ref["done"])[0]
    assert len(cells)
    slot_of_done = ref["done"][c["rows"]]
    empty = ref["done"] & (ref["volume_f"] == 0.0)
    solid = ref["done"] & ~empty
    assert not any(v == 0 for a, v in ref["volume"].items() if solid[a])          # 0 as a float is 0 as a Fraction
    if empty.any():
        assert (out["volume"][empty] == 0.0).all() and np.isnan(out["centroid"][empty]).all()
        assert not out["nonempty"][empty].any() and (out["wall_area"][empty] == 0.0).all()
        assert (out["face_area"][empty[c["rows"]]] == 0.0).all()
    s = np.cbrt(ref["volume_f"])
    rv = (np.abs(out["volume"][solid] - ref["volume_f"][solid]) / s[solid] ** 3).max()
    assert out["nonempty"][solid].all()
    rc = (np.abs(out["centroid"][solid] - ref["centroid_f"][solid]).max(1) / s[solid]).max()
    of_solid = solid[c["rows"]]
    ra = (np.abs(out["face_area"][of_solid] - ref["face_area"][of_solid]) / s[c["rows"]][of_solid] ** 2).max()
    rw = (np.abs(out["wall_area"][solid] - ref["wall_area"][solid]).max(1) / s[solid] ** 2).max()
    print(f"{name}: {solid.sum()} solid and {empty.sum()} empty cells compared: |dV| / s^3 = {rv:.3g}, |dc| / s = {rc:.3g}, "
          f"|dA| / s^2 = {ra:.3g} (faces) {rw:.3g} (walls) (bar {BAR:.3g})")
    assert rv <= BAR and rc <= BAR and ra <= BAR and rw <= BAR
    if vertices:
        assert np.array_equal(out["face_vertices"][slot_of_done].astype(np.int64), ref["face_vertices"][slot_of_done])
        assert np.array_equal(out["wall_vertices"][ref["done"]].astype(np.int64), ref["wall_vertices"][ref["done"]])
    return rv, rc, ra, rw


def mates(c: dict) -> np.ndarray:
    """the slot of (b -> a) for every slot (a -> b) of a symmetric CSR"""
    rows, adj, n = c["rows"], c["adjacency"].astype(np.int64), len(c["points"])
    key = rows * n + adj
    order = np.argsort(key)
    back = order[np.searchsorted(key[order], adj * n + rows)]
    assert (adj[back] == rows).all() and (rows[back] == adj).all()
    return back


def check_identities(c: dict, out: dict, partition: bool = True, walls: bool = True, cells=None) -> tuple:
    """Check 2, on a whole cloud with a symmetric CSR and without any reference, to the bar 1e-9 in the units of check 1
    (s from the code's own volumes), each bound the per-cell bar summed over what the identity adds up:

      sum V = V_box, sum V c = V_box centre (unit V_box |diagonal|) and, per wall, sum wall_area = the wall's rectangle
      (``partition`` / ``walls``: the cells of a Delaunay CSR partition the box);
      face_area[a->b] == face_area[b->a] on every slot, to 1e-9 (s_a^2 + s_b^2); where both cells are flat or empty
      (s = 0 gives no unit, and a flat cell's faces are as large as its solid neighbours') to 1e-9 of the mean cell's
      (V_box / N)^(2/3);
      per non-empty cell the area vectors of its faces and walls close, to 1e-9 s^2, and volume == the signed pyramid
      sum, to 1e-9 s^3;
      every output is finite, except the centroid where nonempty is False.

    ``cells``: the cells the two per-cell identities are asked of, in place of the non-empty ones, and the only ones
    with a size of their own in the symmetry's unit (where the others are known to be flat, and come out with a volume
    of a few ulps on either side of 0 by rounding)."""
    check_shapes(c, out)
    box, pts = c["box"], c["points"].astype(np.float64)
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    vol, ne = out["volume"], out["nonempty"]
    assert np.isfinite(vol).all() and np.isfinite(out["face_area"]).all() and np.isfinite(out["wall_area"]).all()
    assert np.isfinite(out["centroid"][ne]).all() and np.isnan(out["centroid"][~ne]).all()
    vbox, diag = box_volume(box), float(np.linalg.norm(box[3:] - box[:3]))
    worst = {}
    if partition:
        worst["sum V"] = abs(vol.sum() - vbox) / vbox
        first = (vol[ne, None] * out["centroid"][ne]).sum(0)
        worst["sum V c"] = float(np.linalg.norm(first - vbox * 0.5 * (box[:3] + box[3:]))) / (vbox * diag)
    if walls:
        worst["walls"] = float((np.abs(out["wall_area"].sum(0) - wall_rectangles(box)) / wall_rectangles(box)).max())
    s = np.cbrt(np.maximum(vol, 0.0))
    back = mates(c)
    solid = s if cells is None else np.where(np.asarray(cells, dtype=bool), s, 0.0)
    pair = solid[rows] ** 2 + solid[adj] ** 2
    pair[pair == 0.0] = (vbox / len(pts)) ** (2.0 / 3.0)
    diff = np.abs(out["face_area"] - out["face_area"][back])
    worst["symmetry"] = float((diff / pair).max()) if len(diff) else 0.0
    d = pts[adj] - pts[rows]
    length = np.linalg.norm(d, axis=1)
    n = len(pts)
    closed, pyr = np.zeros((n, 3)), np.zeros(n)
    np.add.at(closed, rows, out["face_area"][:, None] * d / length[:, None])
    np.add.at(pyr, rows, out["face_area"] * length / 6.0)
    h = np.stack([pts[:, 0] - box[0], box[3] - pts[:, 0], pts[:, 1] - box[1], box[4] - pts[:, 1], pts[:, 2] - box[2],
                  box[5] - pts[:, 2]], axis=1)
    normal = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.float64)
    closed += out["wall_area"] @ normal
    pyr += (out["wall_area"] * h).sum(1) / 3.0
    per = ne if cells is None else np.asarray(cells, dtype=bool)
    if per.any():
        assert ne[per].all()
        worst["closure"] = float((np.linalg.norm(closed[per], axis=1) / s[per] ** 2).max())
        worst["pyramids"] = float((np.abs(pyr[per] - vol[per]) / s[per] ** 3).max())
    print(f"{c.get('name', '')}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (bar {BAR:.3g}); "
          f"{ne.sum()} of {n} cells non-empty")
    assert all(v <= BAR for v in worst.values()), worst
    return worst


def check_agreement(c: dict, out: dict, geo: dict, share=None) -> int:
    """Check 3: on every cell cell_geometry calls bounded and whose wall_area is all zero, volume, centroid and face areas
    agree with cell_geometry's to 2e-9 in the units of check 1 (each is within 1e-9 of exact; the two start from squares
    of different half-sides, so their bits may differ).  ``share``: at least that part of the cloud is such a cell."""
    free = geo["bounded"] & (out["wall_area"] == 0.0).all(1)
    print(f"{c.get('name', '')}: {free.sum()} of {free.size} cells are bounded and touch no wall")
    if share is not None:
        assert free.sum() >= share * free.size
    if not free.any():
        return 0
    s = np.cbrt(geo["volume"][free])
    rv = (np.abs(out["volume"][free] - geo["volume"][free]) / s ** 3).max()
    rc = (np.abs(out["centroid"][free] - geo["centroid"][free]).max(1) / s).max()
    of_free = free[c["rows"]]
    sf = np.cbrt(geo["volume"][c["rows"]][of_free])
    ra = (np.abs(out["face_area"][of_free] - geo["face_area"][of_free]) / sf ** 2).max()
    print(f"    |dV| / s^3 = {rv:.3g}, |dc| / s = {rc:.3g}, |dA| / s^2 = {ra:.3g} (bar {2 * BAR:.3g})")
    assert rv <= 2 * BAR and rc <= 2 * BAR and ra <= 2 * BAR
    assert np.array_equal(out["face_vertices"][of_free], geo["face_vertices"][of_free])
    return int(free.sum())


def check_whole_box(box, out: dict, a: int):
    """cell a is the whole box: the volume the product the code forms, the centre, the six rectangles"""
    box = np.asarray(box, dtype=np.float64)
    ex, ey, ez = box[3] - box[0], box[4] - box[1], box[5] - box[2]
    assert out["volume"][a] == ex * ey * ez and out["nonempty"][a]
    assert np.array_equal(out["centroid"][a], 0.5 * (box[:3] + box[3:]))
    assert np.array_equal(out["wall_area"][a], wall_rectangles(box)) and (out["wall_vertices"][a] == 4).all()


def check_grid(name: str, out: dict):
    """Check 5, the unjittered grid (spacing 0.25) in its three boxes: the cells partition the box; in 'grid_between'
    every interior cell keeps its volume 0.25^3; in 'grid_bisectors' the walls are bisector planes of the first layer:
    the row's face keeps the area 0.0625 and the wall gets 0 there, and the flat cells outside have |volume| <= 1e-9 0.25^3
    (the wall identity is not asserted in that box)."""
    c = case(name)
    h = H.GRID_H
    pts, box = c["points"].astype(np.float64), c["box"]
    if name == "grid_bisectors":      # the cells outside are flat: the per-cell identities are asked of the 64 inside
        check_identities(c, out, walls=False, cells=((pts > box[:3]) & (pts < box[3:])).all(1))
    else:
        check_identities(c, out)
    if name == "grid_between":
        inner = H.grid_interior()
        assert np.abs(out["volume"][inner] - h ** 3).max() <= BAR * h ** 3
    if name == "grid_sites":
        on_wall = ((pts == box[:3]) | (pts == box[3:])).any(1)
        assert on_wall.sum() > 0 and out["nonempty"][on_wall & ((pts >= box[:3]) & (pts <= box[3:])).all(1)].all()
    if name == "grid_bisectors":
        inside = ((pts > box[:3]) & (pts < box[3:])).all(1)
        assert inside.sum() == 64 and np.abs(out["volume"][inside] - h ** 3).max() <= BAR * h ** 3
        assert np.abs(out["volume"][~inside]).max() <= BAR * h ** 3
        rows, adj = c["rows"], c["adjacency"].astype(np.int64)
        d = pts[adj] - pts[rows]
        axis = np.abs(d).sum(1) == h                                               # an axis neighbour
        hits = 0
        for w in range(6):
            k, sign = w // 2, (1.0 if w % 2 else -1.0)
            wall_at = box[3 + k] if w % 2 else box[k]
            first = inside & (np.abs(pts[:, k] + sign * 0.5 * h - wall_at) == 0.0)    # the layer whose bisector is the wall
            assert first.sum() == 16
            slot = first[rows] & axis & (d[:, k] == sign * h)
            assert slot.sum() == 16
            assert np.abs(out["face_area"][slot] - h * h).max() <= BAR * h * h
            assert (out["wall_area"][first, w] == 0.0).all()
            hits += int(slot.sum())
        assert hits == 96
