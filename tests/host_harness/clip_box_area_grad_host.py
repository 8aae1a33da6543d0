"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_box_area_grad.hpp (test harness; see
clip_box_area_grad_host.cpp), and the checks the CPU and GPU tests of radfoam.face_area_in_box_grad share.  A check takes
a case ``c`` (points, adjacency, offsets, rows, box), the forward's answer ``out`` for it (volume, centroid, nonempty,
face_area, wall_area as numpy) and ``run``, a callable ``run(c, out, grad_face_area, grad_wall_area) -> grad f64[N,3]``
(numpy; either upstream may be None), and does not care where ``run`` computes."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_box_area_grad_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_box_area_grad_host.cpp")] + [os.path.join(_CSRC, n) for n in (
    "rf_clip_box_area_grad.hpp", "rf_clip_area_grad.hpp", "rf_clip_box.hpp", "rf_clip.hpp")]

ROW_BAR = 1e-9          # per row, with the O(1) rows of unit upstreams: the bar of the cell-geometry gradients
CLOSURE_BAR = 1e-9      # the closure identity, of sum |p_a| |term_a|: the unit of clip_area_grad_host.check_identities
AGREEMENT_BAR = 2e-9    # against face_area_grad away from the walls: the forward's agreement bar
LABEL_BAR = 1e-10       # an edge's end points on its label's plane, of the face's size
NO_LABEL = 0xFFFFFFFF
WALL_COLUMNS = np.array([0.75, -0.5, 1.25, 0.375, -1.125, 0.875])     # a grad_wall_area constant down each column
NORMALS = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.float64)


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
        _lib.clip_box_area_grad_host_run.restype = C.c_int
        _lib.clip_box_area_grad_host_run.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
        _lib.clip_box_area_grad_host_polygon.restype = C.c_int
        _lib.clip_box_area_grad_host_polygon.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 3 + [C.c_void_p] * 2
        _lib.clip_box_area_grad_host_same_vertices.restype = C.c_int
        _lib.clip_box_area_grad_host_same_vertices.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 3
    return _lib


def _f64(x, shape):
    if x is None:
        return None
    out = np.ascontiguousarray(x, dtype=np.float64)
    assert out.shape == shape
    return out


def _arrays(points, adjacency, offsets, box):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    six = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
    assert six.shape == (6,)
    return pts, adj, off, six, (H.bbox_of(pts) if pts.shape[0] else np.zeros(6, dtype=np.float32))


def cell_box_area_grad(points, adjacency, offsets, box, geo: dict, grad_face_area, grad_wall_area, cap: int = 256) -> dict:
    """The host build of the pre-pass and of the serial row over every cell: grad f64[N,3], status u32[N] (0 ok, 1 a face
    outgrew ``cap`` vertices, 2 bad row) and ``bad``.  ``geo`` is what clip_box_host.cell_box returned for the same cloud
    and box; either upstream may be None."""
    pts, adj, off, six, bbox = _arrays(points, adjacency, offsets, box)
    n, e = pts.shape[0], adj.shape[0]
    ne = np.ascontiguousarray(geo["nonempty"], dtype=np.uint8)
    fa, wa = _f64(geo["face_area"], (e,)), _f64(geo["wall_area"], (n, 6))
    g, gw = _f64(grad_face_area, (e,)), _f64(grad_wall_area, (n, 6))
    grad, status = np.empty((n, 3)), np.empty(n, dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data
    bad = lib().clip_box_area_grad_host_run(ptr(pts), n, ptr(adj), ptr(off), e, ptr(bbox), ptr(six), cap, ptr(ne), ptr(fa),
                                            ptr(wa), ptr(g), ptr(gw), ptr(grad), ptr(status))
    return dict(grad=grad, status=status, bad=bad)


def labelled_polygon(c: dict, a: int, i: int, cap: int = 256):
    """(xyz f64[m,3] relative to p_a, label u32[m]) of row face i of cell a as the serial row clips it, and whether the
    unlabelled clipping gives the same vertices bit for bit; None past ``cap``"""
    pts, adj, off, six, bbox = _arrays(c["points"], c["adjacency"], c["offsets"], c["box"])
    xyz, label = np.empty((cap, 3)), np.empty(cap, dtype=np.uint32)
    args = (pts.ctypes.data, adj.ctypes.data, off.ctypes.data, bbox.ctypes.data, six.ctypes.data, cap, a, i)
    m = lib().clip_box_area_grad_host_polygon(*args, xyz.ctypes.data, label.ctypes.data)
    if m < 0:
        return None
    return xyz[:m].copy(), label[:m].copy(), bool(lib().clip_box_area_grad_host_same_vertices(*args))


def host_run(c: dict, out: dict, g, gw) -> np.ndarray:
    got = cell_box_area_grad(c["points"], c["adjacency"], c["offsets"], c["box"], out, g, gw)
    assert got["bad"] == 0
    return got["grad"]


def write_arrays(name: str, path: str):
    """a case (of tests/cell_box_grad_ref.FD_CASES, else of clip_box_host.CASES) as the plain arrays
    tests/host_harness/clip_box_area_grad_sanitize.cpp reads"""
    from tests.host_harness import clip_box_grad_host as BG

    BG.write_arrays(name, path)


_FORWARD = {}


def host_forward(key, c: dict) -> dict:
    """clip_box_host.cell_box of a case, once"""
    if key not in _FORWARD:
        _FORWARD[key] = B.cell_box(c["points"], c["adjacency"], c["offsets"], c["box"])
        assert _FORWARD[key]["bad"] == 0
    return _FORWARD[key]


def with_rows(c: dict) -> dict:
    if "rows" not in c:
        c = dict(c, rows=np.repeat(np.arange(len(c["points"])), np.diff(np.asarray(c["offsets"]).astype(np.int64))))
    return c


def unit_upstreams(c: dict, out: dict, seed: int = 0):
    """(g f64[E], gw f64[N,6]): r / s_a per slot and per wall of cell a, r uniform in [-1,1] and s_a = V_a^(1/3), so that
    g A is of the order of the cell's size and the rows of the gradient are O(1).  The two slots of a face draw their own
    r.  On the empty cells (s_a = 1) the draws stay finite; check_empty_cells_are_ignored overwrites them."""
    rng = np.random.default_rng(seed)
    c = with_rows(c)
    ne = out["nonempty"]
    size = np.cbrt(np.where(ne, out["volume"], 1.0))
    g = rng.uniform(-1.0, 1.0, len(c["adjacency"])) / size[c["rows"]]
    gw = rng.uniform(-1.0, 1.0, (len(ne), 6)) / size[:, None]
    return g, gw


def _rows(grad: np.ndarray) -> np.ndarray:
    return np.linalg.norm(grad, axis=1) if len(grad) else np.zeros(0)


# ---- the checks --------------------------------------------------------------------------------------------------------

def check_constant_wall_upstream(c: dict, out: dict, run, exact: bool) -> float:
    """Check 1: sum_a wall_area[a,w] is the wall's rectangle, so a grad_wall_area that is constant down each column (and
    no grad_face_area) has the gradient 0: exactly (``exact``), or at most 1e-9 of the row scale of the unit-upstream
    gradient where walls of area exactly 0, whose upstream is masked, can sit next to an edge."""
    n = len(c["points"])
    grad = run(c, out, None, np.tile(WALL_COLUMNS, (n, 1)))
    assert grad.shape == (n, 3) and grad.dtype == np.float64 and np.isfinite(grad).all()
    if exact:
        assert (grad == 0.0).all(), f"{c.get('name', '')}: max |grad| = {np.abs(grad).max():.3g}"
        return 0.0
    unit = run(c, out, *unit_upstreams(c, out))
    ratio = float((_rows(grad) / np.maximum(_rows(unit), 1.0)).max())
    print(f"{c.get('name', '')}: constant wall upstream: |grad| / row scale = {ratio:.3g} (bar {ROW_BAR:.3g})")
    assert ratio <= ROW_BAR
    return ratio


def closure_upstreams(c: dict, out: dict, seed: int = 7):
    """For per-cell u_a (zero on the empty cells) the upstreams of  sum_a u_a . (sum_b A_ab d^_ab + sum_w A_aw n_w)  with
    d^ held fixed, and the gradient of the same sum with the areas held fixed (through d^ alone), in numpy."""
    c = with_rows(c)
    rng = np.random.default_rng(seed)
    p = c["points"].astype(np.float64)
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    u = np.where(out["nonempty"][:, None], rng.uniform(-1.0, 1.0, (len(p), 3)), 0.0)
    d = p[adj] - p[rows]
    length = np.linalg.norm(d, axis=1)
    unit = d / length[:, None]
    g = (u[rows] * unit).sum(1)
    gw = u @ NORMALS.T
    t = (u[rows] - g[:, None] * unit) / length[:, None] * out["face_area"][:, None]
    direct = np.zeros_like(p)
    np.add.at(direct, adj, t)
    np.add.at(direct, rows, -t)
    return u, g, gw, direct


def check_closure(c: dict, out: dict, run) -> float:
    """Check 2 through the operator: the area vectors of every non-empty cell close, so the sum above is identically 0 in
    the points and its gradient -- the operator's half plus the half through d^ -- vanishes: sum_a |p_a| |grad_a| <= 1e-9
    sum_a |p_a| |term_a|, term_a the operator's half alone (both sides weighed alike, the unit of
    clip_area_grad_host.check_identities).  Returns the ratio."""
    p = c["points"].astype(np.float64)
    _, g, gw, direct = closure_upstreams(c, out)
    term = run(c, out, g, gw)
    assert np.isfinite(term).all()
    size = np.linalg.norm(p, axis=1)
    top, scale = (size * _rows(term + direct)).sum(), (size * _rows(term)).sum()
    assert scale > 0.0
    print(f"{c.get('name', '')}: closure: sum |p||grad| = {top:.3g} of sum |p||term| = {scale:.4g}: {top / scale:.3g} "
          f"(bar {CLOSURE_BAR:.3g})")
    assert top <= CLOSURE_BAR * scale
    return top / scale


def check_agreement(c: dict, out: dict, geo: dict, run, plain_grad) -> float:
    """Check 3: with upstreams only on slots both of whose cells cell_geometry calls bounded and whose wall_area rows are
    all zero, the rows equal face_area_grad's to 2e-9 of the O(1) row scale; at least a quarter of the cells qualify.
    ``plain_grad(g) -> grad`` is face_area_grad on the same cloud with ``geo`` (cell_geometry's answer)."""
    c = with_rows(c)
    free = geo["bounded"] & (out["wall_area"] == 0.0).all(1) & out["nonempty"]
    print(f"{c.get('name', '')}: {free.sum()} of {free.size} cells are bounded and touch no wall")
    assert free.sum() >= 0.25 * free.size
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    g = np.where(free[rows] & free[adj], unit_upstreams(c, out, seed=5)[0], 0.0)
    got, want = run(c, out, g, None), plain_grad(g)
    assert np.isfinite(got).all() and np.isfinite(want).all() and _rows(want).max() > 0.1
    ratio = float((_rows(got - want) / np.maximum(_rows(want), 1.0)).max())
    print(f"    worst |grad - face_area_grad| / row scale = {ratio:.3g} (bar {AGREEMENT_BAR:.3g})")
    assert ratio <= AGREEMENT_BAR
    return ratio


def check_empty_cells_are_ignored(c: dict, out: dict, run, least: int = 1):
    """Check 4: NaN and inf upstreams on every slot and wall of the empty cells give the bits that zeros there give;
    everything is finite"""
    c = with_rows(c)
    ne = out["nonempty"]
    assert (~ne).sum() >= least
    assert (out["face_area"][~ne[c["rows"]]] == 0.0).all() and (out["wall_area"][~ne] == 0.0).all()
    g, gw = unit_upstreams(c, out)
    clean = run(c, out, np.where(ne[c["rows"]], g, 0.0), np.where(ne[:, None], gw, 0.0))
    assert np.isfinite(clean).all()
    if ne.any():
        assert np.abs(clean).max() > 0.0
    for bad in (np.nan, np.inf, -np.inf):
        got = run(c, out, np.where(ne[c["rows"]], g, bad), np.where(ne[:, None], gw, bad))
        assert np.array_equal(got, clean)
    assert (clean[~ne] == 0.0).all()


def check_none_and_additivity(c: dict, out: dict, run) -> float:
    """Check 5: None is an all-zero upstream bit for bit, and grad(g, gw) = grad(g, None) + grad(None, gw) per row to 1e-9
    of the row scale (the rows' own size, at least 1)"""
    n, e = len(c["points"]), len(c["adjacency"])
    g, gw = unit_upstreams(c, out, seed=3)
    both, of_g, of_w = run(c, out, g, gw), run(c, out, g, None), run(c, out, None, gw)
    assert np.array_equal(of_g, run(c, out, g, np.zeros((n, 6))))
    assert np.array_equal(of_w, run(c, out, np.zeros(e), gw))
    assert (run(c, out, None, None) == 0.0).all()
    assert np.isfinite(both).all()
    scale = np.maximum(_rows(of_g) + _rows(of_w), 1.0)
    ratio = float((_rows(both - (of_g + of_w)) / scale).max()) if n else 0.0
    print(f"{c.get('name', '')}: |grad(g, gw) - grad(g, None) - grad(None, gw)| / row scale = {ratio:.3g}")
    assert ratio <= ROW_BAR
    return ratio


def check_rows_agree(name: str, got: np.ndarray, want: np.ndarray) -> float:
    """Check 6: two gradients of unit upstreams agree per row to 1e-9 of max(1, |row|)"""
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    ratio = float((_rows(got - want) / np.maximum(_rows(want), 1.0)).max()) if len(got) else 0.0
    print(f"{name}: worst |device row - host row| / row scale = {ratio:.3g} (bar {ROW_BAR:.3g})")
    assert ratio <= ROW_BAR
    return ratio


def tiny_cases() -> dict:
    from tests.host_harness import clip_box_grad_host as BG

    return {k: with_rows(v) for k, v in BG.tiny_cases().items()}


def check_tiny(c: dict, out: dict, run):
    """Check 7 on n1, n2 (empty rows: a zero row) and n4: finite, and checks 1 and 2"""
    n = len(c["points"])
    grad = run(c, out, *unit_upstreams(c, out, seed=2))
    assert grad.shape == (n, 3) and np.isfinite(grad).all()
    empty_rows = np.diff(np.asarray(c["offsets"]).astype(np.int64)) == 0
    assert (grad[empty_rows] == 0.0).all()
    check_constant_wall_upstream(c, out, run, exact=True)
    if not empty_rows.all():
        check_closure(c, out, run)


def check_labels(c: dict, out: dict, cells) -> int:
    """Check 10, on the host build's polygons of the row faces of ``cells``: the labelled clipping gives the unlabelled
    vertices bit for bit, and every labelled edge of nonzero length of a face of positive area lies on its label's plane
    (a bisector or a wall) at both end points, to 1e-10 of the face's size (its largest distance between two vertices).
    Returns the number of (Voronoi, wall) edges seen."""
    p = c["points"].astype(np.float64)
    off, adj = np.asarray(c["offsets"]).astype(np.int64), np.asarray(c["adjacency"]).astype(np.int64)
    box = np.asarray(c["box"], dtype=np.float64)
    seen = [0, 0]
    for a in cells:
        degree = int(off[a + 1] - off[a])
        h_wall = np.array([p[a, 0] - box[0], box[3] - p[a, 0], p[a, 1] - box[1], box[4] - p[a, 1], p[a, 2] - box[2],
                           box[5] - p[a, 2]])
        for i in range(degree):
            got = labelled_polygon(c, int(a), i)
            assert got is not None
            xyz, label, same = got
            assert same
            if not out["face_area"][off[a] + i] > 0.0:
                continue
            m = len(xyz)
            assert m >= 3 and (label != NO_LABEL).all() and (label < degree + 6).all() and (label != i).all()
            size = max(np.linalg.norm(xyz[:, None] - xyz[None], axis=2).max(), 1e-300)
            for v in range(m):
                ends = xyz[[v, (v + 1) % m]]
                if (ends[0] == ends[1]).all():
                    continue
                l = int(label[v])
                if l < degree:
                    d = p[adj[off[a] + l]] - p[a]
                    dist = np.abs(ends @ d - 0.5 * d @ d) / np.linalg.norm(d)
                else:
                    dist = np.abs(ends @ NORMALS[l - degree] - h_wall[l - degree])
                assert (dist <= LABEL_BAR * size).all(), (a, i, v, l, dist, size)
                seen[l >= degree] += 1
    return tuple(seen)
