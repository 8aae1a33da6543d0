"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_box_grad.hpp (test harness; see clip_box_grad_host.cpp), and
the checks the CPU and GPU tests of radfoam.cell_geometry_in_box_grad share.  A check takes a case ``c`` (points,
adjacency, offsets, box), the forward's answer ``out`` for it (volume, centroid, nonempty as numpy) and ``run``, a
callable ``run(c, out, grad_volume, grad_centroid) -> grad f64[N,3]`` (numpy; either upstream may be None), and does not
care where ``run`` computes."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_box_grad_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_box_grad_host.cpp")] + [os.path.join(_CSRC, n) for n in (
    "rf_clip_box_grad.hpp", "rf_clip_box.hpp", "rf_clip_grad.hpp", "rf_clip.hpp")]

ROW_BAR = 1e-9          # per row, with the O(1) rows of unit upstreams: the bar of the cell-geometry gradients
MOMENT_BAR = 1e-9       # the first-moment partition: max |grad| against max |grad of the grad_centroid half alone|
AGREEMENT_BAR = 2e-9    # against cell_geometry_grad away from the walls: the forward's agreement bar


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
        _lib.clip_box_grad_host_cell_box_grad.restype = C.c_int
        _lib.clip_box_grad_host_cell_box_grad.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                          C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
    return _lib


def _f64(x, shape):
    if x is None:
        return None
    out = np.ascontiguousarray(x, dtype=np.float64)
    assert out.shape == shape
    return out


def cell_box_grad(points, adjacency, offsets, box, geo: dict, grad_volume, grad_centroid, cap: int = 256) -> dict:
    """The host build of the serial row over every cell: grad f64[N,3], status u32[N] (0 ok, 1 a face outgrew ``cap``
    vertices, 2 bad row) and ``bad``.  ``geo`` is what clip_box_host.cell_box returned for the same cloud and box; either
    upstream may be None."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    six = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
    assert six.shape == (6,)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    vol, cen = _f64(geo["volume"], (n,)), _f64(geo["centroid"], (n, 3))
    ne = np.ascontiguousarray(geo["nonempty"], dtype=np.uint8)
    gv, gc = _f64(grad_volume, (n,)), _f64(grad_centroid, (n, 3))
    grad, status = np.empty((n, 3)), np.empty(n, dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data
    bad = lib().clip_box_grad_host_cell_box_grad(ptr(pts), n, ptr(adj), ptr(off), e, ptr(bbox), ptr(six), cap, ptr(vol),
                                                 ptr(cen), ptr(ne), ptr(gv), ptr(gc), ptr(grad), ptr(status))
    return dict(grad=grad, status=status, bad=bad)


def host_run(c: dict, out: dict, grad_volume, grad_centroid) -> np.ndarray:
    got = cell_box_grad(c["points"], c["adjacency"], c["offsets"], c["box"], out, grad_volume, grad_centroid)
    assert got["bad"] == 0
    return got["grad"]


def write_arrays(name: str, path: str):
    """a case (of tests/cell_box_grad_ref.FD_CASES, else of clip_box_host.CASES) as the plain arrays
    tests/host_harness/clip_box_grad_sanitize.cpp reads"""
    from tests import cell_box_grad_ref as R

    c = R.recorded_case(name) if name in R.FD_CASES else B.case(name)
    pts = np.ascontiguousarray(c["points"], dtype=np.float32)
    adj, off = c["adjacency"].astype(np.uint32), c["offsets"].astype(np.uint32)
    with open(path, "wb") as f:
        for part in (np.array([len(pts), len(adj)], dtype=np.uint32), pts, adj, off, H.bbox_of(pts), c["box"]):
            f.write(np.ascontiguousarray(part).tobytes())


_FORWARD = {}


def host_forward(key, c: dict) -> dict:
    """clip_box_host.cell_box of a case, once"""
    if key not in _FORWARD:
        _FORWARD[key] = B.cell_box(c["points"], c["adjacency"], c["offsets"], c["box"])
        assert _FORWARD[key]["bad"] == 0
    return _FORWARD[key]


def unit_upstreams(out: dict, seed: int = 0, cells=None):
    """Unit upstreams per cell in units of the cell's own size s_a = V_a^(1/3): gV_a = r_a / s_a^2 and gC_a = r'_a with
    r, r' uniform in [-1,1], so that a cell's own terms of its row are O(1).  On the empty cells they are NaN: nothing
    may read them.  ``cells``: zero on the non-empty cells outside it."""
    rng = np.random.default_rng(seed)
    ne = out["nonempty"]
    n = len(ne)
    size = np.cbrt(np.where(ne, out["volume"], 1.0))
    gv = np.where(ne, rng.uniform(-1.0, 1.0, n) / size ** 2, np.nan)
    gc = np.where(ne[:, None], rng.uniform(-1.0, 1.0, (n, 3)), np.nan)
    if cells is not None:
        off = ne & ~np.asarray(cells, dtype=bool)
        gv[off], gc[off] = 0.0, 0.0
    return gv, gc


def _rows(grad: np.ndarray) -> np.ndarray:
    return np.linalg.norm(grad, axis=1) if len(grad) else np.zeros(0)


# ---- the checks --------------------------------------------------------------------------------------------------------

def check_partition_volume(c: dict, out: dict, run):
    """Check 1: sum V = V_box for any sites, so a constant grad_volume without grad_centroid has the gradient exactly 0"""
    n = len(c["points"])
    grad = run(c, out, np.full(n, 0.75), None)
    assert grad.shape == (n, 3) and grad.dtype == np.float64
    assert (grad == 0.0).all(), f"{c.get('name', '')}: max |grad| = {np.abs(grad).max():.3g}"


def check_partition_moment(c: dict, out: dict, run) -> float:
    """Check 2: sum V c = V_box centre, so grad_volume[a] = e . c_a, grad_centroid[a] = V_a e makes phi_a(x) = e . x on
    every non-empty cell and the gradient vanishes: max_a |grad p_a| <= 1e-9 max_a |grad' p_a|, grad' the gradient of
    the grad_centroid half alone.  grad_volume is NaN on the empty cells, as e . c_a is.  Returns the worst ratio."""
    worst = 0.0
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        gv, gc = out["centroid"] @ e, out["volume"][:, None] * e
        assert np.isnan(gv[~out["nonempty"]]).all() and np.isfinite(gc).all()
        full, half = run(c, out, gv, gc), run(c, out, None, gc)
        assert np.isfinite(full).all() and np.isfinite(half).all()
        top, unit = _rows(full).max(), _rows(half).max()
        assert unit > 0.0
        print(f"{c.get('name', '')}: e_{k}: max |grad| = {top:.3g}, of the grad_centroid half alone {unit:.3g}, ratio "
              f"{top / unit:.3g} (bar {MOMENT_BAR:.3g})")
        assert top <= MOMENT_BAR * unit
        worst = max(worst, top / unit)
    return worst


def check_empty_cells_are_ignored(c: dict, out: dict, run, least: int = 1):
    """Check 3: NaN and inf upstreams on the empty cells give the bits that zeros there give; everything is finite"""
    ne = out["nonempty"]
    assert (~ne).sum() >= least
    gv, gc = unit_upstreams(out)                    # NaN on the empty cells
    clean = run(c, out, np.where(ne, gv, 0.0), np.where(ne[:, None], gc, 0.0))
    assert np.isfinite(clean).all() and np.abs(clean).max() > 0.0
    for bad in (np.nan, np.inf, -np.inf):
        got = run(c, out, np.where(ne, gv, bad), np.where(ne[:, None], gc, bad))
        assert np.array_equal(got, clean)


def check_none_and_linearity(c: dict, out: dict, run):
    """Check 4: None is an all-zero upstream bit for bit, and grad(gV, gC) = grad(gV, None) + grad(None, gC) per row to
    1e-9 of the row scale (the rows' own size, at least 1: unit upstreams give O(1) rows)"""
    n = len(c["points"])
    gv, gc = unit_upstreams(out, seed=3)
    both, of_v, of_c = run(c, out, gv, gc), run(c, out, gv, None), run(c, out, None, gc)
    assert np.array_equal(of_v, run(c, out, gv, np.zeros((n, 3))))
    assert np.array_equal(of_c, run(c, out, np.zeros(n), gc))
    assert (run(c, out, None, None) == 0.0).all()
    assert np.isfinite(both).all()
    scale = np.maximum(_rows(of_v) + _rows(of_c), 1.0)
    ratio = float((_rows(both - (of_v + of_c)) / scale).max()) if n else 0.0
    print(f"{c.get('name', '')}: |grad(gV, gC) - grad(gV, None) - grad(None, gC)| / row scale = {ratio:.3g}")
    assert ratio <= ROW_BAR


def check_agreement(c: dict, out: dict, wall_area: np.ndarray, bounded: np.ndarray, run, plain_grad) -> float:
    """Check 5: with upstreams that are non-zero only on cells cell_geometry calls bounded and whose wall_area is all
    zero, the gradient equals cell_geometry_grad's per row to 2e-9 times the O(1) row scale; at least a quarter of the
    cells are such cells.  ``plain_grad(gv, gc) -> grad`` is cell_geometry_grad on the same cloud (its upstreams are zero
    on every other cell too).  Returns the worst ratio."""
    free = bounded & (wall_area == 0.0).all(1) & out["nonempty"]
    print(f"{c.get('name', '')}: {free.sum()} of {free.size} cells are bounded and touch no wall")
    assert free.sum() >= 0.25 * free.size
    gv, gc = unit_upstreams(out, seed=5, cells=free)
    gv, gc = np.where(out["nonempty"], gv, 0.0), np.where(out["nonempty"][:, None], gc, 0.0)
    got, want = run(c, out, gv, gc), plain_grad(gv, gc)
    assert np.isfinite(got).all() and np.isfinite(want).all() and _rows(want).max() > 0.1
    ratio = float((_rows(got - want) / np.maximum(_rows(want), 1.0)).max())
    print(f"    worst |grad - cell_geometry_grad| / row scale = {ratio:.3g} (bar {AGREEMENT_BAR:.3g})")
    assert ratio <= AGREEMENT_BAR
    return ratio


def check_rows_agree(name: str, got: np.ndarray, want: np.ndarray) -> float:
    """Check 6: two gradients of unit upstreams agree per row to 1e-9 (O(1) rows)"""
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    ratio = float((_rows(got - want) / np.maximum(_rows(want), 1.0)).max()) if len(got) else 0.0
    print(f"{name}: worst |device row - host row| / row scale = {ratio:.3g} (bar {ROW_BAR:.3g})")
    assert ratio <= ROW_BAR
    return ratio


def tiny_cases() -> dict:
    """name -> case dict of clip_host.tiny_inputs() n1, n2, n4 in one box"""
    tiny = H.tiny_inputs()
    box = np.array([-1.0, -2.0, -0.5, 2.0, 1.0, 3.5])
    out = {}
    for name in ("n1", "n2", "n4"):
        pts, off, adj = tiny[name]
        out[name] = dict(points=pts, offsets=off, adjacency=adj, box=box, name=name)
    return out


def check_tiny(c: dict, out: dict, run):
    """Check 8 on n1, n2 (empty rows: the whole box, a zero row) and n4: finite, and checks 1 and 2"""
    n = len(c["points"])
    gv, gc = unit_upstreams(out, seed=2)
    grad = run(c, out, gv, gc)
    assert grad.shape == (n, 3) and np.isfinite(grad).all()
    empty_rows = np.diff(np.asarray(c["offsets"]).astype(np.int64)) == 0
    assert (grad[empty_rows] == 0.0).all()
    check_partition_volume(c, out, run)
    if not empty_rows.all():
        check_partition_moment(c, out, run)
    else:       # nothing moves anything: both halves are exactly zero
        assert (run(c, out, out["centroid"][:, 0], out["volume"][:, None] * np.array([1.0, 0.0, 0.0])) == 0.0).all()
