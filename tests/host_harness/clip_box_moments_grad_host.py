"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_box_moments_grad.hpp (test harness; see
clip_box_moments_grad_host.cpp), and the checks the CPU and GPU tests of radfoam.cell_moments_in_box_grad share.  A check
takes a case ``c`` (points, adjacency, offsets, box), the forward's answer ``out`` for it (volume, centroid, nonempty as
numpy) and ``run``, a callable ``run(c, out, grad_site_moment, grad_central_moment, grad_volume, grad_centroid) -> grad
f64[N,3]`` (numpy; any upstream may be None), and does not care where ``run`` computes."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_box_grad_host as BG
from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_box_moments_grad_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_box_moments_grad_host.cpp")] + [os.path.join(_CSRC, n) for n in (
    "rf_clip_box_moments_grad.hpp", "rf_clip_box.hpp", "rf_clip_grad.hpp", "rf_clip_moments_grad.hpp",
    "rf_clip_moments.hpp", "rf_clip.hpp")]

ROW_BAR = 1e-9          # per row, of the row scale: the bar of the closed forms and identities
AGREEMENT_BAR = 2e-9    # against cell_moments_grad away from the walls: the forward's agreement bar
PLAIN_CASES = ("uniform400", "tight", "wide", "disjoint", "offset")
TRACE = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
# three fixed symmetric G as six numbers (xx, yy, zz, xy, xz, yz: S(g) halves the last three), one with off-diagonals
PARTITION_G = (np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]), np.array([2.0, -0.5, 0.75, 0.0, 0.0, 0.0]),
               np.array([0.5, 1.5, -1.0, 0.8, -0.6, 1.2]))


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
        fn = _lib.clip_box_moments_grad_host_cell_box_moments_grad
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                       C.c_uint32] + [C.c_void_p] * 9
    return _lib


def cell_box_moments_grad(points, adjacency, offsets, box, geo: dict, grad_site_moment, grad_central_moment,
                          grad_volume, grad_centroid, cap: int = 256) -> dict:
    """The host build of the serial row over every cell: grad f64[N,3], status u32[N] (0 ok, 1 a face outgrew ``cap``
    vertices, 2 bad row) and ``bad``.  ``geo`` is what clip_box_host.cell_box returned for the same cloud and box; any
    upstream may be None."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    six = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
    assert six.shape == (6,)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    vol, cen = BG._f64(geo["volume"], (n,)), BG._f64(geo["centroid"], (n, 3))
    ne = np.ascontiguousarray(geo["nonempty"], dtype=np.uint8)
    gq, gm = BG._f64(grad_site_moment, (n, 6)), BG._f64(grad_central_moment, (n, 6))
    gv, gc = BG._f64(grad_volume, (n,)), BG._f64(grad_centroid, (n, 3))
    grad, status = np.empty((n, 3)), np.empty(n, dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data
    bad = lib().clip_box_moments_grad_host_cell_box_moments_grad(
        ptr(pts), n, ptr(adj), ptr(off), e, ptr(bbox), ptr(six), cap, ptr(vol), ptr(cen), ptr(ne), ptr(gq), ptr(gm),
        ptr(gv), ptr(gc), ptr(grad), ptr(status))
    return dict(grad=grad, status=status, bad=bad)


def host_run(c: dict, out: dict, gq, gm, gv, gc) -> np.ndarray:
    got = cell_box_moments_grad(c["points"], c["adjacency"], c["offsets"], c["box"], out, gq, gm, gv, gc)
    assert got["bad"] == 0
    return got["grad"]


def host_geometry_run(c: dict, out: dict, gv, gc) -> np.ndarray:
    """cell_box_grad_serial on the same case: the volume / centroid half alone"""
    return BG.host_run(c, out, gv, gc)


host_forward = BG.host_forward
write_arrays = BG.write_arrays


def unit_upstreams(out: dict, seed: int = 0, cells=None):
    """(gQ, gC, gV, gc): unit upstreams per cell in units of the cell's own size s_a = V_a^(1/3): r / s^4 for the two
    moments [N,6], r / s^2 for the volume [N] and r for the centroid [N,3], r uniform in [-1,1], so that a cell's own
    terms of its row are O(1).  On the empty cells they are NaN: nothing may read them.  ``cells``: zero on the non-empty
    cells outside it."""
    rng = np.random.default_rng(seed)
    ne = out["nonempty"].astype(bool)
    n = len(ne)
    size = np.cbrt(np.where(ne, out["volume"], 1.0))
    gq = np.where(ne[:, None], rng.uniform(-1.0, 1.0, (n, 6)) / size[:, None] ** 4, np.nan)
    gm = np.where(ne[:, None], rng.uniform(-1.0, 1.0, (n, 6)) / size[:, None] ** 4, np.nan)
    gv = np.where(ne, rng.uniform(-1.0, 1.0, n) / size ** 2, np.nan)
    gc = np.where(ne[:, None], rng.uniform(-1.0, 1.0, (n, 3)), np.nan)
    if cells is not None:
        off = ne & ~np.asarray(cells, dtype=bool)
        gq[off], gm[off], gv[off], gc[off] = 0.0, 0.0, 0.0, 0.0
    return gq, gm, gv, gc


def symmetric(g6) -> np.ndarray:
    """S(g): six numbers -> [...,3,3], the diagonal as it is and half of each off-diagonal number on both sides"""
    xx, yy, zz, xy, xz, yz = np.moveaxis(np.asarray(g6, dtype=np.float64), -1, 0)
    xy, xz, yz = 0.5 * xy, 0.5 * xz, 0.5 * yz
    return np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)


def _rows(grad: np.ndarray) -> np.ndarray:
    return np.linalg.norm(grad, axis=1) if len(grad) else np.zeros(0)


def _geometry(c: dict, out: dict):
    """(p f64[N,3], nonempty bool[N], V, m = c - p with zeros on the empty cells)"""
    p, ne = c["points"].astype(np.float64), out["nonempty"].astype(bool)
    m = np.where(ne[:, None], out["centroid"] - p, 0.0)
    return p, ne, np.where(ne, out["volume"], 0.0), m


# ---- the checks --------------------------------------------------------------------------------------------------------

def check_cvt(c: dict, out: dict, run, finite_only: bool = False) -> float:
    """Check (a): with grad_site_moment = (1,1,1,0,0,0) on every cell and nothing else, Psi = |x - p|^2 on both sides of a
    face between non-empty cells, which vanishes on the bisector: grad p_a = 2 V_a (p_a - c_a) on EVERY non-empty cell,
    hull cells, empty rows and sites outside the box included, and exactly zero rows on the empty cells.  Per row to 1e-9 of
    the row scale V_a max(longest |d_b| of the row, |c_a - p_a|): the size of the terms the row is made of.  Returns the
    worst ratio."""
    n = len(c["points"])
    p, ne, vol, m = _geometry(c, out)
    grad = run(c, out, np.tile(TRACE, (n, 1)), None, None, None)
    assert grad.shape == (n, 3) and grad.dtype == np.float64 and np.isfinite(grad).all()
    if finite_only:
        return 0.0
    assert (grad[~ne] == 0.0).all()
    off, adj = np.asarray(c["offsets"]).astype(np.int64), np.asarray(c["adjacency"]).astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(off))
    longest = np.zeros(n)
    np.maximum.at(longest, rows, np.linalg.norm(p[adj] - p[rows], axis=1))
    scale = vol * np.maximum(longest, np.linalg.norm(m, axis=1))
    want = -2.0 * vol[:, None] * m
    ratio = float((_rows(grad - want)[ne] / scale[ne]).max()) if ne.any() else 0.0
    print(f"{c.get('name', '')}: CVT gradient on {ne.sum()} non-empty cells, {(~ne).sum()} empty rows exactly zero: worst "
          f"|grad - 2 V (p - c)| / row scale = {ratio:.3g} (bar {ROW_BAR:.3g})")
    assert ratio <= ROW_BAR
    return ratio


def check_partition(c: dict, out: dict, run) -> float:
    """Check (b) without autograd.  sum_a <G, Q_a> + 2 V_a q_a^T G m_a + V_a q_a^T G q_a = <G, V_box diag(e^2 / 12)> with
    q_a = p_a - centre and m_a = c_a - p_a, for any sites.  As a function of (Q, V, c, p) its upstreams are G for the site
    moment, q^T G q + 2 q^T G m for the volume and 2 V G q for the centroid (NaN on the empty cells, passed as they are)
    in ONE call, and what is left of the explicit dependence on p is 2 V_a G m_a.  The sum must vanish: max_a |row| <= 1e-9
    sum_a |row of the moment half alone|.  Returns the worst ratio over PARTITION_G."""
    n = len(c["points"])
    p, ne, vol, m = _geometry(c, out)
    box = np.asarray(c["box"], dtype=np.float64)
    q = p - 0.5 * (box[:3] + box[3:])
    worst = 0.0
    for g6 in PARTITION_G:
        G = symmetric(g6)
        mm = out["centroid"] - p                                   # NaN on the empty cells
        gv = np.einsum("ni,ij,nj->n", q, G, q) + 2.0 * np.einsum("ni,ij,nj->n", q, G, mm)
        gc = 2.0 * out["volume"][:, None] * (q @ G)
        gq = np.tile(g6, (n, 1))
        fused = run(c, out, gq, None, gv, gc)
        half = run(c, out, gq, None, None, None)
        total = fused + 2.0 * vol[:, None] * (m @ G)
        assert np.isfinite(total).all() and np.isfinite(half).all()
        unit = _rows(half).sum()
        assert unit > 0.0
        ratio = float(_rows(total).max() / unit)
        print(f"{c.get('name', '')}: G = {g6.tolist()}: max |grad| = {_rows(total).max():.3g}, sum |rows of the moment "
              f"half| = {unit:.3g}, ratio {ratio:.3g} (bar {ROW_BAR:.3g})")
        assert ratio <= ROW_BAR
        worst = max(worst, ratio)
    return worst


def check_central_path(c: dict, out: dict, run, seed: int = 7) -> float:
    """Check (c) without autograd: C_a = Q_a - V_a m_a m_a^T, so the gradient of sum <H_a, C_a> equals that of
    sum <H_a, Q_a> - V_a m_a^T H_a m_a: upstreams H for the site moment, -m^T H m for the volume, -2 V H m for the
    centroid, plus the explicit 2 V_a H_a m_a.  Random H = r / s^4; per row to 1e-9 of max(1, |row|)."""
    n = len(c["points"])
    p, ne, vol, m = _geometry(c, out)
    h6 = unit_upstreams(out, seed=seed)[1]
    Hm = np.einsum("nij,nj->ni", symmetric(np.where(ne[:, None], h6, 0.0)), m)
    direct = run(c, out, None, h6, None, None)
    gv = np.where(ne, -(m * Hm).sum(1), np.nan)
    gc = np.where(ne[:, None], -2.0 * vol[:, None] * Hm, np.nan)
    other = run(c, out, h6, None, gv, gc) + 2.0 * vol[:, None] * Hm
    assert np.isfinite(direct).all() and np.isfinite(other).all() and np.abs(direct).max() > 0.0
    ratio = float((_rows(direct - other) / np.maximum(_rows(direct), 1.0)).max())
    print(f"{c.get('name', '')}: central path: worst |grad <H,C> - grad (<H,Q> - V m^T H m)| / row scale = {ratio:.3g} "
          f"(bar {ROW_BAR:.3g})")
    assert ratio <= ROW_BAR
    return ratio


def check_fusion(c: dict, out: dict, run, geometry_run) -> tuple:
    """Check (d): with the moment upstreams None the rows agree with the volume / centroid operator's
    (``geometry_run(c, out, gv, gc)``) to 1e-9; all four upstreams against the sum of the two halves to 1e-9; None equals
    an all-zero upstream bit for bit.  Row scale max(1, |row|): unit upstreams give O(1) rows."""
    n = len(c["points"])
    gq, gm, gv, gc = unit_upstreams(out, seed=3)
    geo_half, want = run(c, out, None, None, gv, gc), geometry_run(c, out, gv, gc)
    assert np.isfinite(geo_half).all() and np.isfinite(want).all()
    r1 = float((_rows(geo_half - want) / np.maximum(_rows(want), 1.0)).max()) if n else 0.0
    mom_half, both = run(c, out, gq, gm, None, None), run(c, out, gq, gm, gv, gc)
    assert np.isfinite(both).all() and np.isfinite(mom_half).all()
    scale = np.maximum(_rows(mom_half) + _rows(geo_half), 1.0)
    r2 = float((_rows(both - (mom_half + geo_half)) / scale).max()) if n else 0.0
    print(f"{c.get('name', '')}: fusion: against the volume / centroid operator {r1:.3g}, all four against the two halves "
          f"{r2:.3g} (bar {ROW_BAR:.3g})")
    assert r1 <= ROW_BAR and r2 <= ROW_BAR
    z6, z1, z3 = np.zeros((n, 6)), np.zeros(n), np.zeros((n, 3))
    assert np.array_equal(mom_half, run(c, out, gq, gm, z1, z3))
    assert np.array_equal(geo_half, run(c, out, z6, z6, gv, gc))
    assert np.array_equal(run(c, out, gq, None, None, gc), run(c, out, gq, z6, z1, gc))
    assert (run(c, out, None, None, None, None) == 0.0).all()
    return r1, r2


def check_agreement(c: dict, out: dict, bounded: np.ndarray, run, plain_grad) -> float:
    """Check (e): with moment upstreams that are non-zero only on cells cell_geometry calls bounded and whose wall_area is
    all zero, the rows agree with cell_moments_grad's (``plain_grad(gq, gm) -> grad`` on the same cloud) to 2e-9 of
    max(1, |row|); at least a quarter of the cells are such cells.  Returns the worst ratio."""
    ne = out["nonempty"].astype(bool)
    free = np.asarray(bounded, dtype=bool) & (out["wall_area"] == 0.0).all(1) & ne
    print(f"{c.get('name', '')}: {free.sum()} of {free.size} cells are bounded and touch no wall")
    assert free.sum() >= 0.25 * free.size
    gq, gm, _, _ = unit_upstreams(out, seed=5, cells=free)
    gq, gm = np.where(ne[:, None], gq, 0.0), np.where(ne[:, None], gm, 0.0)
    got, want = run(c, out, gq, gm, None, None), plain_grad(gq, gm)
    assert np.isfinite(got).all() and np.isfinite(want).all() and _rows(want).max() > 0.1
    ratio = float((_rows(got - want) / np.maximum(_rows(want), 1.0)).max())
    print(f"    worst |grad - cell_moments_grad| / row scale = {ratio:.3g} (bar {AGREEMENT_BAR:.3g})")
    assert ratio <= AGREEMENT_BAR
    return ratio


def check_empty_cells_are_ignored(c: dict, out: dict, run, least: int = 1):
    """Check (f): NaN and inf in all four upstreams on the empty cells give the bits that zeros there give; everything is
    finite"""
    ne = out["nonempty"].astype(bool)
    assert (~ne).sum() >= least
    ups = unit_upstreams(out)                    # NaN on the empty cells
    fill = lambda bad: [np.where(ne.reshape((-1,) + (1,) * (u.ndim - 1)), u, bad) for u in ups]
    clean = run(c, out, *fill(0.0))
    assert np.isfinite(clean).all() and np.abs(clean).max() > 0.0 and (clean[~ne] == 0.0).all()
    for bad in (np.nan, np.inf, -np.inf):
        assert np.array_equal(run(c, out, *fill(bad)), clean)


def check_rows_agree(name: str, got: np.ndarray, want: np.ndarray) -> float:
    """Check (g): two gradients agree per row to 1e-9 of max(1, max |host row|)"""
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    ratio = float((np.abs(got - want).max(1) / np.maximum(1.0, np.abs(want).max(1))).max()) if len(got) else 0.0
    print(f"{name}: worst |device row - host row| / row scale = {ratio:.3g} (bar {ROW_BAR:.3g})")
    assert ratio <= ROW_BAR
    return ratio


tiny_cases = BG.tiny_cases


def check_tiny(c: dict, out: dict, run):
    """Check (i) on n1, n2 (empty rows) and n4.  An empty row is the whole box: with a site-moment upstream the row is
    the direct term -2 V_box G (centre - p) to 1e-12 of its size, and zero without one; n4 is finite and satisfies (a)."""
    n = len(c["points"])
    p = c["points"].astype(np.float64)
    box = np.asarray(c["box"], dtype=np.float64)
    gq, gm, gv, gc = unit_upstreams(out, seed=2)
    grad = run(c, out, gq, gm, gv, gc)
    assert grad.shape == (n, 3) and np.isfinite(grad).all()
    empty_rows = np.diff(np.asarray(c["offsets"]).astype(np.int64)) == 0
    if empty_rows.any():
        assert out["nonempty"][empty_rows].all()
        want = -2.0 * (box[3:] - box[:3]).prod() * np.einsum("nij,nj->ni", symmetric(gq), 0.5 * (box[:3] + box[3:]) - p)
        size = np.abs(want[empty_rows]).max()
        assert size > 0.0 and np.abs(grad - want)[empty_rows].max() <= 1e-12 * size
        assert (run(c, out, None, gm, gv, gc)[empty_rows] == 0.0).all()
    check_cvt(c, out, run)
