"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_box_moments.hpp (test harness; see
clip_box_moments_host.cpp), and the checks the CPU and GPU tests of radfoam.cell_moments_in_box share.  The cases, the
clouds and the cells the exact reference works on are those of tests/host_harness/clip_box_host.  Every check takes the
boxed geometry (``geo``: at least volume, centroid, nonempty, wall_area) and the twelve moments (``site``, ``central``)
as numpy arrays and does not care where they were computed."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H
from tests.host_harness import clip_moments_host as M

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_box_moments_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_box_moments_host.cpp")] + [
    os.path.join(_CSRC, n) for n in ("rf_clip_box_moments.hpp", "rf_clip_box.hpp", "rf_clip_moments.hpp",
                                     "rf_clip_grad.hpp", "rf_clip.hpp")]

BAR = M.BAR      # |delta| <= BAR tr Q_exact[a] on each of the twelve numbers of cell a: the bar of the cell moments
EXACT_CASES = ("uniform400", "tight", "wide", "disjoint", "offset", "hub58", "hub59", "ring16", "ring17", "ring256")
PARTITION_CASES = ("uniform400", "tight", "wide", "disjoint", "offset", "hub58", "hub59", "ring16", "ring17", "ring256",
                   "redo_spread")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))          # xx, yy, zz, xy, xz, yz


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
        _lib.clip_box_moments_host_cell_box_moments.restype = C.c_int
        _lib.clip_box_moments_host_cell_box_moments.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32] + [
                                                                   C.c_void_p] * 6
    return _lib


def cell_box_moments(points, adjacency, offsets, box, geo: dict, cap: int = 256) -> dict:
    """The host build of the serial cell over every cell: site f64[N,6], central f64[N,6], status u32[N] and ``bad``.
    ``geo`` is what clip_box_host.cell_box returned for the same cloud and box."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    six = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
    assert six.shape == (6,)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    vol = np.ascontiguousarray(geo["volume"], dtype=np.float64)
    cen = np.ascontiguousarray(geo["centroid"], dtype=np.float64)
    ne = np.ascontiguousarray(geo["nonempty"], dtype=np.uint8)
    assert vol.shape == (n,) and cen.shape == (n, 3) and ne.shape == (n,)
    site, central, status = np.empty((n, 6)), np.empty((n, 6)), np.empty(n, dtype=np.uint32)
    bad = lib().clip_box_moments_host_cell_box_moments(pts.ctypes.data, n, adj.ctypes.data, off.ctypes.data, e,
                                                       bbox.ctypes.data, six.ctypes.data, cap, vol.ctypes.data,
                                                       cen.ctypes.data, ne.ctypes.data, site.ctypes.data,
                                                       central.ctypes.data, status.ctypes.data)
    return dict(site=site, central=central, status=status, bad=bad)


_HOST = {}


def host(name: str, cap: int = 256) -> dict:
    """the host build's moments for a case of clip_box_host.CASES, on clip_box_host.host's geometry (capacity 256), once"""
    if (name, cap) not in _HOST:
        c = B.case(name)
        _HOST[(name, cap)] = cell_box_moments(c["points"], c["adjacency"], c["offsets"], c["box"], B.host(name), cap=cap)
    return _HOST[(name, cap)]


def cells_of(name: str) -> tuple:
    """the cells clip_box_host.exact works on: the listed ones, or pick_cells from the sites' positions alone"""
    c = B.case(name)
    cells = B.CASES[name][2]
    return B.pick_cells(c["points"], c["box"]) if cells is None else tuple(cells)


def exact(name: str) -> dict:
    from tests import cell_box_moments_ref as X

    c = B.case(name)
    return X.exact_moments_in_box(c["points"], c["offsets"], c["adjacency"], c["box"], cells_of(name))


# ---- the checks ----------------------------------------------------------------------------------------------------------

def symmetric(six: np.ndarray) -> np.ndarray:
    """[M,6] as xx, yy, zz, xy, xz, yz -> [M,3,3]"""
    xx, yy, zz, xy, xz, yz = np.moveaxis(six, -1, 0)
    return np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)


def box_moment(box) -> np.ndarray:
    """the second moment of the box about its centre: V_box diag(e_k^2 / 12)"""
    e = np.asarray(box[3:], dtype=np.float64) - np.asarray(box[:3], dtype=np.float64)
    return np.diag(e.prod() * e * e / 12.0)


def check_shapes(c: dict, geo: dict, site, central):
    n = len(c["points"])
    assert site.shape == central.shape == (n, 6) and site.dtype == central.dtype == np.float64
    assert geo["volume"].shape == (n,) and geo["centroid"].shape == (n, 3) and geo["nonempty"].shape == (n,)


def check_against_exact(name: str, geo: dict, site, central) -> tuple:
    """Check 2: on every cell the exact reference worked on (none is left out: a boxed cell is never unbounded),
    |delta| <= 1e-9 tr Q_exact[a] on each of the twelve numbers of a cell that is non-empty in exact arithmetic; a cell
    that is exactly empty has site_moment == 0 exactly and NaN in central_moment.  Returns the worst ratios (site,
    central, and, without a bar, |delta central| / tr C_exact)."""
    c, ref = B.case(name), exact(name)
    check_shapes(c, geo, site, central)
    assert np.array_equal(np.nonzero(ref["done"])[0], np.array(sorted(cells_of(name))))
    empty = ref["done"] & (ref["volume_f"] == 0.0)
    solid = ref["done"] & ~empty
    assert not any(v == 0 for a, v in ref["volume"].items() if solid[a])          # 0 as a float is 0 as a Fraction
    assert solid.any()
    if empty.any():
        assert (site[empty] == 0.0).all() and np.isnan(central[empty]).all() and not geo["nonempty"][empty].any()
    assert geo["nonempty"][solid].all()
    unit = ref["trace_f"][solid][:, None]
    rs = float((np.abs(site[solid] - ref["site_f"][solid]) / unit).max())
    rc = float((np.abs(central[solid] - ref["central_f"][solid]) / unit).max())
    rcc = float((np.abs(central[solid] - ref["central_f"][solid]) / ref["trace_central_f"][solid][:, None]).max())
    print(f"{name}: {solid.sum()} solid and {empty.sum()} empty cells compared: worst |d site| / tr Q = {rs:.3g}, "
          f"|d central| / tr Q = {rc:.3g} (bar {BAR:.3g}); no bar: |d central| / tr C = {rcc:.3g}")
    assert rs <= BAR and rc <= BAR
    return rs, rc, rcc


def check_partition(c: dict, geo: dict, site, central, cells=None, total: bool = True) -> dict:
    """Check 4, on a whole cloud with a Delaunay CSR and without any reference.  Over the non-empty cells

        sum_a [Q_a + V_a (m_a q_a^T + q_a m_a^T + q_a q_a^T)] = V_box diag(e_k^2 / 12),   q_a = p_a - centre, m_a = c_a - p_a,

    to 1e-9 of that matrix's trace (the cells partition the box, and each summand is the cell's moment about the box's
    centre); per non-empty cell (``cells``: of those cells in their place)  tr site = tr central + V |c - p|^2  to 1e-9 tr
    site, and the smallest eigenvalue of central is >= -1e-9 tr site.  Every site_moment is finite, and central_moment
    is finite exactly where nonempty is set."""
    check_shapes(c, geo, site, central)
    box, pts = np.asarray(c["box"], dtype=np.float64), c["points"].astype(np.float64)
    ne, vol = geo["nonempty"].astype(bool), geo["volume"]
    assert np.isfinite(site).all() and np.isfinite(central[ne]).all() and np.isnan(central[~ne]).all()
    worst = {}
    if total:
        want = box_moment(box)
        q = pts[ne] - 0.5 * (box[:3] + box[3:])
        m = geo["centroid"][ne] - pts[ne]
        mq = m[:, :, None] * q[:, None, :]
        about = symmetric(site[ne]) + vol[ne, None, None] * (mq + np.swapaxes(mq, 1, 2) + q[:, :, None] * q[:, None, :])
        worst["partition"] = float(np.abs(about.sum(0) - want).max() / np.trace(want))
    per = ne if cells is None else np.asarray(cells, dtype=bool)
    if per.any():
        assert ne[per].all()
        tr_site, tr_central = site[per, :3].sum(1), central[per, :3].sum(1)
        assert (tr_site > 0).all()
        shift = vol[per] * ((geo["centroid"][per] - pts[per]) ** 2).sum(1)
        worst["trace"] = float((np.abs(tr_site - (tr_central + shift)) / tr_site).max())
        worst["eigenvalue"] = float((-np.linalg.eigvalsh(symmetric(central[per]))[:, 0] / tr_site).max())
    print(f"{c.get('name', '')}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (bar {BAR:.3g}); "
          f"{ne.sum()} of {len(pts)} cells non-empty")
    assert all(v <= BAR for v in worst.values()), worst
    return worst


def check_agreement(c: dict, geo: dict, site, central, bounded, plain_site, plain_central, share=None) -> int:
    """Check 5: on every cell cell_geometry calls bounded and whose wall_area is all zero, the twelve numbers agree with
    cell_moments' to 2e-9 tr site (each is within 1e-9 of exact; the two start from squares of different half-sides).
    ``share``: at least that part of the cloud is such a cell."""
    free = np.asarray(bounded, dtype=bool) & (geo["wall_area"] == 0.0).all(1)
    print(f"{c.get('name', '')}: {free.sum()} of {free.size} cells are bounded and touch no wall")
    if share is not None:
        assert free.sum() >= share * free.size
    assert free.any()
    unit = plain_site[free, :3].sum(1)[:, None]
    rs = float((np.abs(site[free] - plain_site[free]) / unit).max())
    rc = float((np.abs(central[free] - plain_central[free]) / unit).max())
    print(f"    |d site| / tr site = {rs:.3g}, |d central| / tr site = {rc:.3g} (bar {2 * BAR:.3g})")
    assert rs <= 2 * BAR and rc <= 2 * BAR
    return int(free.sum())


def whole_box_moments(box, p) -> tuple:
    """the closed form of the whole box about the site p: (site [6], central [6])"""
    box, p = np.asarray(box, dtype=np.float64), np.asarray(p, dtype=np.float64)
    e = box[3:] - box[:3]
    v = e.prod()
    lo, hi = box[:3] - p, box[3:] - p
    m = 0.5 * (box[:3] + box[3:]) - p
    site = np.concatenate([v / 3.0 * (hi ** 3 - lo ** 3) / e, v * np.array([m[0] * m[1], m[0] * m[2], m[1] * m[2]])])
    return site, np.concatenate([v * e * e / 12.0, np.zeros(3)])


def check_whole_box(box, p, site, central, a: int):
    """cell a is the whole box: the closed form to 1e-12 of its trace, the central off-diagonals exactly 0"""
    want_site, want_central = whole_box_moments(box, p[a])
    tr = want_site[:3].sum()
    assert np.abs(site[a] - want_site).max() <= 1e-12 * tr and np.abs(central[a] - want_central).max() <= 1e-12 * tr
    assert (central[a, 3:] == 0.0).all()


def check_grid(name: str, geo: dict, site, central):
    """Check 7, the unjittered grid (spacing 0.25) in its three boxes: the cells partition the box (in 'grid_bisectors'
    only if the tie rule is honoured: otherwise the first layer's pyramids count twice); in 'grid_between' the 64
    interior cells are cubes, 0.25^5 / 12 on the diagonal of both moments and nothing off it; in 'grid_bisectors' the flat
    cells outside have |site values| <= 1e-9 0.25^5, and the per-cell identities are asked of the 64 inside cells only."""
    c = B.case(name)
    h = H.GRID_H
    pts, box = c["points"].astype(np.float64), c["box"]
    if name == "grid_bisectors":
        inside = ((pts > box[:3]) & (pts < box[3:])).all(1)
        assert inside.sum() == 64
        check_partition(c, geo, site, central, cells=inside)
        assert np.abs(site[~inside]).max() <= BAR * h ** 5
    else:
        check_partition(c, geo, site, central)
    if name == "grid_between":
        inner = H.grid_interior()
        assert inner.sum() == 64
        for six in (site[inner], central[inner]):
            tr = six[:, :3].sum(1)[:, None]
            assert np.abs(six[:, :3] - h ** 5 / 12.0).max() <= BAR * 3.0 * h ** 5 / 12.0
            assert (np.abs(six[:, 3:]) <= BAR * tr).all()
