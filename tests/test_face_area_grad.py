"""Point gradients of the face areas, the part that runs without a GPU: radfoam_amd/csrc/rf_clip_area_grad.hpp compiled
for the host (tests/host_harness/clip_area_grad_host) against difference quotients of the exact face areas
(tests/face_area_grad_ref.py), the labelled clipping against the plain one, the translation, rotation and scaling
identities, and the degenerate inputs.  tests/test_gpu_face_area_grad.py holds the device to the same bars.

Measured on the host (spread / max |R| of the reference, then the worst |<grad, delta> - R| / spread over the probes):
  uniform400 1.1e-6 0.24, hub64 2.4e-8 0.12, hub65 2.9e-10 0.13, ring16 1.8e-8 0.31, ring17 1.6e-8 0.34,
  redo_spread 4.8e-5 0.027.

The identities hold to 2e-15 on uniform and offset, 2e-11 on clustered and 2e-16 on the unjittered grid.  On the grid
four sites are cocircular around every Voronoi edge, the planes of two neighbours pass through the same edge line and
which of them labels an edge is decided by rounding, differently from row to row: the rows agree there because
add_polygon_terms takes an edge's triangles from the adjacency (DESIGN, "Cocircular sites"), not from the label alone;
with the label alone the three identities were off by 0.10, 0.031 and 0.062 of sum |p||grad|."""
import os

import numpy as np
import pytest

from tests import face_area_grad_ref as F
from tests.host_harness import clip_area_grad_host as HA
from tests.host_harness import clip_grad_host as HG
from tests.host_harness import clip_host as H

# A clipped vertex is the crossing of two lines in the face's plane, computed in double from numbers of the face's size:
# a few ulp of that size, times the conditioning of the crossing (the 17-gons and the hubs' faces have edges that meet at
# flat angles).  Measured worst over every labelled edge of a face of finite positive area, of the face's size:
# uniform400 3.8e-13, hub64 6.9e-13, hub65 1.3e-12, ring16 4.5e-13, ring17 5.1e-13, redo_spread 2.4e-13.  The bar leaves
# a margin of 75 over the worst of them; a wrong label is off by the order of 1.
BISECTOR_BAR = 1e-10


def _rounded(name):
    """(case on the 2^-16 grid, host forward)"""
    c = F.case(name)
    return c, HG.host_forward(("rounded", name), c)


def _host_grad(c, geo, g, cap=256):
    got = HA.face_area_grad(c["points"], c["adjacency"], c["offsets"], geo["face_area"], g, cap=cap)
    assert got["bad"] == 0
    return got["grad"]


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_face_area_grad.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_area_grad.hpp", "radfoam_hip_face_area_grad.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_face_area_grad", "rf_face_area_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_face_area_grad_workspace_bytes(1000, 100) >= 1000 + 800
    none = [None] * 4
    assert lib.rf_face_area_grad(None, 0, None, None, 0, None, *none, None, 0, None) == 0      # nothing to do
    assert lib.rf_face_area_grad(None, 5, None, None, 0, None, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_face_area_grad(dummy, 5, dummy, dummy, 4, dummy, *([dummy] * 4), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_input_checks_without_a_device():
    import torch

    import radfoam
    import radfoam_amd

    assert "face_area_grad" in radfoam.__all__ and "face_area_grad" in radfoam_amd.__all__
    assert callable(radfoam.face_area_grad)
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.face_area_grad(pts, adj, off, None, None)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.differentiable_cell_geometry(pts, adj, off, face_area=True)


@pytest.mark.parametrize("name", F.FD_CASES)
def test_gradient_matches_difference_quotients_of_the_exact_areas(name):
    c, geo = _rounded(name)
    pairs = F.faces_and_weights(c)[0]
    keep = F.kept(c, pairs, geo["face_area"])
    ref, rec = F.reference(name, keep), F.recorded(name)
    assert np.array_equal(rec["keep"], keep) and np.array_equal(rec["R"], ref["R"])             # the record the GPU
    assert np.array_equal(rec["spread"], ref["spread"]) and np.array_equal(rec["g"], ref["g"])   # tests read
    g = np.where(np.isfinite(geo["face_area"]), ref["g"], np.nan)      # nothing may read the slots of infinite area
    grad = _host_grad(c, geo, g)
    F.check_against_reference(name, ref, grad)
    # the same through a capacity that just fits, and a capacity below the face is reported, never a wrong number
    if name in ("ring16", "ring17"):
        k = int(name[4:])
        fits = HA.face_area_grad(c["points"], c["adjacency"], c["offsets"], geo["face_area"], g, cap=k)
        assert (fits["status"][:2] == 0).all() and np.array_equal(fits["grad"][:2], grad[:2])
        small = HA.face_area_grad(c["points"], c["adjacency"], c["offsets"], geo["face_area"], g, cap=k - 1)
        assert (small["status"][:2] == 1).all() and np.isnan(small["grad"][:2]).all()
        ok = small["status"] == 0
        assert np.array_equal(small["grad"][ok], grad[ok])


@pytest.mark.parametrize("name", F.FD_CASES)
def test_labelled_clipping_keeps_the_vertices_and_labels_the_bisectors(name):
    """Every face of the cloud: the labelled step's vertices are clip_step's bit for bit (both from the backward's
    square), and on the faces of finite positive area every edge of nonzero length lies on the bisector plane of the
    neighbour its label names, at both endpoints, to BISECTOR_BAR of the face's size."""
    c, geo = _rounded(name)
    p, off, adj = c["points"].astype(np.float64), c["offsets"].astype(np.int64), c["adjacency"].astype(np.int64)
    worst, edges = 0.0, 0
    for a in range(len(p)):
        for slot in range(off[a], off[a + 1]):
            poly = HA.labelled_polygon(c["points"], c["adjacency"], c["offsets"], a, slot)
            assert poly is not None and np.array_equal(poly["st"], poly["plain"])
            if not 0.0 < geo["face_area"][slot] < np.inf:     # unbounded, or clipped away by the forward's square
                continue
            y, lab = poly["xyz"], poly["label"]
            assert (lab != HA.NO_LABEL).all() and (lab < off[a + 1] - off[a]).all() and (lab != slot - off[a]).all()
            size = np.linalg.norm(y - 0.5 * (p[adj[slot]] - p[a]), axis=1).max()
            nxt = np.roll(y, -1, axis=0)
            for i in np.nonzero(np.linalg.norm(nxt - y, axis=1) > 0.0)[0]:
                d = p[adj[off[a] + lab[i]]] - p[a]
                for end in (y[i], nxt[i]):
                    worst = max(worst, abs(d @ end - 0.5 * d @ d) / np.linalg.norm(d) / size)
                edges += 1
    print(f"{name}: worst distance of a labelled edge's endpoint from its bisector = {worst:.3g} of the face's size, "
          f"{edges} edges")
    assert edges > 100 and worst <= BISECTOR_BAR


@pytest.mark.parametrize("name", ["uniform", "offset", "clustered", "grid"])
def test_translation_rotation_and_scaling_identities(name):
    c = H.case(name)
    geo = HG.host_forward(("plain", name), c)
    assert np.isfinite(geo["face_area"]).sum() >= (1000 if name == "grid" else 3000)
    g = HA.unit_upstream(c, geo)
    HA.check_identities(c["points"], geo["face_area"], g, _host_grad(c, geo, g))


def test_non_finite_upstreams_on_unbounded_faces_do_not_leak():
    c, geo = _rounded("uniform400")
    fin = np.isfinite(geo["face_area"])
    assert (~fin).sum() > 100
    g = HA.unit_upstream(c, geo)                 # NaN on the slots of infinite area
    clean = _host_grad(c, geo, np.where(fin, g, 0.0))
    for bad in (np.nan, np.inf, -np.inf):
        assert np.array_equal(_host_grad(c, geo, np.where(fin, g, bad)), clean)
    unbounded = ~geo["bounded"]
    assert np.isfinite(clean).all() and np.abs(clean[unbounded]).max() > 0.0   # open rows carry their finite faces


def test_tiny_inputs_and_asymmetric_rows_stay_finite():
    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):          # every face is unbounded: zeros, whatever arrives
        pts, off, adj = tiny[name]
        geo = H.cell_geometry(pts, adj, off)
        assert not np.isfinite(geo["face_area"]).any()
        got = HA.face_area_grad(pts, adj, off, geo["face_area"], np.full(len(adj), np.nan))
        assert got["bad"] == 0 and (got["grad"] == 0.0).all()
    # an empty row, which is also a row that omits sites that list it: the mate slots and the slots b -> c it would
    # hold have weight zero
    pts, off, adj = tiny["empty_row"]
    geo = H.cell_geometry(pts, adj, off)
    a = H.EMPTY_ROW_SITE
    assert off[a] == off[a + 1] and (adj == a).sum() > 3
    c = dict(rows=np.repeat(np.arange(len(pts)), np.diff(off.astype(np.int64))), adjacency=adj)
    got = HA.face_area_grad(pts, adj, off, geo["face_area"], HA.unit_upstream(c, geo))
    assert got["bad"] == 0 and np.isfinite(got["grad"]).all() and (got["grad"][a] == 0.0).all()
    assert np.abs(got["grad"]).max() > 0.0
    # a row that drops one of its sites while that site still lists it
    pts, off, adj = tiny["empty_row_full"]
    off = off.astype(np.int64)
    b = int(adj[off[a]])
    adj2, off2 = np.delete(adj, off[a]), off.copy()
    off2[a + 1:] -= 1
    geo = H.cell_geometry(pts, adj2, off2)
    c = dict(rows=np.repeat(np.arange(len(pts)), np.diff(off2)), adjacency=adj2)
    assert a in adj2[off2[b]:off2[b + 1]] and b not in adj2[off2[a]:off2[a + 1]]
    got = HA.face_area_grad(pts, adj2, off2, geo["face_area"], HA.unit_upstream(c, geo))
    assert got["bad"] == 0 and np.isfinite(got["grad"]).all()


def test_malformed_rows_are_reported():
    c, geo = _rounded("ring16")
    adj = c["adjacency"].copy()
    off = c["offsets"].astype(np.int64)
    adj[off[3]] = 3                       # the site itself
    adj[off[7] + 1] = len(c["points"])    # past the end
    g = np.where(np.isfinite(geo["face_area"]), 1.0, np.nan)
    got = HA.face_area_grad(c["points"], adj, c["offsets"], geo["face_area"], g)
    assert got["status"][3] == 2 and got["status"][7] == 2 and got["bad"] == 2
    assert np.isnan(got["grad"][[3, 7]]).all() and np.isfinite(np.delete(got["grad"], [3, 7], axis=0)).all()
