"""radfoam.delaunay_tets without a GPU: the host build of csrc/rf_tets.hpp (tests/host_harness/tets_host.cpp) and the
CPU-tensor path against Qhull's simplices canonicalised with exact signs (tests/tets_ref.py).

The clouds: uniform, clustered over three decades, a sphere shell, a cloud offset by +1000 and one scaled by 1e-3, each
with n = 33, 64, 65, 400 and 3000 -- below, at and above the 64 sites of a wave, and sizes with several hundred owners;
hubs with 100 and 300 neighbours for the second and third star instance; malformed and stale lists; a 4x4x4 lattice.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import radfoam_amd.build as build
from radfoam_amd.triangulation import TriangulationFailedError
from tests import tets_ref as R
from tests.host_harness import tets_host as HT


def test_sources_are_outside_the_source_hash():
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_tets.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_tets.hpp", "radfoam_hip_tets.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    for path in build.EXTRA_SOURCES + build.EXTRA_HEADERS:
        assert os.path.exists(path)


@pytest.mark.parametrize("kind,n", R.CLOUDS)
def test_host_build_equals_qhull(kind, n):
    ref = R.cloud(kind, n)
    got = HT.delaunay_tets(ref["points"], ref["adjacency"], ref["offsets"])
    R.check_against(ref, got["tets"], got["vert_to_tet"], got["tet_adjacency"], got["hull_faces"])
    # every site emits exactly the rows it is the smallest site of
    assert np.array_equal(got["owned"], np.bincount(ref["tets"][:, 0], minlength=n))


@pytest.mark.parametrize("k,instance", [(100, "big"), (300, "huge")])
def test_host_hub_goes_through_the_larger_instances(k, instance):
    ref = R.cloud("hub", k)
    assert int(ref["offsets"][1]) - int(ref["offsets"][0]) == k     # Qhull gives the centre every shell point
    got = HT.delaunay_tets(ref["points"], ref["adjacency"], ref["offsets"])
    assert got[instance] >= 1 and got["code"][0] == (4 if instance == "big" else 5)
    R.check_against(ref, got["tets"], got["vert_to_tet"], got["tet_adjacency"], got["hull_faces"])


@pytest.mark.parametrize("name", ["self", "twice", "above", "below", "offsets", "short"])
def test_host_malformed_lists_raise_runtime_error(name):
    ref = R.cloud("uniform", 400)
    adj, off = R.malformed_lists(ref)[name]
    with pytest.raises(RuntimeError) as err:
        HT.delaunay_tets(ref["points"], adj, off)
    assert not isinstance(err.value, TriangulationFailedError)


@pytest.mark.parametrize("name", ["removed", "added"])
def test_host_stale_lists_raise_triangulation_failed(name):
    ref = R.cloud("uniform", 400)
    adj, off = R.stale_lists(ref)[name]
    with pytest.raises(TriangulationFailedError):
        HT.delaunay_tets(ref["points"], adj, off)


def test_host_lattice_raises_or_returns_a_checked_mesh():
    def run(pts, adj, off):
        got = HT.delaunay_tets(pts, adj, off)
        return got["tets"], got["vert_to_tet"], got["tet_adjacency"], got["hull_faces"]
    assert R.lattice_outcome(run) in ("raised", "returned")


# ---- the public operator on CPU tensors -------------------------------------------------------------------------------

def _call(ref, adj=None, off=None, dtype=torch.int64, adjacency=True, device="cpu"):
    import radfoam
    adj = ref["adjacency"] if adj is None else adj
    off = ref["offsets"] if off is None else off
    as_t = lambda x: torch.from_numpy(np.asarray(x).astype(np.int64)).to(dtype).to(device)
    return radfoam.delaunay_tets(torch.from_numpy(ref["points"]).to(device), as_t(adj), as_t(off), adjacency=adjacency)


def test_cpu_tensors_equal_the_reference():
    import radfoam
    ref = R.cloud("uniform", 400)
    got = _call(ref)
    assert isinstance(got, radfoam.DelaunayTets) and got.tets.dtype == torch.uint32 and got.tets.device.type == "cpu"
    R.check_against(ref, got.tets.numpy(), got.vert_to_tet.numpy(), got.tet_adjacency.numpy(), got.hull_faces)
    assert _call(ref, adjacency=False).tet_adjacency is None
    for dtype in (torch.int32, torch.uint32):
        again = _call(ref, dtype=dtype)
        assert torch.equal(again.tets, got.tets) and torch.equal(again.tet_adjacency, got.tet_adjacency)


def test_cpu_tensors_raise_on_stale_and_malformed_lists():
    ref = R.cloud("uniform", 400)
    for adj, off in R.stale_lists(ref).values():
        with pytest.raises(TriangulationFailedError):
            _call(ref, adj, off)
    for adj, off in R.malformed_lists(ref).values():
        with pytest.raises(RuntimeError) as err:
            _call(ref, adj, off)
        assert not isinstance(err.value, TriangulationFailedError)
