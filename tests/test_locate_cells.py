"""radfoam.locate_cells without a GPU: the host build of csrc/rf_nearest.hpp (tests/host_harness/nearest_host.cpp) and the
numpy restatement of radfoam_amd/nearest.py against each other and against the exact nearest sites (Fractions of the
float32 inputs, tests/nearest_ref.py); the local-minimum guarantee on stale lists, the faults, the small shapes, the exact
path's share, and the fp32 brute-force operator."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import nearest_ref as R
from tests.host_harness import nearest_host as H

MODES = ("seeded", "site0", "given")


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t if dtype is None else t.to(dtype)


def _lists(adj, offsets, dtype=torch.int64):
    a, o = _t(np.asarray(adj).astype(np.int64)), _t(np.asarray(offsets).astype(np.int64))
    if dtype == torch.uint32:
        return a.to(torch.int32).view(torch.uint32), o.to(torch.int32).view(torch.uint32)
    return a.to(dtype), o.to(dtype)


def _mode(kind, n, mode):
    """the keywords of a start mode, for the host build (numpy) and for radfoam.locate_cells (torch)"""
    if mode == "seeded":
        return {}, {}
    if mode == "site0":
        return dict(seeds=0), dict(seeds=0)
    start = R.given_starts(kind, n)
    return dict(start=start), dict(start=_t(start))


def _locate(points, adj, offsets, q, dtype=torch.int64, **kw):
    import radfoam
    got = radfoam.locate_cells(_t(points), *_lists(adj, offsets, dtype), _t(q), **kw)
    assert got.cell.dtype == torch.int64 and got.hops.dtype == torch.int32
    return got.cell.numpy(), got.hops.numpy()


@pytest.mark.parametrize("kind,n", R.CLOUDS)
def test_the_two_builds_agree_and_every_cell_is_a_nearest_site(kind, n):
    m, q = R.cloud(kind, n), R.queries(kind, n)["q"]
    for mode in MODES:
        host_kw, kw = _mode(kind, n, mode)
        host = H.locate(m["points"], m["adjacency"], m["offsets"], q, **host_kw)
        cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q, **kw)
        assert np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"]), mode
        # zero mismatches: the one nearest site where it is unique -- from every start --, one of them where sites tie
        assert R.check_nearest(kind, n, cell) == 0, mode
        assert (cell[-2:] == -1).all() and (hops[-2:] == 0).all()


@pytest.mark.parametrize("kind,n", [("uniform", 400), ("clustered", 400), ("hub", 301)])
def test_no_entry_of_the_cells_row_has_a_smaller_key_stale_lists_included(kind, n):
    m, q = R.cloud(kind, n), R.queries(kind, n)["q"]
    for adj, off in ((m["adjacency"], m["offsets"]), R.stale(m)):
        for mode in MODES:
            host_kw, kw = _mode(kind, n, mode)
            host = H.locate(m["points"], adj, off, q, **host_kw)
            cell, hops = _locate(m["points"], adj, off, q, **kw)
            assert np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"])
            assert (cell[:-2] >= 0).all()
            R.check_local_minimum(m["points"], adj, off, q, cell)


def test_every_fault_kind_raises_naming_the_first_query_and_leaves_nothing_behind():
    m = R.cloud("uniform", 400)
    valid = R.valid_queries(m)
    want = H.locate(m["points"], m["adjacency"], m["offsets"], valid)
    kinds = {"start": 0, "offsets": 1, "past": 1, "above": 2, "below": 2}
    for name, (adj, off, start, q) in R.malformed(m).items():
        for dtype in (torch.int64, torch.int32):
            host = H.locate(m["points"], adj.astype(np.int32) if dtype == torch.int32 else adj,
                            off.astype(np.int32) if dtype == torch.int32 else off, q, start=start)
            first = int(np.nonzero(host["cell"] < -1)[0][0])
            assert (-2 - int(host["cell"][first])) & 7 == kinds[name], name
            with pytest.raises(RuntimeError, match=f"locate_cells: query {first}:"):
                _locate(m["points"], adj, off, q, dtype, start=_t(start))
            cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], valid)
            assert np.array_equal(cell, want["cell"]) and np.array_equal(hops, want["hops"]), name


def test_the_hop_cap_raises():
    m, q = R.cloud("uniform", 400), R.queries("uniform", 400)["q"]
    host = H.locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0, max_hops=2)
    first = int(np.nonzero(host["cell"] < -1)[0][0])
    assert (-2 - int(host["cell"][first])) & 7 == 3
    with pytest.raises(RuntimeError, match=f"query {first}: its walk would take more than max_hops = 2"):
        _locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0, max_hops=2)
    whole = H.locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0)
    cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0)
    assert np.array_equal(cell, whole["cell"]) and np.array_equal(hops, whole["hops"]) and hops.max() > 2


def test_small_shapes():
    import radfoam
    m, q = R.cloud("uniform", 64), R.queries("uniform", 64)["q"]
    cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q)
    assert (hops == 0).all() and R.check_nearest("uniform", 64, cell) == 0      # N < S: every site is a seed
    for count in (0, 1):
        cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q[:count])
        host = H.locate(m["points"], m["adjacency"], m["offsets"], q[:count])
        assert cell.shape == (count,) and np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"])
    grid = radfoam.locate_cells(_t(m["points"]), _t(m["adjacency"]), _t(m["offsets"]), _t(q[:60]).reshape(6, 10, 3),
                                start=torch.zeros((6, 10), dtype=torch.int32))
    flat = H.locate(m["points"], m["adjacency"], m["offsets"], q[:60], start=np.zeros(60, dtype=np.int64))
    assert grid.cell.shape == (6, 10) and np.array_equal(grid.cell.numpy().reshape(-1), flat["cell"])
    # an empty row answers its own site
    adj, off = m["adjacency"].astype(np.int64), m["offsets"].astype(np.int64)
    i = 9
    lone_adj = np.concatenate([adj[:off[i]], adj[off[i + 1]:]])
    lone_off = off.copy()
    lone_off[i + 1:] -= off[i + 1] - off[i]
    start = np.full(len(q), i, dtype=np.int64)
    host = H.locate(m["points"], lone_adj, lone_off, q, start=start)
    cell, hops = _locate(m["points"], lone_adj, lone_off, q, start=_t(start))
    assert np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"])
    assert (cell[:-2] == i).all() and (hops == 0).all()


@pytest.mark.parametrize("dtype", [torch.uint32, torch.int32, torch.int64])
def test_list_dtypes(dtype):
    m, q = R.cloud("clustered", 400), R.queries("clustered", 400)["q"]
    want = H.locate(m["points"], m["adjacency"], m["offsets"], q)
    cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q, dtype)
    assert np.array_equal(cell, want["cell"]) and np.array_equal(hops, want["hops"])
    wide = H.locate(m["points"], m["adjacency"].astype(np.int64), m["offsets"].astype(np.int64), q)
    assert np.array_equal(wide["cell"], want["cell"]) and np.array_equal(wide["hops"], want["hops"])


@pytest.mark.parametrize("kind,n", [("uniform", 400), ("offset", 400), ("hub", 301)])
def test_the_exact_path_is_taken_on_the_ties_and_only_there(kind, n):
    m, parts = R.cloud(kind, n), R.queries(kind, n)
    q = parts["q"]
    for kw in ({}, dict(seeds=0)):
        ties = H.locate(m["points"], m["adjacency"], m["offsets"], q[parts["mids"]], **kw)
        uniform = H.locate(m["points"], m["adjacency"], m["offsets"], q[parts["uniform"]], **kw)
        print(f"{kind} {n} {kw}: {ties['exact']} of {ties['predicates']} predicates left the filter on the ties, "
              f"{uniform['exact']} of {uniform['predicates']} on the uniform queries")
        assert ties["exact"] >= len(q[parts["mids"]]) and uniform["exact"] == 0 and uniform["predicates"] > 0


def test_the_exact_path_equals_fractions():
    from radfoam_amd.nearest import exact_closer
    rng = np.random.default_rng(17)
    for scale in (1.0, 1e-3, 1e3):
        a, q = (scale * rng.uniform(-1, 1, (2, 40, 3))).astype(np.float32)
        b = (2 * q.astype(np.float64) - a.astype(np.float64)).astype(np.float32)      # the mirror image of a, rounded
        b[::4] = a[::4]                                                           # and the same point
        for k in range(40):
            assert H.exact_closer(a[k], b[k], q[k]) == exact_closer(a[k], b[k], q[k]), (scale, k)
            assert H.exact_closer(b[k], a[k], q[k]) == -exact_closer(a[k], b[k], q[k])


def _nearest_point_fp32(points, q):
    """nearest_point restated: squared fp32 distance, lowest index among ties"""
    d = points[None, :, :] - q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    return d2.argmin(1), d2


@pytest.mark.parametrize("kind,n", [("uniform", 3000), ("clustered", 3000), ("offset", 400)])
def test_against_the_fp32_operator(kind, n):
    """Equal to the fp32 brute force except where the two candidates' fp32 distances are within rounding of each other --
    an fp32 squared distance carries at most 5 roundings of 2^-24 (the difference twice, the square, two sums), so two
    whose exact order is the reverse of their fp32 order differ by at most 10 of them, second order included 12 -- and
    there the exact predicate sides with locate_cells."""
    from radfoam_amd.nearest import exact_closer
    m, parts = R.cloud(kind, n), R.queries(kind, n)
    q = parts["q"][parts["uniform"]]
    cell, _ = _locate(m["points"], m["adjacency"], m["offsets"], q)
    theirs, d2 = _nearest_point_fp32(m["points"], q)
    differ = np.nonzero(cell != theirs)[0]
    print(f"{kind} {n}: {len(differ)} of {len(q)} queries differ from the fp32 operator")
    for k in differ:
        mine, other = d2[k, cell[k]], d2[k, theirs[k]]
        assert abs(float(mine) - float(other)) <= 12 * 2.0 ** -24 * max(float(mine), float(other)), k
        assert exact_closer(m["points"][cell[k]], m["points"][theirs[k]], q[k]) <= 0, k


def test_arguments_are_checked():
    import radfoam
    m, q = R.cloud("uniform", 64), R.queries("uniform", 64)["q"]
    p, (a, o), x = _t(m["points"]), _lists(m["adjacency"], m["offsets"]), _t(q)
    assert radfoam.CellLocation is type(radfoam.locate_cells(p, a, o, x))
    for bad in (lambda: radfoam.locate_cells(p.double(), a, o, x), lambda: radfoam.locate_cells(p, a, o[:-1], x),
                lambda: radfoam.locate_cells(p, a, o, x.double()), lambda: radfoam.locate_cells(p, a.float(), o, x),
                lambda: radfoam.locate_cells(p, a, o, x, seeds=1025), lambda: radfoam.locate_cells(p, a, o, x, seeds=-1),
                lambda: radfoam.locate_cells(p, a, o, x, start=torch.zeros(3, dtype=torch.int64)),
                lambda: radfoam.locate_cells(p[:0], a, o[:1], x), lambda: radfoam.locate_cells(p, a, o, x, backend="hip")):
        with pytest.raises(RuntimeError):
            bad()
