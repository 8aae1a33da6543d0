"""The foams of tests/foam_zoo.py on the CPU oracle alone: each one has the property it is there for, the oracle's
outputs on it are finite and opaque enough to carry gradients, the mirror of the kernels' scan (scan_mode("filtered"))
equals the literal reference scan bit for bit, and the reference's own summation-order noise leaves room under the
project's gradient bar (helpers.grad_close and relative L2 < 1e-5), which tests/test_gpu_foam_zoo.py applies unchanged."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import foam_zoo as Z
from tests import helpers as H
from tests import segments_ref as S


def _degrees(fm):
    return np.diff(fm["point_adjacency_offsets"].astype(np.int64))


def _scans(name):
    return int(Z.flat(name)["fwd"]["num_intersections"].sum())


def _nearest_neighbour_distances(pts):
    from scipy.spatial import cKDTree

    p = pts.astype(np.float64)
    return cKDTree(p).query(p, k=2)[0][:, 1]


def test_construction_rules():
    for name in Z.NAMES:
        fm = Z.foam(name)
        p, (r, s) = fm["points"], Z.rays(name)
        assert p.dtype == np.float32 and len(p) <= 7000 and not (p == 0).all(1).any(), name
        assert fm["sh_degree"] == Z.DEGREE[name] and fm["attributes"].shape == (len(p), 1 + 3 * (Z.DEGREE[name] + 1) ** 2)
        assert r.shape == (Z.NUM_RAYS, 6) and r.dtype == np.float32 and s.dtype == np.uint32
        d = p.astype(np.float64)[None, :, :] - r[:64, None, :3].astype(np.float64)       # exact start cells, a sample
        np.testing.assert_array_equal(np.argmin((d * d).sum(-1), axis=1), s[:64], err_msg=name)
        length = np.linalg.norm(r[:, 3:].astype(np.float64), axis=1)
        assert (np.abs(length - 1) > 1e-3).mean() > 0.1 and 0.45 < length.min() and length.max() < 2.1, name
        lo, hi = p.min(0), p.max(0)
        ext = Z.extent(p)
        o = r[:, :3].astype(np.float64)
        near = np.linalg.norm(o - p[s.astype(np.int64)], axis=1) < 6e-3 * ext
        far = np.linalg.norm(o - (lo.astype(np.float64) + hi) / 2, axis=1) > 0.9 * ext    # outside the box: > 0.87
        assert near.mean() >= 0.45 and far.mean() >= 0.2 and (near | far).all(), (name, near.mean(), far.mean())
        img, starts = Z.image(name)
        assert img.shape == (48, 64, 6) and starts.shape == (48, 64) and len(np.unique(starts)) == 1
        assert not ((img[0, 0, :3] >= lo) & (img[0, 0, :3] <= hi)).all(), name
        own = Z.edge_owner(fm)
        q = p.astype(np.float64)
        dist = np.linalg.norm(q[fm["point_adjacency"].astype(np.int64)] - q[own], axis=1)
        mean = np.bincount(own, dist) / np.bincount(own)
        np.testing.assert_allclose(fm["attributes"][:, -1] * mean, Z.TAU_OF.get(name, Z.TAU), rtol=1e-6, err_msg=name)
    a, b = Z.foam("scaled_2p13"), Z.foam("scaled_2p14")
    np.testing.assert_array_equal(a["point_adjacency"], b["point_adjacency"])          # found by delaunay_csr twice
    np.testing.assert_array_equal(a["point_adjacency_offsets"], b["point_adjacency_offsets"])
    np.testing.assert_array_equal(a["points"] * np.float32(2), b["points"])
    np.testing.assert_array_equal(a["attributes"][:, -1] * np.float32(0.5), b["attributes"][:, -1])
    np.testing.assert_array_equal(a["attributes"][:, :-1], b["attributes"][:, :-1])


@pytest.mark.parametrize("name", Z.NAMES)
def test_preconditions(name):
    """What each foam is there for (the figures in brackets: measured when the zoo was written)."""
    fm, (r, s) = Z.foam(name), Z.rays(name)
    deg, ho, m = _degrees(fm), Z.edge_offsets(fm), Z.mirror(name)
    scans, over = _scans(name), Z.overflowed_paddings(fm)
    print("%s: N %d, largest list %d, cell scans %d, contested in the mirror %d, largest offset %.4g, overflowed paddings "
          "%d, longest walk %d" % (name, len(fm["points"]), deg.max(), scans, m["contested"], ho.max(), over,
                                   Z.flat(name)["fwd"]["num_intersections"].max()))
    if name in ("scaled_2p13", "scaled_2p14"):
        big, bigger = int((ho > 8190).sum()), int((ho > 16380).sum())
        print("   offsets with a component > 8190: %d, > 16380: %d" % (big, bigger))
        assert not (ho >= 65504).any()
        base = Z.build(Z.points(name) * np.float32(2.0 ** -int(name[-2:])), 1, 1)
        unit = r.copy()
        unit[:, :3] *= np.float32(2.0 ** -int(name[-2:]))
        with O.scan_mode("filtered") as unscaled:
            O.trace_forward(*Z._args(base), unit, s, num_threads=1)
        print("   contested at the cloud's own scale: %d" % unscaled.final_contested)
        assert unscaled.final_contested < 50                              # [5]
        if name == "scaled_2p13":
            assert big > 100 and bigger == 0 and over > 0                 # [156, 0, 18]
            assert m["contested"] > 1000                                  # [2162 of 102,159]
        else:
            assert big > 500 and bigger > 100 and over > 50               # [774, 156, 77]
            assert m["contested"] > 3000                                  # [5753 of 101,442]
    else:
        assert over == 0, name
    if name == "hub":
        assert deg.max() > 2000                                           # [2312: 578 blocks of four]
        cells, _, _ = O.trace_paths(*Z._args(fm), r, s, cap=S.CAP)
        share = float((cells == Z.hub_site(fm)).any(1).mean())
        print("   rays that visit the hub's cell: %.3f" % share)
        assert share >= 0.25                                              # [0.553]
    if name == "clustered":
        nn = _nearest_neighbour_distances(fm["points"])
        print("   nearest-neighbour distances %.3g to %.3g" % (nn.min(), nn.max()))
        assert nn.max() / nn.min() >= 1e3                                 # [4.6e-6 to 1.27]
        half = fm["points"][fm["point_adjacency"].astype(np.int64)] - fm["points"][Z.edge_owner(fm)]
        tiny = np.abs(half.astype(np.float16).astype(np.float32))
        assert ((tiny > 0) & (tiny < 6.2e-5)).any() and (tiny > 1).any()  # subnormal and normal fp16 offsets together
    if name == "sheet":
        longest = int(Z.flat(name)["fwd"]["num_intersections"].max())
        assert 100 < longest < S.CAP                                      # [112]
    if name == "lattice":
        o, d = r[:, :3], r[:, 3:]
        on_site = (o[:, None, :] == fm["points"][None, :, :]).all(-1).any(1)
        axis = ((d != 0).sum(1) == 1) & (np.abs(d).sum(1) == 1)
        assert (on_site & axis).sum() == Z.NUM_RAYS // 2
        assert m["contested"] > 0                                         # [10,030 of 39,490]
    if name == "unbounded":
        assert 2000 < ho.max() < 8190                                     # [2833]
    if name == "near_duplicates":
        nn = _nearest_neighbour_distances(fm["points"])
        assert len(fm["points"]) == 400 and (nn < 3e-4).sum() == 200
        assert m["contested"] > 100                                       # [436 of 57,244]


@pytest.mark.parametrize("name", Z.NAMES)
def test_oracle_outputs_are_finite_and_opaque(name):
    flat, frame = Z.flat(name), Z.frame(name)
    for group in (flat["fwd"], flat["bwd"], frame, Z.noise(name), Z.half_forward(name)[1]):
        for key, value in group.items():
            if value.dtype.kind == "f":
                assert np.isfinite(value).all(), (name, key)
    alpha = flat["fwd"]["rgba"][:, 3]
    print("%s: rays with alpha > 0.5: %.3f, saturated: %d; frame: largest alpha %.3f" % (
        name, (alpha > 0.5).mean(), (alpha == 1).sum(), frame["rgba"][..., 3].max()))
    assert (alpha > 0.5).mean() >= 0.9 and (alpha == 1).mean() < 0.1
    assert frame["rgba"][..., 3].max() > 0.5
    di = flat["fwd"]["depth_indices"]
    assert (di != Z.NONE).any()
    for key in flat["bwd"]:
        assert np.abs(flat["bwd"][key]).max() > 0, (name, key)
    if name in Z.HALF_BACKWARD:
        h = Z.half(name)
        for key in ("attr_grad", "point_error"):
            assert np.isfinite(h["bwd"][key]).all() and np.abs(h["bwd32"][key]).max() < 65504.0, (name, key)


@pytest.mark.parametrize("name", Z.NAMES)
def test_mirror_equals_the_literal_scan(name):
    """scan_mode("filtered") against the reference's loop, forward and one-thread backward, bit for bit."""
    lit, mir = Z.flat(name), Z.mirror(name)
    for part, keys in (("fwd", ("rgba", "num_intersections", "depth", "depth_indices", "contribution")),
                       ("bwd", ("points_grad", "attr_grad", "point_error"))):
        for key in keys:
            np.testing.assert_array_equal(lit[part][key].view(np.uint32), mir[part][key].view(np.uint32),
                                          err_msg="%s %s" % (name, key))
    if name in Z.QUANTILE_GRADS:
        assert (lit["fwd"]["depth_indices"] != Z.NONE).any()


@pytest.mark.parametrize("name", Z.NAMES)
def test_order_noise_of_the_oracle_leaves_room_under_the_gradient_bar(name):
    """The same one-thread backward with the rays permuted: the two results differ by the order of the sums alone.  At
    most 0.1 of grad_close's bound on the worst element and 1e-6 relative L2 [measured over all foams: 0.0043 and 4.6e-7],
    so the bar of the GPU comparisons (1.0 of the bound, 1e-5) is ten times wider than the reference's own noise."""
    ref, other = Z.flat(name)["bwd"], Z.noise(name)
    for key in ("points_grad", "attr_grad", "point_error"):
        ok, rel, worst = H.grad_close(other[key], ref[key])
        print("%s %s: order noise: worst element at %.3g of its bound, relative L2 %.3g" % (name, key, worst, rel))
        assert ok and worst <= 0.1 and rel <= 1e-6, (name, key, worst, rel)


def test_world_origin_site_poisons_exactly_its_own_row():
    """The reference's phantom first-cell term is 0/0 for a start cell whose site is (0, 0, 0): the oracle's points_grad
    is NaN in that row and finite everywhere else, attr_grad is finite."""
    c = Z.origin_case()
    assert (c["fm"]["points"][c["site"]] == 0).all() and (c["starts"] == c["site"]).all()
    bad = ~np.isfinite(c["bwd"]["points_grad"])
    assert bad[c["site"]].all() and not np.delete(bad, c["site"], axis=0).any()
    assert np.isfinite(c["bwd"]["attr_grad"]).all() and np.isfinite(c["fwd"]["rgba"]).all()
    assert (c["fwd"]["rgba"][:, 3] > 0.5).mean() >= 0.9


def test_walk_reference_enters_at_zero_behind_a_negative_first_exit():
    """segments_ref.to_csr derives t_enter as the compositing's t0: 0, then the running maximum of 0 and the earlier exits.
    A ray whose origin lies a rounding outside its start cell leaves that cell at a negative t (far from the world origin
    the rounding is large: `translated`, `unbounded`); its second cell is entered at 0, not at the negative exit."""
    negative_first_exits = 0
    for name in Z.NAMES:
        seg = Z.segments(name)
        first = seg["offsets"][:-1]
        assert (seg["t_enter"][first] == 0).all() and (seg["t_enter"] >= 0).all(), name
        behind = first[(seg["t_exit"][first] < 0) & (seg["counts"] > 1)] + 1
        assert (seg["t_enter"][behind] == 0).all(), name
        negative_first_exits += len(behind)
        np.testing.assert_array_equal(seg["n"], Z.flat(name)["fwd"]["num_intersections"].reshape(-1))
    print("rays with a negative first exit:", negative_first_exits)
    assert negative_first_exits > 0
