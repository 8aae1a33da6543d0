"""Non-uniform and degenerate foams for the parity tests, with the CPU oracle's answers (tests/test_foam_zoo.py asserts
what each one is for, tests/test_gpu_foam_zoo.py traces them on the GPU).  Everything is seeded, built with foam.kd_order
and foam.delaunay_csr, computed once per process and never modified by its users.

Every cloud is translated by SHIFT x its extent so that no site is the world origin (the reference's phantom first-cell
term is 0/0 for a start cell at (0, 0, 0): `origin_case` below is the one input that keeps such a site, on purpose).  The
density of a cell is TAU / (mean distance to its neighbours), whatever the foam's scale.

  foam(name, sh_degree=None)  the foam dict (sh_degree: DEGREE[name] unless given)
  rays(name)                  4096 flat rays [R, 6] and their start cells [R]
  image(name)                 a 64x48 pinhole frame [48, 64, 6] from outside the bounding box, and its start cells [48, 64]
  flat / mirror / noise / frame / half_forward / half / segments (name), origin_case()   the oracle's answers
"""
import numpy as np

from radfoam_amd import foam as foam_mod

NAMES = ("scaled_2p13", "scaled_2p14", "hub", "clustered", "sheet", "lattice", "translated", "unbounded",
         "near_duplicates")
#: SH degree the oracle's answers are computed at
DEGREE = {"scaled_2p13": 1, "scaled_2p14": 1, "hub": 2, "clustered": 3, "sheet": 0, "lattice": 1, "translated": 2,
          "unbounded": 0, "near_duplicates": 1}
#: foams whose flat backward carries depth-quantile gradients (the others run the instances without them)
QUANTILE_GRADS = ("hub", "clustered", "sheet", "lattice", "unbounded")
#: foams whose fp16 backward is checked (helpers.half_reference; attr_grad leaves fp16 on `unbounded`)
HALF_BACKWARD = ("hub", "scaled_2p14")
SHIFT = np.array([0.013, -0.007, 0.021])
TAU = 0.3
#: the sheet alone is thinner: at 0.3 a ray is opaque after ~65 of its cells, and the sheet is there for walks of 100+
TAU_OF = {"sheet": 0.1}
NUM_RAYS = 4096
NONE = 0xFFFFFFFF

_SEED = {name: 100 + i for i, name in enumerate(NAMES)}
# how many of the 100 pairs get the same fp16 offset from a common neighbour (an exact tie in that neighbour's list)
# varies a lot with the cloud: over twelve seeds the mirror's contested count ran from 97 to 717, median about 430
_SEED["near_duplicates"] = 209
_POINTS, _FOAMS, _RAYS, _IMAGES, _ANSWERS = {}, {}, {}, {}, {}


def _kd(points):
    p = np.ascontiguousarray(points, dtype=np.float32)
    return np.ascontiguousarray(p[foam_mod.kd_order(p)])


def extent(points):
    p = points.astype(np.float64)
    return float((p.max(0) - p.min(0)).max())


def _shifted(cloud):
    return cloud + SHIFT * extent(np.asarray(cloud))


def _uniform(rng, n=3000):
    return rng.uniform(-1, 1, size=(n, 3))


def lattice_points(shift=True):
    g = np.arange(-3, 4, dtype=np.float32) * np.float32(0.25)
    cloud = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return _kd(_shifted(cloud) if shift else cloud)


def _cloud(name):
    rng = np.random.default_rng(_SEED[name])
    if name in ("scaled_2p13", "scaled_2p14"):
        # one cloud, shifted before the scaling: the two foams differ by an exact factor of 2 in every coordinate
        base = _kd(_shifted(_uniform(np.random.default_rng(_SEED["scaled_2p13"]))))
        return base * np.float32(2.0 ** int(name[-2:]))
    if name == "hub":
        shell = rng.normal(size=(3000, 3))
        shell /= np.linalg.norm(shell, axis=1, keepdims=True)
        outside = rng.uniform(-3, 3, size=(4000, 3))
        outside = outside[np.linalg.norm(outside, axis=1) > 1.5]
        return _kd(_shifted(np.concatenate([shell * (1 + 1e-3 * rng.normal(size=(3000, 1))), np.zeros((1, 3)), outside])))
    if name == "clustered":
        return _kd(_shifted(np.concatenate([rng.normal(0, s, (800, 3)) + rng.uniform(-1, 1, 3)
                                            for s in (1.0, 0.3, 0.1, 0.01, 0.001)])))
    if name == "sheet":
        cloud = _uniform(rng)
        cloud[:, 2] *= 1e-4
        return _kd(_shifted(cloud))
    if name == "lattice":
        return lattice_points()
    if name == "translated":
        return _kd(_shifted(_uniform(rng)) + np.array([30000.0, -15000.0, 10000.0]))
    if name == "unbounded":
        far = rng.normal(size=(500, 3))
        far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(5, 3000, (500, 1))
        return _kd(_shifted(np.concatenate([rng.normal(0, 0.3, (2500, 3)), far])))
    if name == "near_duplicates":
        cloud = rng.uniform(-1, 1, size=(400, 3)).astype(np.float32)
        cloud[200:300] = cloud[100:200] + np.float32(1e-4)
        return _kd(_shifted(cloud))
    raise KeyError(name)


def edge_owner(fm):
    return np.repeat(np.arange(len(fm["points"])), np.diff(fm["point_adjacency_offsets"].astype(np.int64)))


def edge_offsets(fm):
    """Largest |component| of every face offset q - p, in float32 as the half table is built from."""
    p = fm["points"]
    return np.abs(p[fm["point_adjacency"].astype(np.int64)] - p[edge_owner(fm)]).max(1)


def overflowed_paddings(fm):
    """How many padding entries of the lists padded to four are written all-zero: entry j (1..3) of a list's last block
    is the block's first fp16 offset times 2^j, unless a component of that leaves fp16 (pad_offset, rf_kernels.hip)."""
    off = fm["point_adjacency_offsets"].astype(np.int64)
    deg = np.diff(off)
    p = fm["points"]
    count = 0
    for cell in np.flatnonzero(deg % 4):
        first = off[cell] + (deg[cell] & ~3)
        with np.errstate(over="ignore"):
            h = (p[fm["point_adjacency"][first]] - p[cell]).astype(np.float16).astype(np.float32)
            for j in range(deg[cell] % 4, 4):
                count += int(np.isinf((h * np.float32(1 << j)).astype(np.float16)).any())
    return count


def build(points, sh_degree, seed, tau=TAU):
    """Foam dict over kd-ordered float32 `points`: seeded normal(0, 0.3) colour coefficients, density tau / (mean distance
    to the cell's neighbours)."""
    rng = np.random.default_rng(seed)
    offsets, adjacency = foam_mod.delaunay_csr(points)
    fm = {"points": points, "point_adjacency": adjacency, "point_adjacency_offsets": offsets, "sh_degree": sh_degree}
    a = foam_mod.attribute_dim(sh_degree)
    attrs = rng.normal(0.0, 0.3, size=(len(points), a)).astype(np.float32)
    p = points.astype(np.float64)
    own = edge_owner(fm)
    dist = np.linalg.norm(p[adjacency.astype(np.int64)] - p[own], axis=1)
    mean = np.bincount(own, dist, len(p)) / np.maximum(np.bincount(own, minlength=len(p)), 1)
    attrs[:, -1] = (tau / mean).astype(np.float32)
    fm["attributes"] = attrs
    return fm


def points(name):
    if name not in _POINTS:
        _POINTS[name] = _cloud(name)
    return _POINTS[name]


def foam(name, sh_degree=None):
    d = DEGREE[name] if sh_degree is None else sh_degree
    if (name, d) not in _FOAMS:
        # the two scaled foams share their colours (and, the density rule being exact under a factor of 2, differ by
        # that factor in points and by its inverse in density, and in nothing else)
        seed = _SEED["scaled_2p13" if name == "scaled_2p14" else name]
        _FOAMS[name, d] = build(points(name), d, seed + 1000 * d, TAU_OF.get(name, TAU))
    return _FOAMS[name, d]


def hub_site(fm):
    return int(np.argmax(np.diff(fm["point_adjacency_offsets"].astype(np.int64))))


def exact_starts(pts, origins):
    from scipy.spatial import cKDTree

    return cKDTree(pts.astype(np.float64)).query(origins.astype(np.float64))[1].astype(np.uint32)


def make_rays(fm, n, seed, aim=None, axis_from_sites=0):
    """n rays: half the origins within 1e-3 extents of a random site, half one extent from the centre of the bounding box
    (outside it), all aimed at random sites (or, for every other ray, at site `aim`) with a jitter of 1e-2 extents; every
    fourth direction is scaled by 0.5 to 2.  `axis_from_sites` of the rays, anywhere in the batch, start exactly on a site
    and run exactly along an axis instead, towards the centre plane and across it.  Start cells are the exact nearest
    sites."""
    rng = np.random.default_rng(seed)
    p = fm["points"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    centre, ext = (lo + hi) / 2, (hi - lo).max()
    o = np.empty((n, 3))
    o[: n // 2] = p[rng.integers(0, len(p), n // 2)] + rng.normal(0, 1e-3 * ext, (n // 2, 3))
    out = rng.normal(size=(n - n // 2, 3))
    o[n // 2:] = centre + out / np.linalg.norm(out, axis=1, keepdims=True) * ext * rng.uniform(0.95, 1.05, (n - n // 2, 1))
    target = p[rng.integers(0, len(p), n)]
    if aim is not None:
        target[::2] = p[aim]
    o32 = o.astype(np.float32)
    d = target - o32 + rng.normal(0, 1e-2 * ext, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::4] *= rng.uniform(0.5, 2.0, size=(len(d[::4]), 1))
    k = axis_from_sites
    if k:
        which = rng.permutation(n)[:k]       # spread over both halves, whatever the order of the batch
        o32[which] = fm["points"][rng.integers(0, len(p), k)]
        axis = rng.integers(0, 3, k)
        side = np.sign(o32[which, axis] - centre[axis].astype(np.float32))       # towards and across the centre plane
        side = np.where(np.abs(o32[which, axis] - centre[axis]) < 1e-3 * ext, rng.choice([-1.0, 1.0], k), -side)
        d[which] = np.eye(3)[axis] * side[:, None]
    r = np.concatenate([o32, d.astype(np.float32)], axis=1).astype(np.float32)
    return r, exact_starts(fm["points"], r[:, :3])


def rays(name):
    if name not in _RAYS:
        fm = foam(name)
        _RAYS[name] = make_rays(fm, NUM_RAYS, _SEED[name] + 50, aim=hub_site(fm) if name == "hub" else None,
                                axis_from_sites=NUM_RAYS // 2 if name == "lattice" else 0)
    return _RAYS[name]


def image(name):
    """64x48 pinhole frame from two extents off the centre of the bounding box, aimed at it."""
    if name not in _IMAGES:
        p = points(name).astype(np.float64)
        centre, ext = (p.min(0) + p.max(0)) / 2, extent(p)
        back = np.array([0.3, 0.2, -1.0])
        back /= np.linalg.norm(back)
        cam = foam_mod.default_camera(64, 48)
        fwd = -back
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        cam["position"] = (centre + 2.0 * ext * back).astype(np.float32)
        cam["forward"], cam["right"] = fwd.astype(np.float32), right.astype(np.float32)
        cam["up"] = np.cross(fwd, right).astype(np.float32)
        r = foam_mod.camera_rays(cam)
        start = foam_mod.nearest_point(points(name), cam["position"])
        _IMAGES[name] = (r, np.full(r.shape[:-1], start, dtype=np.uint32), cam)
    return _IMAGES[name][:2]


def camera(name):
    image(name)
    return _IMAGES[name][2]


def _args(fm):
    return (fm["sh_degree"], fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])


def _cached(kind, name, make):
    if (kind, name) not in _ANSWERS:
        _ANSWERS[kind, name] = make()
    return _ANSWERS[kind, name]


def upstream(name):
    """Seeded inputs of the flat batch's forward and backward: two depth quantiles per ray (descending), their upstream
    gradient, the rgba gradient and ray_error."""
    def make():
        rng = np.random.default_rng(_SEED[name] + 70)
        q = np.sort(rng.uniform(0.02, 0.98, size=(NUM_RAYS, 2)).astype(np.float32), axis=1)[:, ::-1].copy()
        return {"q": q, "dg": rng.normal(size=(NUM_RAYS, 2)).astype(np.float32),
                "g": rng.normal(size=(NUM_RAYS, 4)).astype(np.float32),
                "err": rng.uniform(0, 1, size=NUM_RAYS).astype(np.float32)}
    return _cached("upstream", name, make)


def _backward(O, name, fm, r, s, fwd, u):
    kw = {}
    if name in QUANTILE_GRADS:
        kw = dict(depth_quantiles=u["q"], depth_indices=fwd["depth_indices"], depth_grad_in=u["dg"])
    return O.trace_backward(*_args(fm), r, s, fwd["rgba"], u["g"], ray_error=u["err"], num_threads=1, **kw)


def flat(name):
    """The oracle's literal reference scan on the flat batch: {"fwd": trace_forward with two quantiles and contribution,
    "bwd": trace_backward on one thread with ray_error (and quantile gradients for QUANTILE_GRADS)}."""
    def make():
        from oracle import oracle as O

        fm, (r, s), u = foam(name), rays(name), upstream(name)
        fwd = O.trace_forward(*_args(fm), r, s, depth_quantiles=u["q"], return_contribution=True, num_threads=1)
        return {"fwd": fwd, "bwd": _backward(O, name, fm, r, s, fwd, u)}
    return _cached("flat", name, make)


def mirror(name):
    """The same through scan_mode("filtered"), the mirror of the kernels' evaluation, and its statistics."""
    def make():
        from oracle import oracle as O

        fm, (r, s), u = foam(name), rays(name), upstream(name)
        with O.scan_mode("filtered") as m:
            fwd = O.trace_forward(*_args(fm), r, s, depth_quantiles=u["q"], return_contribution=True, num_threads=1)
            contested = m.contested
            bwd = _backward(O, name, fm, r, s, fwd, u)
        return {"fwd": fwd, "bwd": bwd, "contested": contested}
    return _cached("mirror", name, make)


def noise(name):
    """The oracle's one-thread backward with the rays in another order: the summation-order noise of the reference."""
    def make():
        from oracle import oracle as O

        fm, (r, s), u = foam(name), rays(name), upstream(name)
        fwd = flat(name)["fwd"]
        perm = np.random.default_rng(_SEED[name] + 90).permutation(NUM_RAYS)
        pf = {k: v[perm] for k, v in fwd.items() if k != "contribution"}
        return _backward(O, name, fm, r[perm], s[perm], pf, {k: v[perm] for k, v in u.items()})
    return _cached("noise", name, make)


def frame(name):
    """The oracle's forward on image(name)."""
    def make():
        from oracle import oracle as O

        r, s = image(name)
        return O.trace_forward(*_args(foam(name)), r, s)
    return _cached("frame", name, make)


def _half_inputs(name):
    fm = dict(foam(name))
    fm["attributes"] = fm["attributes"].astype(np.float16)
    return fm, rays(name), upstream(name)


def half_forward(name):
    """(foam with fp16 attributes, the oracle's fp16 forward on the flat batch: two quantiles and contribution)."""
    def make():
        from oracle import oracle as O

        fm, (r, s), u = _half_inputs(name)
        return fm, O.trace_forward(*_args(fm), r, s, depth_quantiles=u["q"], return_contribution=True, num_threads=1)
    return _cached("half_forward", name, make)


def half(name):
    """helpers.half_reference on the flat batch with fp16 attributes, upstream gradient and ray_error."""
    def make():
        from tests import helpers as H

        fm, (r, s), u = _half_inputs(name)
        quant = name in QUANTILE_GRADS
        return H.half_reference(fm["sh_degree"], fm, r, s, u["q"] if quant else None, u["dg"] if quant else None,
                                u["g"].astype(np.float16), u["err"].astype(np.float16))
    return _cached("half", name, make)


def segments(name):
    """segments_ref.oracle_segments of the flat batch."""
    def make():
        from tests import segments_ref as S

        r, s = rays(name)
        return S.oracle_segments(foam(name), r, s)
    return _cached("segments", name, make)


def origin_case():
    """The lattice WITHOUT its shift -- one site is exactly (0, 0, 0) -- and 512 rays that start in that site's cell."""
    def make():
        from oracle import oracle as O

        pts = lattice_points(shift=False)
        site = int(np.flatnonzero((pts == 0).all(1))[0])
        fm = build(pts, 1, 7)
        rng = np.random.default_rng(8)
        o = rng.uniform(-0.1, 0.1, size=(512, 3)).astype(np.float32)       # the cell is the cube of half-side 0.125
        d = rng.normal(size=(512, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = np.concatenate([o, d.astype(np.float32)], axis=1)
        s = exact_starts(pts, o)
        assert (s == site).all()
        g = rng.normal(size=(512, 4)).astype(np.float32)
        fwd = O.trace_forward(*_args(fm), r, s, num_threads=1)
        bwd = O.trace_backward(*_args(fm), r, s, fwd["rgba"], g, num_threads=1)
        return {"fm": fm, "site": site, "rays": r, "starts": s, "g": g, "fwd": fwd, "bwd": bwd}
    return _cached("origin", "lattice", make)
