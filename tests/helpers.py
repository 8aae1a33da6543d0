"""Shared helpers for the parity tests (CPU oracle vs HIP path on identical seeded inputs)."""
import numpy as np

from radfoam_amd import foam as foam_mod


def camera_setup(fm, width, height, position=(0.0, 0.0, -3.0)):
    cam = foam_mod.default_camera(width, height)
    cam["position"] = np.asarray(position, dtype=np.float32)
    rays = foam_mod.camera_rays(cam)
    start = foam_mod.nearest_point(fm["points"], cam["position"])
    return cam, rays, np.uint32(start)


def random_rays(fm, n_rays, seed):
    """Incoherent rays from a few origins inside/outside the foam, with their entry cells."""
    rng = np.random.default_rng(seed)
    origins = np.array([[0.0, 0.0, -3.0], [2.5, 0.3, 0.2], [0.05, -0.02, 0.01], [-0.4, 0.5, 0.3]], dtype=np.float32)
    starts = np.array([foam_mod.nearest_point(fm["points"], o) for o in origins], dtype=np.uint32)
    which = rng.integers(0, len(origins), size=n_rays)
    target = rng.uniform(-0.7, 0.7, size=(n_rays, 3)).astype(np.float32)
    d = target - origins[which]
    d = d * rng.uniform(0.5, 2.0, size=(n_rays, 1)).astype(np.float32)  # un-normalised on purpose
    rays = np.concatenate([origins[which], d.astype(np.float32)], axis=1).astype(np.float32)
    return rays, starts[which]


def to_torch_foam(fm, device, attr_dtype=None):
    import torch

    attrs = torch.from_numpy(fm["attributes"])
    if attr_dtype is not None:
        attrs = attrs.to(attr_dtype)
    return (
        torch.from_numpy(fm["points"]).to(device),
        attrs.to(device),
        torch.from_numpy(fm["point_adjacency"]).to(device),
        torch.from_numpy(fm["point_adjacency_offsets"]).to(device),
    )


def half_backward_case(foam_factory, d, seed, image, quantiles, with_error, n_points=5000, width=80, height=56,
                       n_rays=4000):
    """One fp16 forward+backward case with the CPU oracle's answers, computed once (num_threads=1) and shared.

    Inputs: the foam's attributes, the upstream rgba gradient (normal(0,1)) and ray_error (uniform(0,1)) are fp16;
    points, rays, quantiles and depth_grad are fp32; rgb_out is the oracle's own fp16 forward result.
    `fwd` / `bwd` are the oracle in fp16 mode.  `fwd32` / `bwd32` are its fp32 mode on the same fp16 values widened
    to fp32 -- what an fp32 accumulator of an fp16 kernel holds before its single rounding."""
    fm = dict(foam_factory(n_points, d, seed))
    fm["attributes"] = fm["attributes"].astype(np.float16)
    rng = np.random.default_rng(seed)
    if image:
        cam, rays, start = camera_setup(fm, width, height)
        starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
    else:
        rays, starts = random_rays(fm, n_rays, seed=seed + 1)
    batch = rays.shape[:-1]
    q = dg = None
    if quantiles:
        q = np.sort(rng.uniform(0.02, 0.98, size=batch + (2,)).astype(np.float32), axis=-1)[..., ::-1].copy()
        dg = rng.normal(size=batch + (2,)).astype(np.float32)
    g = rng.normal(0, 1, size=batch + (4,)).astype(np.float16)
    err = rng.uniform(0, 1, size=batch).astype(np.float16) if with_error else None
    return half_reference(d, fm, rays, starts, q, dg, g, err)


def half_reference(d, fm, rays, starts, q, dg, g, err):
    """The oracle's answers for one fp16 case (see half_backward_case), one thread."""
    from oracle import oracle as O

    assert fm["attributes"].dtype == np.float16 and g.dtype == np.float16 and (err is None or err.dtype == np.float16)
    wide = lambda x: None if x is None else x.astype(np.float32)
    topo = (fm["point_adjacency"], fm["point_adjacency_offsets"])
    a16 = (d, fm["points"], fm["attributes"]) + topo
    a32 = (d, fm["points"], wide(fm["attributes"])) + topo
    fwd = O.trace_forward(*a16, rays, starts, depth_quantiles=q, return_contribution=True, num_threads=1)
    fwd32 = O.trace_forward(*a32, rays, starts, depth_quantiles=q, return_contribution=True, num_threads=1)
    kw = dict(depth_quantiles=q, depth_indices=fwd.get("depth_indices"), depth_grad_in=dg, num_threads=1)
    bwd = O.trace_backward(*a16, rays, starts, fwd["rgba"], g, ray_error=err, **kw)
    bwd32 = O.trace_backward(*a32, rays, starts, wide(fwd["rgba"]), wide(g), ray_error=wide(err), **kw)
    return {"d": d, "fm": fm, "rays": rays, "starts": starts, "q": q, "dg": dg, "g": g, "err": err,
            "fwd": fwd, "fwd32": fwd32, "bwd": bwd, "bwd32": bwd32}


def _half_order(x):
    """fp16 values as integers ordered like the values (sign-magnitude -> signed; +0 and -0 coincide)."""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float16, x.dtype
    bits = x.view(np.uint16).astype(np.int32)
    mag = bits & 0x7FFF
    return np.where(bits & 0x8000, -mag, mag)


def half_step_check(got, ref, max_share=0.01):
    """The "one fp16 step" rule for fp16 outputs rounded once from fp32 sums whose order differs: both arrays
    finite, every element of `got` is the reference's fp16 value or one of its two fp16 neighbours, and at most
    `max_share` of the reference's non-zero elements differ at all.  The share is a cap, not a measurement: a flip
    needs the fp32 sum within ~1e-7 relative of a rounding boundary whose spacing is ~1e-3 relative, so ~1e-4 is
    expected.  Returns (ok, message)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == np.float16 and ref.dtype == np.float16 and got.shape == ref.shape, (got.dtype, ref.dtype)
    finite = bool(np.isfinite(got).all() and np.isfinite(ref).all())
    dist = np.abs(_half_order(got) - _half_order(ref))
    nz = max(int((ref != 0).sum()), 1)
    share = float((dist != 0).sum()) / nz
    worst = int(dist.max()) if dist.size else 0
    ok = finite and worst <= 1 and share <= max_share
    return ok, "finite=%s, largest fp16 distance %d, share of non-zero elements that differ %.3g (cap %.3g)" % (
        finite, worst, share, max_share)


def grad_close(got, ref, rtol=1e-3):
    """Gradient parity bound of the north star (1e-3 relative): every element within
    rtol*|ref| + rtol*rms(ref) (the second term absorbs summation-order noise on elements that
    are sums of cancelling contributions); also returns the global relative L2 error."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    nz = ref[ref != 0]
    rms = np.sqrt(np.mean(nz ** 2)) if nz.size else 0.0
    err = np.abs(got - ref)
    bound = rtol * np.abs(ref) + rtol * rms
    rel_l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    return bool((err <= bound).all()), float(rel_l2), float((err / np.maximum(bound, 1e-30)).max())
