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
                       n_rays=4000, return_magnitude=False):
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
    return half_reference(d, fm, rays, starts, q, dg, g, err, return_magnitude=return_magnitude)


def half_reference(d, fm, rays, starts, q, dg, g, err, return_magnitude=False):
    """The oracle's answers for one fp16 case (see half_backward_case), one thread.  return_magnitude: `bwd` and `bwd32`
    carry the magnitude of every gradient element as well (oracle.trace_backward)."""
    from oracle import oracle as O

    assert fm["attributes"].dtype == np.float16 and g.dtype == np.float16 and (err is None or err.dtype == np.float16)
    wide = lambda x: None if x is None else x.astype(np.float32)
    topo = (fm["point_adjacency"], fm["point_adjacency_offsets"])
    a16 = (d, fm["points"], fm["attributes"]) + topo
    a32 = (d, fm["points"], wide(fm["attributes"])) + topo
    fwd = O.trace_forward(*a16, rays, starts, depth_quantiles=q, return_contribution=True, num_threads=1)
    fwd32 = O.trace_forward(*a32, rays, starts, depth_quantiles=q, return_contribution=True, num_threads=1)
    kw = dict(depth_quantiles=q, depth_indices=fwd.get("depth_indices"), depth_grad_in=dg, num_threads=1)
    if return_magnitude:
        kw["return_magnitude"] = True
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


def grad_close_elements(got, ref, mag, k, extra_rel=0.0, extra_abs=0.0):
    """Per-element gradient parity, each element on its own scale.

    `mag[i]` is the sum of |addend| over everything the oracle adds into element i (oracle.trace_backward(...,
    return_magnitude=True)): rounding and the order of the sum can move the element by a few 2^-24 * mag[i] and no
    more, whatever the rest of the tensor holds.  Requires |got - ref| <= k * 2^-24 * mag + (2^-22 + extra_rel) * |ref|
    on every element, and got == 0 exactly where mag == 0 (nothing was added there).  `extra_rel` and `extra_abs` are for
    an output rounded once more on its way out: an fp16 output of an fp32 sum is half an fp16 step from it, 2^-11 relative
    for a normal half and 2^-25 absolute among the subnormal ones (|x| < 2^-14), where the step no longer shrinks with x;
    `extra_abs` is added to the bound of the touched elements only.

    Returns (ok, worst_ratio, index_of_worst): worst_ratio is the largest |got - ref| / (2^-24 * mag) over the touched
    elements (inf if an untouched element is not 0, nan counts as inf), index_of_worst its index as a tuple."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    mag = np.asarray(mag, dtype=np.float64)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    touched = mag != 0
    err = np.abs(got - ref)
    bound = k * 2.0 ** -24 * mag + (2.0 ** -22 + extra_rel) * np.abs(ref) + np.where(touched, extra_abs, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(touched, err / (2.0 ** -24 * mag), np.where(got == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    ok = bool((err <= bound).all()) and bool((got[~touched] == 0).all())
    if ratio.size == 0:
        return ok, 0.0, ()
    flat = int(np.argmax(ratio))
    return ok, float(ratio.reshape(-1)[flat]), tuple(int(i) for i in np.unravel_index(flat, ratio.shape))


GRAD_TENSORS = ("points_grad", "attr_grad", "point_error")


def element_k(k0):
    """The k of grad_close_elements for a case whose oracle, run with the rays in reverse order, differs from itself by
    k0 (a worst_ratio): 4 * max(k0, 4).  The 4 inside is the floor for cases whose reordering happens to be quiet; the
    4 outside is for a kernel addend that differs from the oracle's by a rounding or two of its own (a contracted
    multiply-add, the divide sequence, partial sums held in double and rounded once), which no reordering shows."""
    return 4.0 * max(float(k0), 4.0)


def oracle_backward_elements(d, fm, rays, starts, g, q=None, dg=None, err=None, fwd=None, **settings):
    """The oracle's forward and backward (one thread) with the magnitude of every gradient element, and k0: the largest
    worst_ratio, over the gradient tensors, of the same backward with the rays in reverse order against it.  Inputs of
    any batch shape; fp16 attributes / g / err select the oracle's fp16 mode.  Returns (fwd, ref, k0, k0_by_tensor)."""
    from oracle import oracle as O

    args = (d, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    if fwd is None:
        fwd = O.trace_forward(*args, rays, starts, depth_quantiles=q, num_threads=1, **settings)
    ref = O.trace_backward(*args, rays, starts, fwd["rgba"], g, depth_quantiles=q, depth_indices=fwd.get("depth_indices"),
                           depth_grad_in=dg, ray_error=err, num_threads=1, return_magnitude=True, **settings)
    n = int(np.prod(rays.shape[:-1]))
    rev = lambda x, w: None if x is None else np.ascontiguousarray(np.asarray(x).reshape((n,) + w)[::-1])
    nq = 0 if q is None else q.shape[-1]
    back = O.trace_backward(*args, rev(rays, (6,)), rev(np.broadcast_to(starts, rays.shape[:-1]), ()),
                            rev(fwd["rgba"], (4,)), rev(g, (4,)), depth_quantiles=rev(q, (nq,)),
                            depth_indices=rev(fwd.get("depth_indices"), (nq,)), depth_grad_in=rev(dg, (nq,)),
                            ray_error=rev(err, ()), num_threads=1, **settings)
    k0s = {}
    for key in GRAD_TENSORS:
        if key in ref:
            fin = np.isfinite(ref[key].astype(np.float64)) & np.isfinite(ref[key + "_mag"])
            pick = lambda x: np.where(fin, x, 0.0)
            k0s[key] = grad_close_elements(pick(back[key]), pick(ref[key]), pick(ref[key + "_mag"]), 0.0)[1]
    return fwd, ref, max(k0s.values()), k0s


def backward_case(foam_factory, d, seed, image, quantiles, with_error, n_points=5000):
    """The inputs of tests/test_gpu_parity.py::_backward_case, value for value (same foam, rays and draws from the same
    generator in the same order), with the oracle's answers from oracle_backward_elements.  Returns a dict."""
    fm = foam_factory(n_points, d, seed)
    rng = np.random.default_rng(seed)
    if image:
        cam, rays, start = camera_setup(fm, 80, 56)
        starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
    else:
        rays, starts = random_rays(fm, 4000, seed=seed + 1)
    batch = rays.shape[:-1]
    q = dg = None
    if quantiles:
        q = np.sort(rng.uniform(0.02, 0.98, size=batch + (2,)).astype(np.float32), axis=-1)[..., ::-1].copy()
        dg = rng.normal(size=batch + (2,)).astype(np.float32)
    g = rng.normal(size=batch + (4,)).astype(np.float32)
    err = rng.uniform(0, 1, size=batch).astype(np.float32) if with_error else None
    fwd, ref, k0, k0s = oracle_backward_elements(d, fm, rays, starts, g, q, dg, err)
    return {"d": d, "fm": fm, "rays": rays, "starts": starts, "q": q, "dg": dg, "g": g, "err": err, "fwd": fwd,
            "ref": ref, "k0": k0, "k0_by_tensor": k0s, "settings": {}}


def cell_list_lengths(k):
    """Entries per cell, in cell order, for the kernels that sweep a walk by cell in chunks of k positions.  With K the
    chunk: 0, 1, 63, 64, 65, K-1, K, K+1 and 2K+130 all occur; cell 7 ends exactly on a chunk boundary and cell 8, of K
    entries, begins and ends on one; cell 10 begins one position behind a boundary, so the chunk after that lies wholly
    inside it; cells are empty at both ends and in the middle; the total is no multiple of 64."""
    lengths = [0, 1, 63, 64, 65, 0, k - 1]
    lengths.append(k - sum(lengths) % k)                           # cell 7: up to the next boundary
    assert sum(lengths) % k == 0 and lengths[7] > 0
    lengths += [k, k + 1, 2 * k + 130, 7, 0, 0]
    begin = sum(lengths[:10])
    assert begin % k == 1 and (begin + lengths[10]) // k - begin // k == 2 and sum(lengths) % 64 != 0
    return lengths


def cell_list_lengths_long(k):
    """cell_list_lengths, then one list of 70 chunks, more than the boundary launch adds in one step, and an empty cell
    behind it."""
    lengths = cell_list_lengths(k) + [70 * k + 5, 0]
    assert sum(lengths) % 64 != 0
    return lengths
