"""-m gpu: the empty-run memo of the image backward (backward_replay_cached_kernel, backward_mode 3; TrailWalker::step).

A ray keeps dL/dalpha of its last segment through a cell of density exactly 0 and reuses it while it stays in such cells;
a wave-step whose every segment is of that kind skips the functor.  backward_mode 5 is mode 3 with the full functor on
every segment.  The foam: 20,000 uniform points in [-1,1]^3, SH 2, fp32; density exactly 0 outside r = 0.8 and in the
shell 0.3 < r < 0.5, uniform(0.4, 0.6) elsewhere, every 16th lit cell 5e-7 (0 < s <= 1e-6: no colour, but alpha != 0).
Camera at (0, 0, -3) looking at +z.  The bars are the project's: helpers.grad_close (1e-3 per element) and relative L2
below 1e-5; single rays (one lane, one order of adds) bit for bit.
"""
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 2
N_POINTS, SEED = 20000, 91
TINY = np.float32(5e-7)
_FOAMS, _CASES, _WALKS = {}, {}, {}


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _foam(foam_factory, kind="shells"):
    """kind "shells": the density pattern above; "no-zero": the same with max(density, 4.5e-6), no exact zero left."""
    if kind not in _FOAMS:
        fm = dict(foam_factory(N_POINTS, D, SEED))
        r = np.linalg.norm(fm["points"].astype(np.float64), axis=1)
        rng = np.random.default_rng(SEED + 1)
        dens = rng.uniform(0.4, 0.6, size=N_POINTS).astype(np.float32)
        dens[(r > 0.8) | ((r > 0.3) & (r < 0.5))] = 0.0
        lit = np.flatnonzero(dens > 0)
        dens[lit[::16]] = TINY
        if kind == "no-zero":
            dens = np.maximum(dens, np.float32(4.5e-6))
        fm["attributes"] = fm["attributes"].copy()
        fm["attributes"][:, -1] = dens
        _FOAMS[kind] = fm
    return _FOAMS[kind]


def _case(foam_factory, side, kind="shells", quantiles=False, bad_pixels=False, **settings):
    """Frame, upstream gradients and the oracle's answers (one thread), computed once and never modified."""
    key = (side, kind, quantiles, bad_pixels, tuple(sorted(settings.items())))
    if key not in _CASES:
        fm = _foam(foam_factory, kind)
        cam, rays, start = H.camera_setup(fm, side, side)
        starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
        rng = np.random.default_rng(SEED + side)
        g = rng.normal(size=rays.shape[:-1] + (4,)).astype(np.float32)
        q = dg = None
        if quantiles:
            q = np.sort(rng.uniform(0.02, 0.98, size=rays.shape[:-1] + (2,)).astype(np.float32), axis=-1)[..., ::-1].copy()
            dg = rng.normal(size=rays.shape[:-1] + (2,)).astype(np.float32)
        c = dict(fm=fm, rays=rays, starts=starts, g=g, q=q, dg=dg, settings=settings)
        args = (D, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
        fwd = O.trace_forward(*args, rays, starts, depth_quantiles=q, num_threads=1, **settings)
        c["fwd"] = fwd
        if bad_pixels:
            # no oracle for these: the two modes are compared with one another
            c["g"] = g.copy()
            c["g"][side // 2, side // 2, 1] = np.inf
            c["g"][side // 4, side // 2, 3] = np.nan
        else:
            c["bwd"] = O.trace_backward(*args, rays, starts, fwd["rgba"], g, depth_quantiles=q,
                                        depth_indices=fwd.get("depth_indices"), depth_grad_in=dg, num_threads=1, **settings)
        _CASES[key] = c
    return _CASES[key]


def _pipeline(mode):
    import radfoam

    pipe = radfoam.create_pipeline(D)
    pipe.record_trail = True
    pipe.backward_mode = mode
    return pipe


def _run(c, mode, pixel=None):
    """Forward (records the trail) and image backward in `mode` on one pipeline; pixel = (row, col): that ray alone, as
    a 1x1 frame.  The forward is checked bit for bit against the oracle."""
    pipe = _pipeline(mode)
    p, a, adj, off = H.to_torch_foam(c["fm"], DEV)
    sel = (slice(None), slice(None)) if pixel is None else (slice(pixel[0], pixel[0] + 1), slice(pixel[1], pixel[1] + 1))
    cut = lambda x: None if x is None else _t(x[sel])
    tr, ts, tq = cut(c["rays"]), cut(c["starts"]), cut(c["q"])
    f = pipe.trace_forward(p, a, adj, off, tr, ts, depth_quantiles=tq, **c["settings"])
    np.testing.assert_array_equal(f["rgba"].cpu().numpy().view(np.uint32), c["fwd"]["rgba"][sel].view(np.uint32))
    assert pipe._trail is not None
    out = pipe.trace_backward(p, a, adj, off, tr, ts, f["rgba"], cut(c["g"]), tq, cut(c["fwd"].get("depth_indices")),
                              cut(c["dg"]), **c["settings"])
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("points_grad", "attr_grad")}


def _check(got, ref, what=""):
    for key in ("points_grad", "attr_grad"):
        print(what, key, "grad_close / rel L2 / worst element of its bound:", H.grad_close(got[key], ref[key]))
    for key in ("points_grad", "attr_grad"):
        ok, rel, worst = H.grad_close(got[key], ref[key])
        assert ok and rel < 1e-5, (what, key, rel, worst)
        assert np.abs(ref[key]).max() > 0


def _walks(foam_factory, side, kind="shells"):
    """Per ray of the side x side frame, the kinds of the segments the backward composites, in order, from the exported
    walk: E = density exactly 0, T = 0 < density <= 1e-6, L = lit.  (An entry with t_exit <= t_enter is no segment, and
    the walk's last cell has no exit.)"""
    if (side, kind) not in _WALKS:
        c = _case(foam_factory, side, kind)
        pipe = _pipeline(3)
        p, a, adj, off = H.to_torch_foam(c["fm"], DEV)
        s = pipe.trace_segments(p, a, adj, off, _t(c["rays"]), _t(c["starts"]))
        offsets, cells = s["offsets"].cpu().numpy(), s["cells"].cpu().numpy().astype(np.int64)
        t_enter, t_exit = s["t_enter"].cpu().numpy(), s["t_exit"].cpu().numpy()
        dens = c["fm"]["attributes"][:, -1]
        kinds = np.where(dens[cells] == 0, "E", np.where(dens[cells] <= 1e-6, "T", "L"))
        real = (t_exit > t_enter) & np.isfinite(t_exit)
        _WALKS[side, kind] = ["".join(kinds[a0:a1][real[a0:a1]]) for a0, a1 in zip(offsets[:-1], offsets[1:])]
    return _WALKS[side, kind]


_PATTERNS = {
    "an empty run of at least three segments before the first lit segment": r"^E{3,}[ET]*L",
    "empty -> lit -> empty -> lit": r"EL+E+L",
    "an empty run interrupted by a 5e-7 cell": r"ETE",
    "a ray that ends inside an empty run": r"[LT]EE+$",
}


def _rays_with(walks, pattern):
    return [i for i, w in enumerate(walks) if re.search(pattern, w)]


def test_the_rays_hold_every_pattern(foam_factory):
    """Not vacuous: the rays of the 64x64 frame contain each pattern the memo has to get right."""
    walks = _walks(foam_factory, 64)
    for what, pattern in _PATTERNS.items():
        n = len(_rays_with(walks, pattern))
        print(what, n, "rays")
        assert n > 0, what


def _eight_pixels(foam_factory, kind="shells"):
    """Two rays of the 64x64 frame per pattern (the first and the last that has it)."""
    walks = _walks(foam_factory, 64, kind)
    picked = []
    for pattern in _PATTERNS.values():
        rays = [i for i in _rays_with(walks, pattern) if i not in picked]
        assert len(rays) >= 2, pattern
        picked += [rays[0], rays[-1]]
    assert len(set(picked)) == 8
    return [(i // 64, i % 64) for i in picked]


def _assert_bitwise(c, pixels):
    for px in pixels:
        memo, full = _run(c, 3, px), _run(c, 5, px)
        for key in ("points_grad", "attr_grad"):
            assert np.abs(full[key]).max() > 0, (px, key)
            np.testing.assert_array_equal(memo[key].view(np.uint32), full[key].view(np.uint32), err_msg=str((px, key)))


def test_single_rays_bitwise(foam_factory):
    """One ray per launch, one lane, one order of adds: the memo's contributions are the full functor's, bit for bit."""
    _assert_bitwise(_case(foam_factory, 64), _eight_pixels(foam_factory))


@pytest.mark.parametrize("side", [16, 64])
def test_frames(foam_factory, side):
    """Lanes of one wave in empty and lit cells at once, the path switching per wave-step."""
    c = _case(foam_factory, side)
    memo, full = _run(c, 3), _run(c, 5)
    _check(memo, full, "memo against full functor, %d" % side)
    _check(memo, c["bwd"], "memo against the oracle, %d" % side)
    _check(full, c["bwd"], "full functor against the oracle, %d" % side)


def test_two_depth_quantiles(foam_factory):
    c = _case(foam_factory, 16, quantiles=True)
    assert np.abs(c["dg"]).max() > 0
    memo, full = _run(c, 3), _run(c, 5)
    _check(memo, full, "quantiles, memo against full functor")
    _check(memo, c["bwd"], "quantiles, memo against the oracle")


def test_weight_threshold_zero(foam_factory):
    """T runs into the subnormals where nothing cuts the ray off (div3_guarded's case)."""
    c = _case(foam_factory, 16, weight_threshold=0.0)
    memo, full = _run(c, 3), _run(c, 5)
    _check(memo, full, "threshold 0, memo against full functor")
    _check(memo, c["bwd"], "threshold 0, memo against the oracle")


def test_nonfinite_upstream_gradients(foam_factory):
    """One upstream pixel inf, one NaN: a non-finite dL/dalpha never becomes a memo, so both modes poison the same
    entries and agree on the others."""
    c = _case(foam_factory, 16, bad_pixels=True)
    assert np.isinf(c["g"]).sum() == 1 and np.isnan(c["g"]).sum() == 1
    memo, full = _run(c, 3), _run(c, 5)
    for key in ("points_grad", "attr_grad"):
        bad = ~np.isfinite(full[key])
        assert bad.any() and not bad.all(), key
        np.testing.assert_array_equal(~np.isfinite(memo[key]), bad, err_msg=key)
    fin = lambda out: {k: np.where(np.isfinite(full[k]), out[k], 0.0) for k in out}
    _check(fin(memo), fin(full), "non-finite pixels, the finite entries")


def test_foam_without_an_exact_zero(foam_factory):
    """max(density, 4.5e-6): the memo never becomes valid, and nothing depends on it."""
    c = _case(foam_factory, 64, kind="no-zero")
    assert (c["fm"]["attributes"][:, -1] > 0).all()
    walks = _walks(foam_factory, 64, "no-zero")
    assert not any("E" in w for w in walks)
    lit = [i for i, w in enumerate(walks) if "L" in w]
    _assert_bitwise(c, [(i // 64, i % 64) for i in lit[::max(len(lit) // 8, 1)][:8]])
    memo, full = _run(c, 3), _run(c, 5)
    _check(memo, full, "no exact zero, memo against full functor")
    _check(memo, c["bwd"], "no exact zero, memo against the oracle")
