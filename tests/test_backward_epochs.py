"""-m gpu: the image backward's flush epochs (backward_replay_cached_kernel, backward_mode 3).  The block's epoch gets
longer while its table holds only a few density-only rows and falls back to the short length when colour or point
gradients arrive (radfoam_amd/csrc/rf_epoch.hpp); whatever lengths a frame produces, the gradients are the oracle's and
those of backward_mode 2 (no cache) on the same call.

A 48x32 frame is six 16x16 blocks; the foam has 20,000 points.  Cases:
  ball    a lit ball of radius 0.25 in a shell of density exactly 0, camera outside: long empty runs before and behind
          the ball, a lit phase in the middle, tiles at the frame's edge that never see the ball;
  lit     every cell lit (densities of at least 4.5e-6): wide rows all the way, the epoch never lengthens;
  inside  camera inside a four times denser foam with weight_threshold = 0: every ray runs to the hull, the rays of a block
          differ in length, waves finish epochs apart and the table is under pressure;
  ragged  a 43x27 frame: partly empty blocks and waves.

Bars: those of tests/test_gpu_parity.py for scatter outputs -- 1e-3 per element (helpers.grad_close) and a relative L2
below 1e-5 -- against the oracle and against backward_mode 2.

Measured on the MI355X over the ten cases: relative L2 at most 1.4e-6 (inside, SH 0, points_grad against the oracle), worst
element 0.015 of its bound; the file runs in under 5 s."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_POINTS = 20000
CASES = {
    # name: (seed, width, height, camera position, weight_threshold or None for the default)
    "ball": (101, 48, 32, (0.0, 0.0, -3.0), None),
    "lit": (102, 48, 32, (0.0, 0.0, -3.0), None),
    "inside": (103, 48, 32, (-0.4, 0.5, -0.3), 0.0),
    "ragged": (104, 43, 27, (0.0, 0.0, -3.0), None),
}
_REF = {}


def _case(foam_factory, name, d):
    """The foam, rays and upstream gradient of a case and the oracle's gradients, computed once"""
    if (name, d) in _REF:
        return _REF[(name, d)]
    seed, width, height, position, threshold = CASES[name]
    fm = dict(foam_factory(N_POINTS, d, seed))
    fm["attributes"] = fm["attributes"].copy()
    dens = fm["attributes"][:, -1]
    if name == "ball":
        dens[np.linalg.norm(fm["points"].astype(np.float64), axis=1) > 0.25] = 0.0
        assert 50 < int((dens > 0).sum()) < N_POINTS // 20
    elif name == "lit":
        np.maximum(dens, np.float32(4.5e-6), out=dens)
        assert (dens > 0).all()
    elif name == "inside":
        dens *= np.float32(4.0)
    cam, rays, start = H.camera_setup(fm, width, height, position)
    starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
    g = np.random.default_rng(seed).normal(size=rays.shape[:-1] + (4,)).astype(np.float32)
    kw = {} if threshold is None else {"weight_threshold": threshold}
    args = (d, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    fwd = O.trace_forward(*args, rays, starts, **kw)
    ref = O.trace_backward(*args, rays, starts, fwd["rgba"], g, num_threads=1, **kw)
    for key in ("points_grad", "attr_grad"):
        assert np.isfinite(ref[key]).all() and np.abs(ref[key]).max() > 0
    hops = fwd["num_intersections"].reshape(-1)
    if name == "ball":
        # some rays never meet the ball (alpha exactly 0), others do
        alpha = fwd["rgba"][..., 3].reshape(-1)
        assert (alpha == 0).sum() > 256 and (alpha > 0).sum() > 64
    if name == "inside":
        assert hops.max() > 1.5 * hops.min()
    _REF[(name, d)] = (fm, rays, starts, g, kw, fwd, ref)
    return _REF[(name, d)]


def _backward(fm, d, rays, starts, g, kw, fwd, mode):
    import radfoam

    pipe = radfoam.create_pipeline(d)
    pipe.record_trail = True
    pipe.backward_mode = mode
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    t = lambda x: torch.from_numpy(x).to(DEV)
    f = pipe.trace_forward(p, a, adj, off, t(rays), t(starts), **kw)
    np.testing.assert_array_equal(f["rgba"].cpu().numpy().view(np.uint32), fwd["rgba"].view(np.uint32))
    assert pipe._trail is not None
    out = pipe.trace_backward(p, a, adj, off, t(rays), t(starts), f["rgba"], t(g), **kw)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("points_grad", "attr_grad")}


@pytest.mark.parametrize("name,d", [(n, d) for n in CASES for d in (0, 2)] + [("ball", 3), ("inside", 3)])
def test_epochs_do_not_change_the_gradients(foam_factory, name, d):
    fm, rays, starts, g, kw, fwd, ref = _case(foam_factory, name, d)
    cached = _backward(fm, d, rays, starts, g, kw, fwd, 3)
    plain = _backward(fm, d, rays, starts, g, kw, fwd, 2)
    for key in ("points_grad", "attr_grad"):
        for what, want in (("oracle", ref[key]), ("backward_mode 2", plain[key])):
            ok, rel, worst = H.grad_close(cached[key], want)
            print(f"{name} d={d} {key} against {what}: relative L2 {rel:.3g}, worst element {worst:.3g} of its bound")
            assert ok and rel < 1e-5, (name, d, key, what, rel, worst)
