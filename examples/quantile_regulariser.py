"""The reference's depth regulariser for a shading model of one's own: ``Pipeline.trace_differentiable_segments``
exports the walk, a colour and a density per cell are fitted with Adam through ``radfoam.composite_entries`` to the
picture the foam's own attributes give, once with the photometric loss alone and once with the reference's quantile loss
added to it: ``weight * |depth[:, 0] - depth[:, 1]|.mean()`` for the depths ``radfoam.ray_quantiles`` gives at two sorted
random quantiles per ray, masked where either is never reached.  It pulls the depths at which a ray's transmittance
falls together: surfaces instead of fog.  Both runs start from the same thin fog everywhere.  A median-depth map
(q = 0.5) of the regularised result comes with it.  Compositing and quantiles are HIP kernels, forward and backward, on
the device.

    python examples/quantile_regulariser.py [--points 20000] [--width 128] [--height 96] [--steps 30] [--weight 0.1]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import radfoam  # noqa: E402
from radfoam_amd import foam  # noqa: E402


def quantile_gap(seg, sigma, quantiles):
    """The reference's loss: the mean of |depth[:, 0] - depth[:, 1]| over the rays that reach both quantiles."""
    depth, entries = radfoam.ray_quantiles(seg, sigma, quantiles)
    both = (entries >= 0).all(dim=-1)
    gap = torch.where(both, (depth[:, 0] - depth[:, 1]).abs(), torch.zeros_like(depth[:, 0]))
    return gap.sum() / both.sum().clamp_min(1)


def fit_walk(seg, target, num_points, steps, weight, lr=0.05, fog=0.5, seed=0, log=print):
    """Fits a colour [N, 3] and a density [N] per cell along the walk ``seg`` to ``target`` [R, 3] under
    ``mse + weight * mean quantile gap``, with fresh quantiles every step.  Returns the photometric loss and the mean gap
    (on one fixed draw of quantiles) after the last step, and the fitted density per entry."""
    dev = target.device
    num_rays = target.size(0)
    cells = seg["cells"].to(dev).to(torch.int64)
    colour = torch.zeros((num_points, 3), device=dev, requires_grad=True)                # logits: grey
    density = torch.full((num_points,), float(fog), device=dev).expm1().log().requires_grad_(True)   # softplus^-1(fog)
    opt = torch.optim.Adam([colour, density], lr=lr)
    draws = torch.Generator().manual_seed(seed)

    def draw():                                                                          # train.py sorts its rows so
        return torch.rand((num_rays, 2), generator=draws).sort(dim=-1, descending=True).values.to(dev)

    fixed = draw()
    for step in range(steps + 1):
        opt.zero_grad()
        sigma = torch.nn.functional.softplus(density)[cells]                            # one per entry
        out = radfoam.composite_entries(seg, sigma, torch.sigmoid(colour)[cells])       # [R, 4]
        mse = ((out[:, :3] - target) ** 2).mean()
        if step % 10 == 0 or step == steps:
            with torch.no_grad():
                measured = quantile_gap(seg, sigma, fixed)
            log(f"step {step:3d}  mse {float(mse.detach()):.6f}  mean quantile gap {float(measured):.6f}")
        if step == steps:                                                               # the state the last step left
            return float(mse.detach()), float(measured), sigma.detach()
        loss = mse + weight * quantile_gap(seg, sigma, draw()) if weight else mse
        loss.backward()
        opt.step()


def fit(num_points=20000, width=128, height=96, steps=30, weight=0.1, seed=0, device="cuda:0", log=print):
    """Returns ((mse, mean gap) of the run without the regulariser, (mse, mean gap) of the run with, the median depth
    [height, width] of the run with: -1 where a ray's transmittance stays above one half)."""
    fm = foam.make_synthetic_foam(num_points, 2, seed)
    dev = torch.device(device)
    points, attributes = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
    adjacency = torch.from_numpy(fm["point_adjacency"]).to(dev)
    offsets = torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
    cam = foam.default_camera(width, height)
    rays = torch.from_numpy(foam.camera_rays(cam)).to(dev)
    start = torch.full(rays.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=torch.int64,
                       device=dev).to(torch.uint32)

    pipe = radfoam.create_pipeline(2)
    target = pipe.trace_forward(points, attributes, adjacency, offsets, rays, start)["rgba"].reshape(-1, 4)[:, :3]
    # once: the sites stay where they are here.  With points.requires_grad_() the same two losses would move them too.
    seg = pipe.trace_differentiable_segments(points, attributes, adjacency, offsets, rays, start)
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    log(f"{rays.numel() // 6} rays, {seg['cells'].numel()} entries, longest walk {int(counts.max())} cells")
    runs = []
    for lam in (0.0, weight):
        log(f"weight of the quantile loss: {lam}")
        mse, gap, sigma = fit_walk(seg, target, num_points, steps, lam, seed=seed, log=log)
        runs.append((mse, gap))
    with torch.no_grad():
        median, _ = radfoam.ray_quantiles(seg, sigma, torch.full((target.size(0), 1), 0.5, device=dev))
    return runs[0], runs[1], median.reshape(height, width)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    plain, regularised, median = fit(args.points, args.width, args.height, args.steps, args.weight, args.seed)
    print(f"photometric alone:     mse {plain[0]:.6f}  mean quantile gap {plain[1]:.6f}")
    print(f"with the regulariser:  mse {regularised[0]:.6f}  mean quantile gap {regularised[1]:.6f}")
    reached = median[median >= 0]
    spread = f", {float(reached.min()):.3f} .. {float(reached.max()):.3f}" if reached.numel() else ""
    print(f"median depth: reached on {reached.numel()} of {median.numel()} rays{spread}")


if __name__ == "__main__":
    main()
