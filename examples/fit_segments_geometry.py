"""Moving the foam under a shading model of one's own: ``Pipeline.trace_differentiable_segments`` exports every ray's walk
with ``t_enter`` / ``t_exit`` that are differentiable in the point positions, ``radfoam.composite_segments`` composites
it in torch, and autograd carries the loss back to the sites.  As in examples/custom_shading.py the colour of a cell is
three free numbers behind a sigmoid, not an SH row; here the points are fitted with it: they start a little off the
positions the target picture was rendered from.  The triangulation is the target's and stays fixed for the few steps
this runs (a longer fit rebuilds it as examples/fit_points.py does).

    python examples/fit_segments_geometry.py [--points 20000] [--width 128] [--height 96] [--steps 30]
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


def fit(num_points=20000, width=128, height=96, steps=30, seed=0, lr=0.1, point_lr=None, jitter=0.05, device="cuda:0",
        log=print):
    """Returns a dict: ``losses`` (mean squared error over rgb, one per step), ``moved`` (largest distance of a point
    from where it started) and ``points``."""
    fm = foam.make_synthetic_foam(num_points, 0, seed)
    dev = torch.device(device)
    target_points, attributes = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
    adjacency = torch.from_numpy(fm["point_adjacency"]).to(dev)
    offsets = torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
    cam = foam.default_camera(width, height)
    rays = torch.from_numpy(foam.camera_rays(cam)).to(dev)
    start = torch.full(rays.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=torch.int64,
                       device=dev).to(torch.uint32)

    pipe = radfoam.create_pipeline(0)
    target = pipe.trace_forward(target_points, attributes, adjacency, offsets, rays, start)["rgba"].reshape(-1, 4)[:, :3]

    # the learner: the same cells a fraction of the spacing off, grey
    spacing = (8.0 / num_points) ** (1.0 / 3.0)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    begin = target_points + jitter * spacing * torch.randn(num_points, 3, generator=g).to(dev)
    points = begin.clone().requires_grad_(True)
    logits = torch.zeros((num_points, 3), device=dev, requires_grad=True)
    density = attributes[:, -1].contiguous()
    point_lr = 0.02 * spacing if point_lr is None else point_lr
    opt = torch.optim.Adam([{"params": [logits], "lr": lr}, {"params": [points], "lr": point_lr}])
    losses = []
    for step in range(steps):
        opt.zero_grad()
        # the walk follows the points, so it is traced anew in every step
        seg = pipe.trace_differentiable_segments(points, attributes, adjacency, offsets, rays, start)
        rgba = radfoam.composite_segments(seg, density, torch.sigmoid(logits))
        loss = ((rgba[:, :3] - target) ** 2).mean()
        loss.backward()
        # a ray that grazes a face has an unbounded dt/dp there (as in trace_backward): such rows sit this step out
        points.grad.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
        opt.step()
        losses.append(float(loss.detach()))
        if step % 10 == 0 or step == steps - 1:
            log(f"step {step:3d}  mse {losses[-1]:.6f}  {seg['cells'].numel()} entries")
    moved = float((points.detach() - begin).norm(dim=1).max())
    return {"losses": losses, "moved": moved, "points": points.detach()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    out = fit(args.points, args.width, args.height, args.steps, args.seed)
    print(f"mse {out['losses'][0]:.6f} -> {out['losses'][-1]:.6f}; points moved by up to {out['moved']:.5f}")


if __name__ == "__main__":
    main()
