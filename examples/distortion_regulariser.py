"""A regulariser for a shading model of one's own: ``Pipeline.trace_differentiable_segments`` exports the walk, a colour
and a density per cell are fitted with Adam through ``radfoam.composite_entries`` to the picture the foam's own
attributes give, once with the photometric loss alone and once with ``lambda * radfoam.ray_distortion(...).mean()`` added
to it: Mip-NeRF 360's distortion loss, which pulls a ray's compositing weights together in depth.  Both runs start from
the same thin fog everywhere, which is where floaters come from.  Compositing and regulariser are HIP kernels, forward
and backward, on the device.

    python examples/distortion_regulariser.py [--points 20000] [--width 128] [--height 96] [--steps 30] [--weight 0.1]
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


def fit_walk(seg, target, num_points, steps, weight, lr=0.05, fog=0.5, log=print):
    """Fits a colour [N, 3] and a density [N] per cell along the walk ``seg`` to ``target`` [R, 3] under
    ``mse + weight * mean distortion``.  Returns the photometric loss and the mean distortion after the last step."""
    dev = target.device
    cells = seg["cells"].to(dev).to(torch.int64)
    colour = torch.zeros((num_points, 3), device=dev, requires_grad=True)                # logits: grey
    density = torch.full((num_points,), float(fog), device=dev).expm1().log().requires_grad_(True)   # softplus^-1(fog)
    opt = torch.optim.Adam([colour, density], lr=lr)
    for step in range(steps + 1):
        opt.zero_grad()
        sigma = torch.nn.functional.softplus(density)[cells]                            # one per entry
        out = radfoam.composite_entries(seg, sigma, torch.sigmoid(colour)[cells])       # [R, 4]
        mse = ((out[:, :3] - target) ** 2).mean()
        distortion = radfoam.ray_distortion(seg, sigma).mean()
        if step % 10 == 0 or step == steps:
            log(f"step {step:3d}  mse {float(mse.detach()):.6f}  mean distortion {float(distortion.detach()):.6f}")
        if step == steps:                                                               # the state the last step left
            return float(mse.detach()), float(distortion.detach())
        (mse + weight * distortion).backward()
        opt.step()


def fit(num_points=20000, width=128, height=96, steps=30, weight=0.1, seed=0, device="cuda:0", log=print):
    """Returns ((mse, mean distortion) of the run without the regulariser, (mse, mean distortion) of the run with)."""
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
        log(f"weight of the distortion loss: {lam}")
        runs.append(fit_walk(seg, target, num_points, steps, lam, log=log))
    return tuple(runs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    plain, regularised = fit(args.points, args.width, args.height, args.steps, args.weight, args.seed)
    print(f"photometric alone:     mse {plain[0]:.6f}  mean distortion {plain[1]:.6f}")
    print(f"with the regulariser:  mse {regularised[0]:.6f}  mean distortion {regularised[1]:.6f}")


if __name__ == "__main__":
    main()
