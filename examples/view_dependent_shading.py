"""A colour that depends on the ray, which no per-cell table can hold: ``Pipeline.trace_segments`` exports the walk once,
a tiny two-layer MLP turns (an embedding of the entry's cell, the direction of the entry's ray) into a colour PER ENTRY,
and ``radfoam.composite_entries`` composites those along the tracer's intervals (a HIP kernel, forward and backward, on
the device).  The embeddings and the MLP are fitted with Adam to the picture the foam's own SH-degree-2 colours give,
which do change with the direction; the density stays the foam's.

    python examples/view_dependent_shading.py [--points 20000] [--width 128] [--height 96] [--steps 30]
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


def fit(num_points=20000, width=128, height=96, steps=30, seed=0, lr=0.02, features=8, hidden=16, device="cuda:0",
        log=print):
    """Returns the loss (mean squared error over rgb) before the first and after the last step."""
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
    seg = pipe.trace_segments(points, attributes, adjacency, offsets, rays, start)     # once: the walk does not change
    num_rays, total = rays.numel() // 6, seg["cells"].numel()
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    log(f"{num_rays} rays, {total} entries, longest walk {int(counts.max())} cells")

    # what every entry's colour is computed from: its cell and the direction of its ray
    cells = seg["cells"].to(torch.int64)
    ray = torch.repeat_interleave(torch.arange(num_rays, device=dev), counts, output_size=total)
    direction = torch.nn.functional.normalize(rays.reshape(-1, 6)[:, 3:], dim=-1)[ray]
    sigma = attributes[:, -1].float()[cells].contiguous()

    gen = torch.Generator(device="cpu").manual_seed(seed)
    embedding = (0.1 * torch.randn((num_points, features), generator=gen)).to(dev).requires_grad_(True)
    w1 = (torch.randn((features + 3, hidden), generator=gen) / (features + 3) ** 0.5).to(dev).requires_grad_(True)
    b1 = torch.zeros(hidden, device=dev, requires_grad=True)
    w2 = (torch.randn((hidden, 3), generator=gen) / hidden ** 0.5).to(dev).requires_grad_(True)
    b2 = torch.zeros(3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([embedding, w1, b1, w2, b2], lr=lr)
    first = last = None
    for step in range(steps):
        opt.zero_grad()
        hidden_layer = torch.relu(torch.cat([embedding[cells], direction], dim=-1) @ w1 + b1)
        colour = torch.sigmoid(hidden_layer @ w2 + b2)                                  # [S, 3], one per entry
        out = radfoam.composite_entries(seg, sigma, colour)                             # [R, 4]
        loss = ((out[:, :3] - target) ** 2).mean()
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if step % 10 == 0 or step == steps - 1:
            log(f"step {step:3d}  mse {last:.6f}")
    return first, last


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    first, last = fit(args.points, args.width, args.height, args.steps, args.seed)
    print(f"mse {first:.6f} -> {last:.6f}")


if __name__ == "__main__":
    main()
