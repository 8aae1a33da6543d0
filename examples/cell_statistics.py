"""Per-cell statistics for a shading model of one's own: what ``RadFoamScene.prune_and_densify`` consumes -- how much
every cell contributes to the picture, and how much of the picture's error lands on it -- computed over an exported
walk, where ``trace_forward(return_contribution=True)`` and ``trace_backward`` only know the foam's own SH colours.

``Pipeline.trace_segments`` exports the walk and ``radfoam.cell_entries`` transposes it once.  A colour and a density
per cell are looked up with ``radfoam.gather_cells`` (whose backward sums the tables' gradients without atomics, the
same bits every step) and fitted for a few steps through ``radfoam.composite_entries``.  The compositing weight of
every entry is a few lines of torch from the definition in ``composite_entries``' docstring; ``radfoam.reduce_entries``
sums it per cell (the contribution) and, times the squared error of the entry's ray, once more (the error).  The
reference's masks follow: prune where the contribution is below 1e-3, densify candidates where it is above 1e-2.

    python examples/cell_statistics.py [--points 20000] [--width 128] [--height 96] [--steps 10]
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

PRUNE_BELOW, DENSIFY_ABOVE = 1e-3, 1e-2


def entry_weights(seg, sigma):
    """(w [S] float64, ray [S] int64): the compositing weight of every entry of ``seg`` for a density ``sigma`` [S] per
    entry, and the entry's ray.  ``composite_entries``' definition: dt = 0 behind an infinite t_exit, else
    max(t_exit - t_enter, 0); x = sigma dt; w = exp(-(sum of x over the ray's earlier entries)) (1 - exp(-x))."""
    dev = sigma.device
    offsets = seg["offsets"].to(dev)
    t_enter, t_exit = (seg[k].detach().to(dev).to(torch.float64).reshape(-1) for k in ("t_enter", "t_exit"))
    dt = torch.where(torch.isinf(t_exit), torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))
    x = sigma.detach().to(torch.float64) * dt
    upto = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)])        # upto[e]: the sum over the list in front of entry e
    ray = torch.repeat_interleave(torch.arange(offsets.numel() - 1, device=dev), offsets[1:] - offsets[:-1],
                                  output_size=x.numel())
    before = upto[:-1] - upto[offsets[:-1]][ray]                   # over the ray's earlier entries
    return torch.exp(-before) * -torch.expm1(-x), ray


def cell_statistics(seg, index, sigma, rendered, target):
    """(contribution [N], error [N]) float32: per cell the sum of the compositing weights of the entries that scan it,
    and the sum of weight times the squared error of the entry's ray (``rendered`` and ``target`` [R, 3])."""
    weights, ray = entry_weights(seg, sigma)
    ray_error = ((rendered.detach() - target) ** 2).sum(-1).to(torch.float64)
    both = torch.stack([weights, weights * ray_error[ray]], dim=-1).to(torch.float32)
    per_cell = radfoam.reduce_entries(index, both)
    return per_cell[:, 0], per_cell[:, 1]


def run(num_points=20000, width=128, height=96, steps=10, lr=0.05, seed=0, device="cuda:0", log=print):
    """Fits the caller-side tables for ``steps`` steps and returns a dict: ``contribution`` and ``error`` [N], the
    ``prune`` and ``densify`` masks [N], and ``mse`` of the last step."""
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
    seg = pipe.trace_segments(points, attributes, adjacency, offsets, rays, start)
    index = radfoam.cell_entries(seg, num_points)                  # once per walk: every table and backward uses it
    lengths = index.cell_offsets[1:] - index.cell_offsets[:-1]
    log(f"{rays.numel() // 6} rays, {seg['cells'].numel()} entries over {int((lengths > 0).sum())} of {num_points} "
        f"cells; longest list {int(lengths.max())} entries")

    # the shading model: a colour and a density per cell, the density starting from the foam's own
    colour = torch.zeros((num_points, 3), device=dev, requires_grad=True)
    density = attributes[:, -1].float().clamp_min(1e-3).expm1().clamp_min(1e-6).log().requires_grad_(True)
    opt = torch.optim.Adam([colour, density], lr=lr)
    for step in range(steps + 1):
        opt.zero_grad()
        sigma = radfoam.gather_cells(index, torch.nn.functional.softplus(density))
        rendered = radfoam.composite_entries(seg, sigma, radfoam.gather_cells(index, torch.sigmoid(colour)))[:, :3]
        mse = ((rendered - target) ** 2).mean()
        if step % 5 == 0 or step == steps:
            log(f"step {step:3d}  mse {float(mse.detach()):.6f}")
        if step == steps:
            break
        mse.backward()
        opt.step()

    contribution, error = cell_statistics(seg, index, sigma.detach(), rendered, target)
    prune, densify = contribution < PRUNE_BELOW, contribution > DENSIFY_ABOVE
    return {"contribution": contribution, "error": error, "prune": prune, "densify": densify,
            "mse": float(mse.detach())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    out = run(args.points, args.width, args.height, args.steps, seed=args.seed)
    n = out["contribution"].numel()
    print(f"contribution: sum {float(out['contribution'].sum()):.3f}, largest {float(out['contribution'].max()):.3f}")
    print(f"prune (contribution < {PRUNE_BELOW}): {int(out['prune'].sum())} of {n} cells; densify candidates "
          f"(> {DENSIFY_ABOVE}): {int(out['densify'].sum())}, their share of the error "
          f"{float(out['error'][out['densify']].sum() / out['error'].sum().clamp_min(1e-30)):.3f}")


if __name__ == "__main__":
    main()
