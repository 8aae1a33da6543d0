"""A loss that is not linear in the compositing weights: the ray-entropy regulariser ``-sum_e w_e log(w_e + eps)``,
which is small where a ray's weight sits in few entries (a surface) and large where it is smeared along the ray (fog).
``radfoam.composite_entries`` cannot give it, as it only sums the weights; ``radfoam.entry_weights`` hands them out, one
per entry of the exported walk, with a backward of its own.

``Pipeline.trace_segments`` exports the walk and ``radfoam.cell_entries`` transposes it once.  A colour and a density
per cell are looked up with ``radfoam.gather_cells`` and fitted for a few steps through ``radfoam.composite_entries``,
once on the photometric loss alone and once with ``lambda`` times the mean ray entropy added.  At the end the same
weights, summed per cell with ``radfoam.reduce_entries``, give what ``RadFoamScene.prune_and_densify`` consumes: the
contribution of every cell and the weight-times-error that lands on it (examples/cell_statistics.py spells those
weights out by hand in float64 torch).

    python examples/weight_entropy.py [--points 20000] [--width 128] [--height 96] [--steps 20] [--weight 0.05]
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

EPS = 1e-8


def ray_entropy(seg, sigma, ray):
    """[R]: ``-sum_e w_e log(w_e + EPS)`` over the entries of every ray, differentiable in ``sigma``."""
    weights = radfoam.entry_weights(seg, sigma)
    per_entry = -weights * torch.log(weights + EPS)
    return torch.zeros(seg["offsets"].numel() - 1, dtype=sigma.dtype, device=sigma.device).index_add(0, ray, per_entry)


def fit(seg, index, ray, target, density0, steps, lr, entropy_weight, log):
    """Fits a colour and a density per cell for ``steps`` steps on ``mse + entropy_weight * mean ray entropy``; returns
    (mse, mean ray entropy, sigma [S], rendered [R, 3]) of the fitted tables."""
    colour = torch.zeros((density0.numel(), 3), device=density0.device, requires_grad=True)
    density = density0.clone().requires_grad_(True)
    opt = torch.optim.Adam([colour, density], lr=lr)
    for step in range(steps + 1):
        opt.zero_grad()
        sigma = radfoam.gather_cells(index, torch.nn.functional.softplus(density))
        rendered = radfoam.composite_entries(seg, sigma, radfoam.gather_cells(index, torch.sigmoid(colour)))[:, :3]
        mse = ((rendered - target) ** 2).mean()
        entropy = ray_entropy(seg, sigma, ray).mean()
        if step % 5 == 0 or step == steps:
            log(f"  step {step:3d}  mse {float(mse.detach()):.6f}  mean ray entropy {float(entropy.detach()):.4f}")
        if step == steps:
            break
        (mse + entropy_weight * entropy if entropy_weight else mse).backward()
        opt.step()
    return float(mse.detach()), float(entropy.detach()), sigma.detach(), rendered.detach()


def run(num_points=20000, width=128, height=96, steps=20, lr=0.05, entropy_weight=0.05, seed=0, device="cuda:0",
        log=print):
    """Fits the caller-side tables twice and returns a dict: ``mse_without`` / ``mse_with`` and ``entropy_without`` /
    ``entropy_with`` (the mean ray entropy) of the two fits, and ``contribution`` and ``error`` [N] of the second."""
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
    num_rays, total = seg["offsets"].numel() - 1, seg["cells"].numel()
    ray = torch.repeat_interleave(torch.arange(num_rays, device=dev), seg["offsets"][1:] - seg["offsets"][:-1],
                                  output_size=total)
    log(f"{num_rays} rays, {total} entries")

    # the shading model: a colour and a density per cell, the density starting from the foam's own
    density0 = attributes[:, -1].float().clamp_min(1e-3).expm1().clamp_min(1e-6).log()
    out = {}
    for name, weight in (("without", 0.0), ("with", entropy_weight)):
        log(f"{name} the entropy term (weight {weight}):")
        mse, entropy, sigma, rendered = fit(seg, index, ray, target, density0, steps, lr, weight, log)
        out["mse_" + name], out["entropy_" + name] = mse, entropy

    # per cell: the sum of the weights of the entries that scan it, and of weight times the squared error of their ray
    weights = radfoam.entry_weights(seg, sigma)
    ray_error = ((rendered - target) ** 2).sum(-1)
    per_cell = radfoam.reduce_entries(index, torch.stack([weights, weights * ray_error[ray]], dim=-1))
    out["contribution"], out["error"] = per_cell[:, 0], per_cell[:, 1]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--weight", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    out = run(args.points, args.width, args.height, args.steps, entropy_weight=args.weight, seed=args.seed)
    print(f"mse {out['mse_without']:.6f} -> {out['mse_with']:.6f}, mean ray entropy {out['entropy_without']:.4f} -> "
          f"{out['entropy_with']:.4f} with the term")
    print(f"contribution: sum {float(out['contribution'].sum()):.3f}, largest {float(out['contribution'].max()):.3f}; "
          f"error: sum {float(out['error'].sum()):.4f}")


if __name__ == "__main__":
    main()
