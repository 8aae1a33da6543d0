"""The tracer's own shading model, taken apart: spherical-harmonic coefficients and a density per cell, fitted along an
exported walk with every part replaceable.

``Pipeline.trace_segments`` exports the walk once and ``radfoam.cell_entries`` transposes it.  Per step the density of
every entry is looked up with ``radfoam.gather_cells``, its colour on its ray comes from ``radfoam.sh_entries`` (SH
degree 2 here: 27 coefficients per cell, never gathered per entry), and ``radfoam.composite_entries`` composites them
as ``trace_forward`` does.  The targets are ``trace_forward``'s picture of the foam in another state (its own
attributes); the tables start from a flat grey.  Where this example has ``softplus`` and nothing else, a caller puts a
density model of their own, a residual on the colour, a distortion or quantile loss on ``sigma``.

On a CPU device the walk and the targets come from the CPU oracle (oracle/), and the operators run their torch
backends: the same program at toy size.

    python examples/sh_shading.py [--points 20000] [--width 128] [--height 96] [--steps 40] [--device cuda:0]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import radfoam  # noqa: E402
from radfoam_amd import foam  # noqa: E402

DEGREE = 2


def _oracle_walk(fm, rays, start, cap=512):
    """(seg, target [R, 3]) from the CPU oracle: its trace_paths in the form trace_segments returns."""
    from oracle import oracle as O

    args = (DEGREE, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    cells, t_exit, n = O.trace_paths(*args, rays, start.reshape(-1), cap=cap)
    counts = n.astype(np.int64)
    if counts.max(initial=0) > cap:
        raise RuntimeError("a ray of this frame scans more cells than the oracle was asked to record")
    keep = np.arange(cap)[None, :] < counts[:, None]
    # the compositing's t0: the running maximum of 0 and the earlier exits (a first exit may be negative)
    t_enter = np.fmax.accumulate(np.concatenate([np.zeros((len(n), 1), np.float32), t_exit], axis=1), axis=1)[:, :-1]
    seg = {"offsets": torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)),
           "cells": torch.from_numpy(cells[keep].astype(np.int64)), "t_enter": torch.from_numpy(t_enter[keep]),
           "t_exit": torch.from_numpy(t_exit[keep])}
    target = O.trace_forward(*args, rays, start)["rgba"].reshape(-1, 4)[:, :3]
    return seg, torch.from_numpy(np.ascontiguousarray(target))


def main(num_points=20000, width=128, height=96, steps=40, lr=0.05, seed=0, device="cuda:0", log=print):
    """Fits the tables for ``steps`` steps and returns {"first": the loss before, "last": the loss after}."""
    fm = foam.make_synthetic_foam(num_points, DEGREE, seed)
    dev = torch.device(device)
    cam = foam.default_camera(width, height)
    rays_np = foam.camera_rays(cam)
    start_np = np.full(rays_np.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=np.uint32)
    rays = torch.from_numpy(rays_np).to(dev)
    if dev.type == "cpu":
        seg, target = _oracle_walk(fm, rays_np, start_np)
    else:
        points, attributes = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
        adjacency = torch.from_numpy(fm["point_adjacency"]).to(dev)
        offsets = torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
        start = torch.from_numpy(start_np.astype(np.int64)).to(dev).to(torch.uint32)
        pipe = radfoam.create_pipeline(DEGREE)
        target = pipe.trace_forward(points, attributes, adjacency, offsets, rays, start)["rgba"].reshape(-1, 4)[:, :3]
        seg = pipe.trace_segments(points, attributes, adjacency, offsets, rays, start)
    index = radfoam.cell_entries(seg, num_points)                  # once per walk: every table and backward uses it
    log(f"{rays.numel() // 6} rays, {index.cells.numel()} entries")

    # the shading model: SH-2 coefficients (flat grey to begin with) and a density per cell
    coeffs = torch.zeros((num_points, 3 * (DEGREE + 1) ** 2), device=dev, requires_grad=True)
    density = torch.zeros(num_points, device=dev, requires_grad=True)
    opt = torch.optim.Adam([coeffs, density], lr=lr)
    losses = []
    for step in range(steps + 1):
        opt.zero_grad()
        sigma = radfoam.gather_cells(index, torch.nn.functional.softplus(density))
        rgb = radfoam.sh_entries(seg, index, coeffs, rays[..., 3:6])
        loss = ((radfoam.composite_entries(seg, sigma, rgb)[:, :3] - target) ** 2).mean()
        losses.append(float(loss.detach()))
        if step % 10 == 0 or step == steps:
            log(f"step {step:3d}  mse {losses[-1]:.6f}")
        if step == steps:
            break
        loss.backward()
        opt.step()
    log(f"loss before {losses[0]:.6f}, after {losses[-1]:.6f}")
    return {"first": losses[0], "last": losses[-1]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    main(a.points, a.width, a.height, a.steps, seed=a.seed, device=a.device)
