"""Classical Lloyd iteration in a box: every site moves to the centroid of its cell,

    points <- centroid of (cell n box),

through ``radfoam.cell_geometry_in_box``.  The triangulation is rebuilt on the GPU every step.  Clipped to the box every
cell is a bounded polytope, so ALL sites move, the hull included, and the cells partition the box at every step: the
script prints the share of sites that moved, sum V / V_box (1 to rounding) and the spread of the volumes (standard
deviation over mean), which Lloyd's iteration drives down.  examples/foam_lloyd.py is the contrast: without a box the
hull's cells are unbounded and its sites have to stay where they are.

    python examples/foam_lloyd_box.py [--points 4000] [--steps 20]
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
from radfoam_amd.triangulation import Triangulation  # noqa: E402

BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


def run(num_points=4000, steps=20, seed=0, device="cuda:0", quiet=False):
    """(share of sites moved by the step, sum V / V_box, std V / mean V) before every step, and after the last one with
    the share 0: steps + 1 rows."""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()      # kd-order, kept from here on
    box_volume = (BOX[3] - BOX[0]) * (BOX[4] - BOX[1]) * (BOX[5] - BOX[2])
    rows = []
    for step in range(steps + 1):
        if step:
            tri.rebuild(points, incremental=True)
        geo = radfoam.cell_geometry_in_box(points, tri.point_adjacency(), tri.point_adjacency_offsets(), BOX)
        ratio = float(geo.volume.sum()) / box_volume
        spread = float(geo.volume.std() / geo.volume.mean())
        moved = 0.0
        if step < steps:
            target = torch.where(geo.nonempty[:, None], geo.centroid, points.double()).to(torch.float32)
            moved = float((target != points).any(1).double().mean())
            points = target.contiguous()
        rows.append((moved, ratio, spread))
        if not quiet:
            print(f"step {step:3d}: moved {100.0 * moved:6.2f} % of the sites, sum V / V_box = 1 {ratio - 1.0:+.2e}, "
                  f"std V / mean V = {spread:.4f}")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    run(args.points, args.steps, args.seed)


if __name__ == "__main__":
    main()
