"""Area-weighted total variation of a per-cell density on a foam in a box, by gradient descent: Adam on

    L(points) = tv * sum_{faces {a,b}} A_ab |sigma_a - sigma_b| / (N s^2)  +  sum_a V_a |p_a - c_a|^2 / (V_box s^2),

s = (V_box / N)^(1/3), with A_ab, V_a and c_a those of the cells clipped to the box through
``radfoam.differentiable_cell_geometry_in_box(..., face_area=True)``: the boxed face areas carry autograd to the points
(``radfoam.face_area_in_box_grad``) beside the volumes and centroids of the Lloyd energy, every site moves, and the
triangulation is rebuilt on the GPU every step.  sigma is a fixed density per site (a smooth bump plus noise).

In the box every face is a bounded polygon, so the face term reaches every site, the hull included.  The unboxed operator
``radfoam.face_area_grad`` only reaches faces of finite area: the script prints, per step, how many sites receive a nonzero
face-area gradient from the same upstream with and without the box, and how many adjacency slots only the box reaches:
slots whose unboxed area is +inf, where face_area_grad ignores the upstream, and whose boxed area is positive.  A hull
site usually keeps some finite faces, so the site counts can agree while those faces go unregularised without the box.

    python examples/foam_tv_box.py [--points 4000] [--steps 20] [--tv 1.0]
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


def reached(grad: torch.Tensor) -> int:
    """the number of sites with a nonzero row"""
    return int((grad != 0.0).any(1).sum())


def run(num_points=4000, steps=20, seed=0, device="cuda:0", tv=1.0, lr=None, quiet=False):
    """(loss, sites the boxed face-area gradient reaches, sites the unboxed one reaches, every site's gradient finite,
    slots only the box reaches) per step: ``steps`` rows, the loss evaluated before the step's update."""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous().requires_grad_(True)      # kd-order, kept from here on
    noise = torch.rand(num_points, generator=gen, dtype=torch.float64).to(dev)
    sigma = torch.exp(-2.0 * (points.detach().double() ** 2).sum(1)) + 0.25 * noise          # fixed per site
    box_volume = (BOX[3] - BOX[0]) * (BOX[4] - BOX[1]) * (BOX[5] - BOX[2])
    size = (box_volume / num_points) ** (1.0 / 3.0)
    if lr is None:
        lr = 0.05 * size                                           # a twentieth of the mean cell's size per step
    opt = torch.optim.Adam([points], lr=lr)
    rows = []
    for step in range(steps):
        if step:
            tri.rebuild(points.detach(), incremental=True)
        adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
        geo = radfoam.differentiable_cell_geometry_in_box(points, adj, off, BOX, face_area=True)
        row = torch.repeat_interleave(torch.arange(num_points, device=dev), torch.diff(off.to(torch.int64)))
        jump = (sigma[row] - sigma[adj.to(torch.int64)]).abs()
        weight = 0.5 * tv * jump / (num_points * size * size)       # every face has two slots
        ne = geo.nonempty
        offset = points.double()[ne] - geo.centroid[ne]
        lloyd = (geo.volume[ne] * (offset * offset).sum(1)).sum() / (box_volume * size * size)
        loss = (weight * geo.face_area).sum() + lloyd
        opt.zero_grad(set_to_none=True)
        loss.backward()
        finite = bool(torch.isfinite(points.grad).all())
        with torch.no_grad():       # the face term alone, from the same upstream, with and without the box
            plain = radfoam.cell_geometry(points.detach(), adj, off)
            boxed = reached(radfoam.face_area_in_box_grad(points.detach(), adj, off, BOX,
                                                          radfoam.BoxedCellGeometry(*(x.detach() for x in geo)), weight))
            unboxed = reached(radfoam.face_area_grad(points.detach(), adj, off, plain, weight))
            rescued = int((torch.isinf(plain.face_area) & (geo.face_area.detach() > 0)).sum())
        rows.append((float(loss.detach()), boxed, unboxed, finite, rescued))
        if not quiet:
            print(f"step {step:3d}: loss = {rows[-1][0]:.6e}, face-area gradient reaches {boxed} of {num_points} sites in "
                  f"the box, {unboxed} without it; {rescued} of {adj.numel()} slots only the box reaches; gradients "
                  f"{'finite' if finite else 'NOT finite'}")
        opt.step()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tv", type=float, default=1.0, help="weight of the total-variation term")
    args = ap.parse_args()
    run(args.points, args.steps, args.seed, tv=args.tv)


if __name__ == "__main__":
    main()
