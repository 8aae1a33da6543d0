"""Centroidal Voronoi tessellation of a box by gradient descent: Adam on the Lloyd energy of the cells clipped to the box,

    E(points) = sum_a V_a |p_a - c_a|^2   (+ weight * N * sum_a (V_a - V_box / N)^2 / V_box^2, an equal-volume penalty),

through ``radfoam.differentiable_cell_geometry_in_box``: V_a and c_a carry autograd to the points, and the explicit p_a
does through torch.  The triangulation is rebuilt on the GPU every step.  Clipped to the box every cell is a bounded
polytope, so every site has a gradient, the hull included, and the energy can be mixed with any other loss; the
fixed-point iteration of examples/foam_lloyd_box.py cannot.  The script prints sum V / V_box (1 to rounding) and the
energy per step.

With ``--energy cvt`` the energy is the true centroidal-Voronoi energy of the whole box,

    E(points) = sum_a tr site_moment[a] = sum_a int_{cell a n box} |x - p_a|^2 dx,

through ``radfoam.differentiable_cell_moments_in_box`` (the Lloyd energy above is the part of it a site can remove by
moving to its centroid), and ``--aniso LAMBDA`` adds LAMBDA * E0 * anisotropy, the penalty of examples/foam_cvt.py on the
cells' covariance S_a = central_moment[a] / V_a, here over every non-empty cell, hull cells included:

    anisotropy = mean_a |S_a - (tr S_a / 3) I|_F^2 / (tr S_a)^2,        E0 = V_box (V_box / N)^(2/3).

Both combine with ``--equal-volume``: moments and volumes in one loss, which the backward takes in one launch.

    python examples/foam_cvt_box.py [--points 4000] [--steps 20] [--equal-volume 0.0] [--energy lloyd|cvt] [--aniso 0.0]
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


def anisotropy(moments):
    """mean over the non-empty cells of |S - (tr S / 3) I|_F^2 / (tr S)^2, S = central_moment / volume"""
    ne = moments.geometry.nonempty
    xx, yy, zz, xy, xz, yz = (moments.central_moment[ne] / moments.geometry.volume[ne][:, None]).unbind(-1)
    tr = xx + yy + zz
    dev = (xx - tr / 3.0) ** 2 + (yy - tr / 3.0) ** 2 + (zz - tr / 3.0) ** 2 + 2.0 * (xy ** 2 + xz ** 2 + yz ** 2)
    return (dev / (tr * tr)).mean()


def run(num_points=4000, steps=20, seed=0, device="cuda:0", equal_volume=0.0, lr=None, quiet=False, energy="lloyd",
        aniso=0.0):
    """(sum V / V_box, energy, every site's gradient finite) per step: ``steps`` rows, the energy evaluated before the
    step's update.  ``energy``: "lloyd" (sum V |p - c|^2) or "cvt" (sum tr site_moment); ``aniso``: the weight of the
    anisotropy penalty.  Either of the two takes the cells through differentiable_cell_moments_in_box."""
    if energy not in ("lloyd", "cvt"):
        raise ValueError("energy must be 'lloyd' or 'cvt'")
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous().requires_grad_(True)      # kd-order, kept from here on
    box_volume = (BOX[3] - BOX[0]) * (BOX[4] - BOX[1]) * (BOX[5] - BOX[2])
    if lr is None:
        lr = 0.05 * (box_volume / num_points) ** (1.0 / 3.0)       # a twentieth of the mean cell's size per step
    opt = torch.optim.Adam([points], lr=lr)
    rows = []
    for step in range(steps):
        if step:
            tri.rebuild(points.detach(), incremental=True)
        if energy == "cvt" or aniso:
            moments = radfoam.differentiable_cell_moments_in_box(points, tri.point_adjacency(),
                                                                 tri.point_adjacency_offsets(), BOX)
            geo = moments.geometry
        else:
            moments = None
            geo = radfoam.differentiable_cell_geometry_in_box(points, tri.point_adjacency(),
                                                              tri.point_adjacency_offsets(), BOX)
        ne = geo.nonempty
        if energy == "cvt":
            value = moments.site_moment[ne][:, :3].sum()
        else:
            offset = points.double()[ne] - geo.centroid[ne]
            value = (geo.volume[ne] * (offset * offset).sum(1)).sum()
        loss = value
        if aniso:
            loss = loss + aniso * box_volume * (box_volume / num_points) ** (2.0 / 3.0) * anisotropy(moments)
        if equal_volume:
            share = geo.volume / box_volume - 1.0 / num_points
            loss = loss + equal_volume * num_points * (share * share).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        finite = bool(torch.isfinite(points.grad).all())
        ratio = float(geo.volume.detach().sum()) / box_volume
        rows.append((ratio, float(value.detach()), finite))
        if not quiet:
            print(f"step {step:3d}: sum V / V_box = 1 {ratio - 1.0:+.2e}, energy = {rows[-1][1]:.6e}, "
                  f"gradients {'finite' if finite else 'NOT finite'}")
        opt.step()      # a site that leaves the box keeps what its cell cuts out of it, and its gradient
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--equal-volume", type=float, default=0.0)
    ap.add_argument("--energy", choices=("lloyd", "cvt"), default="lloyd",
                    help="lloyd: sum V |p - c|^2; cvt: sum tr site_moment, the true centroidal-Voronoi energy of the box")
    ap.add_argument("--aniso", type=float, default=0.0, help="weight of the anisotropy penalty on central_moment / volume")
    args = ap.parse_args()
    run(args.points, args.steps, args.seed, equal_volume=args.equal_volume, energy=args.energy, aniso=args.aniso)


if __name__ == "__main__":
    main()
