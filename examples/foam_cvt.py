"""Descending the foam's true centroidal-Voronoi energy: Adam on

    loss = mean over bounded cells of tr(site_moment[a]) / h^5  [+ lambda * anisotropy],      h = N^(-1/3),

through ``radfoam.differentiable_cell_moments``; tr(site_moment[a]) = int_{cell a} |x - p_a|^2 dx.  The counterpart of
examples/foam_lloyd.py, which descends the surrogate  sum_a V_a |p_a - c_a|^2  (the part of the energy a site can remove
by moving to its centroid): both are printed every step.  With ``--aniso LAMBDA`` the loss also penalises slivers through
the cells' covariance S_a = central_moment[a] / V_a,

    anisotropy = mean over bounded cells of |S_a - (tr S_a / 3) I|_F^2 / (tr S_a)^2,

which is zero for a cell whose covariance is a multiple of the identity and independent of the cell's size.  The
triangulation is rebuilt on the GPU every step.  Unbounded cells (the hull) have NaN moments and are masked out.

    python examples/foam_cvt.py [--points 4000] [--steps 50] [--aniso 0.0]
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


def anisotropy(moments):
    """mean over the bounded cells of |S - (tr S / 3) I|_F^2 / (tr S)^2, S = central_moment / volume"""
    b = moments.geometry.bounded
    xx, yy, zz, xy, xz, yz = (moments.central_moment[b] / moments.geometry.volume[b][:, None]).unbind(-1)
    tr = xx + yy + zz
    dev = (xx - tr / 3.0) ** 2 + (yy - tr / 3.0) ** 2 + (zz - tr / 3.0) ** 2 + 2.0 * (xy ** 2 + xz ** 2 + yz ** 2)
    return (dev / (tr * tr)).mean()


def cvt_loss(points, moments, lam):
    b = moments.geometry.bounded
    h = float(points.size(0)) ** (-1.0 / 3.0)
    loss = moments.site_moment[b][:, :3].sum(1).mean() / h ** 5
    return loss + lam * anisotropy(moments) if lam else loss


def run(num_points=4000, steps=50, lam=0.0, lr=2e-3, seed=0, device="cuda:0", quiet=False):
    """(loss, CVT energy, Lloyd surrogate, anisotropy) before every step and after the last one: steps + 1 tuples."""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].clone().requires_grad_(True)      # kd-order, kept from here on
    opt = torch.optim.Adam([points], lr=lr)
    history = []
    for step in range(steps + 1):
        if step:
            tri.rebuild(points, incremental=True)
        moments = radfoam.differentiable_cell_moments(points, tri.point_adjacency(), tri.point_adjacency_offsets())
        loss = cvt_loss(points, moments, lam)
        with torch.no_grad():
            geo = moments.geometry
            b = geo.bounded
            energy = float(moments.site_moment[b][:, :3].sum())
            surrogate = float((geo.volume[b] * ((points[b].double() - geo.centroid[b]) ** 2).sum(1)).sum())
            history.append((float(loss), energy, surrogate, float(anisotropy(moments))))
        if not quiet:
            print(f"step {step:3d}: loss {history[-1][0]:.6f}, CVT energy sum tr(site_moment) = {energy:.6g}, Lloyd "
                  f"surrogate sum V |p - c|^2 = {surrogate:.6g}, anisotropy {history[-1][3]:.5f} over {int(b.sum())} "
                  f"bounded cells")
        if step == steps:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--aniso", type=float, default=0.0, help="weight of the anisotropy penalty on central_moment / volume")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    run(args.points, args.steps, args.aniso, args.lr, args.seed)


if __name__ == "__main__":
    main()
