"""A foam as anisotropic Gaussians: one 3-D Gaussian per bounded Voronoi cell (or, with ``--box``, one per site: every
cell clipped to the box), written as a 3DGS-layout binary PLY that any splat viewer or splat-based tool reads.

The Gaussian of cell a is the one that matches the uniform distribution on the cell up to second order: mean the
centroid c_a, covariance C_a / V_a with C_a the cell's central second moment (``radfoam.cell_moments``).  Its scales are
the square roots of the covariance's eigenvalues and its rotation the eigenvectors as a unit quaternion (w, x, y, z).
The opacity is what a ray through the cell's middle would lose, 1 - exp(-sigma * 2 r) with r = (3 V / 4 pi)^(1/3) the
radius of the ball of the cell's volume, and the DC colour is the cell's colour.

Also prints the foam's true centroidal-Voronoi energy  sum_a int_{cell a} |x - p_a|^2 dx = sum_a tr site_moment[a]
next to the surrogate examples/foam_lloyd.py descends,  sum_a V_a |p_a - c_a|^2  (the part of the energy a site can
remove by moving to its centroid: tr site = tr central + V |c - p|^2).

Without a box the unbounded cells of the hull have no moments and are left out, of the export and of the energy.  With
``--box lo lo lo hi hi hi`` the cells are clipped to that box (``radfoam.cell_moments_in_box``): every site whose cell
reaches into the box has a Gaussian, the hull's large cells included, and the energy is that of the whole box.

    python examples/foam_to_gaussians.py [--points 4000] [--out foam_gaussians.ply] [--box -1 -1 -1 1 1 1]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SH_C0 = 0.28209479177387814      # the constant spherical harmonic: colour = 0.5 + SH_C0 * f_dc
PLY_FIELDS = ("x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
              "rot_0", "rot_1", "rot_2", "rot_3")


def _symmetric(six):
    """[M,6] as xx, yy, zz, xy, xz, yz -> [M,3,3]"""
    xx, yy, zz, xy, xz, yz = six.unbind(-1)
    return torch.stack([torch.stack([xx, xy, xz], -1), torch.stack([xy, yy, yz], -1), torch.stack([xz, yz, zz], -1)], -2)


def _quaternion(rot):
    """[M,3,3] proper rotations -> unit quaternions [M,4] as (w, x, y, z), w >= 0"""
    m00, m11, m22 = rot[:, 0, 0], rot[:, 1, 1], rot[:, 2, 2]
    # four times the squares of the components; the largest one is at least 1, so its root is a safe divisor
    sq = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1)
    big = sq.argmax(-1)
    # row k: the quaternion times 4 q_k, from the sums and differences of the off-diagonal entries
    a, b, c = rot[:, 2, 1] - rot[:, 1, 2], rot[:, 0, 2] - rot[:, 2, 0], rot[:, 1, 0] - rot[:, 0, 1]
    d, e, f = rot[:, 0, 1] + rot[:, 1, 0], rot[:, 0, 2] + rot[:, 2, 0], rot[:, 1, 2] + rot[:, 2, 1]
    cand = torch.stack([torch.stack([sq[:, 0], a, b, c], -1), torch.stack([a, sq[:, 1], d, e], -1),
                        torch.stack([b, d, sq[:, 2], f], -1), torch.stack([c, e, f, sq[:, 3]], -1)], -2)
    q = cand[torch.arange(rot.size(0), device=rot.device), big]
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.where(q[:, :1] < 0, -q, q)


def gaussians_from_moments(moments):
    """``moments``: a ``radfoam.CellMoments`` or a ``radfoam.BoxedCellMoments`` (CUDA or CPU tensors).  Returns a dict
    over the M bounded cells, or over the M non-empty cells of the boxed moments:

      cell      int64[M]   the cell's index
      mean      f64[M,3]   the centroid
      scale     f64[M,3]   square roots of the eigenvalues of central_moment / volume (clamped at 0), ascending
      rotation  f64[M,4]   unit quaternion (w, x, y, z) of the proper rotation R whose columns are the eigenvectors

    so that R diag(scale^2) R^T is the covariance central_moment / volume."""
    geo = moments.geometry
    cell = torch.nonzero(geo.nonempty if hasattr(geo, "nonempty") else geo.bounded).reshape(-1)
    cov = _symmetric(moments.central_moment[cell] / geo.volume[cell, None])
    lam, vec = torch.linalg.eigh(cov)
    flip = torch.linalg.det(vec) < 0                       # eigh promises an orthogonal matrix, not a proper one
    vec = torch.where(flip[:, None, None], vec * vec.new_tensor([1.0, 1.0, -1.0]), vec)
    return dict(cell=cell, mean=geo.centroid[cell], scale=lam.clamp_min(0.0).sqrt(), rotation=_quaternion(vec))


def write_ply(path, g, colour, opacity):
    """3DGS layout, binary little endian: x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3, all float32; scales as
    logarithms, the opacity as a logit, the colour as the DC coefficient."""
    m = g["mean"].size(0)
    tiny = torch.finfo(torch.float32).tiny
    alpha = opacity.double().clamp(1e-6, 1.0 - 1e-6)
    cols = [g["mean"], torch.zeros((m, 3), dtype=torch.float64, device=g["mean"].device),
            (colour.double() - 0.5) / SH_C0, torch.log(alpha / (1.0 - alpha))[:, None],
            torch.log(g["scale"].clamp_min(tiny)), g["rotation"]]
    table = torch.cat(cols, 1).to(torch.float32).cpu().numpy().astype("<f4")
    assert table.shape == (m, len(PLY_FIELDS))
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n%send_header\n" % (
        m, "".join(f"property float {name}\n" for name in PLY_FIELDS))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())
    return m


def cell_opacity(volume, density):
    """1 - exp(-sigma 2 r), r the radius of the ball of the cell's volume"""
    radius = (3.0 * volume / (4.0 * math.pi)) ** (1.0 / 3.0)
    return 1.0 - torch.exp(-density.double() * 2.0 * radius)


def run(num_points=4000, out="foam_gaussians.ply", seed=0, device="cuda:0", quiet=False, box=None):
    """Builds a foam of ``num_points`` uniform sites with the GPU triangulation, a density that falls off from the origin
    and a colour that follows the position, writes the PLY and returns (cells written, true CVT energy, surrogate).
    ``box``: six numbers (lo, hi); the cells are clipped to it and every non-empty one is written."""
    import radfoam
    from radfoam_amd.triangulation import Triangulation

    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    if box is None:
        moments = radfoam.cell_moments(points, tri.point_adjacency(), tri.point_adjacency_offsets())
    else:
        moments = radfoam.cell_moments_in_box(points, tri.point_adjacency(), tri.point_adjacency_offsets(), box)
    geo = moments.geometry
    g = gaussians_from_moments(moments)
    cell = g["cell"]
    density = 8.0 * torch.exp(-2.0 * (points[cell].double() ** 2).sum(1))
    colour = 0.5 + 0.5 * points[cell].double().clamp(-1.0, 1.0)
    written = write_ply(out, g, colour, cell_opacity(geo.volume[cell], density))
    energy = float(moments.site_moment[cell, :3].sum())
    surrogate = float((geo.volume[cell] * ((points[cell].double() - geo.centroid[cell]) ** 2).sum(1)).sum())
    if not quiet:
        ratio = g["scale"][:, 2] / g["scale"][:, 0].clamp_min(1e-300)
        print(f"{written} Gaussians of {num_points} cells written to {out}")
        print(f"anisotropy (largest / smallest scale): median {float(ratio.median()):.3f}, max {float(ratio.max()):.3f}")
        print(f"CVT energy sum tr(site_moment) = {energy:.6g}; Lloyd surrogate sum V |p - c|^2 = {surrogate:.6g} "
              f"({100.0 * surrogate / energy:.2f} % of it)")
    return written, energy, surrogate


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--out", default="foam_gaussians.ply")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--box", type=float, nargs=6, default=None, metavar=("LOX", "LOY", "LOZ", "HIX", "HIY", "HIZ"),
                    help="clip the cells to this box: one Gaussian per site")
    args = ap.parse_args()
    run(args.points, args.out, args.seed, box=args.box)


if __name__ == "__main__":
    main()
