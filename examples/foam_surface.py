"""The foam's own surface of ``density > tau``: the Voronoi faces between cells above and below the threshold, written
as a PLY triangle mesh.  The mesh is watertight by construction (every face separates exactly one selected cell from
one unselected cell); vertices are not welded.

    python examples/foam_surface.py [--points 20000] [--tau 0] [--out foam_surface.ply]
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


def write_ply(path: str, triangles: np.ndarray) -> None:
    """Binary little-endian PLY: three vertices per triangle, in order."""
    t = np.ascontiguousarray(triangles, dtype="<f4").reshape(-1, 3)
    faces = np.empty(len(t) // 3, dtype=[("n", "u1"), ("v", "<i4", 3)])
    faces["n"] = 3
    faces["v"] = np.arange(len(t), dtype=np.int32).reshape(-1, 3)
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(t)}\nproperty float x\nproperty float y\n"
                 f"property float z\nelement face {len(faces)}\nproperty list uchar int vertex_indices\n"
                 "end_header\n").encode())
        f.write(t.tobytes())
        f.write(faces.tobytes())


def extract(num_points=20000, tau=0.0, seed=0, device="cuda:0", log=print):
    fm = foam.make_synthetic_foam(num_points, 0, seed)      # density > 0 inside a ball of radius 0.8, exactly 0 outside
    dev = torch.device(device)
    points = torch.from_numpy(fm["points"]).to(dev)
    adj = torch.from_numpy(fm["point_adjacency"].astype(np.int64)).to(dev)
    off = torch.from_numpy(fm["point_adjacency_offsets"].astype(np.int64)).to(dev)
    density = torch.from_numpy(fm["attributes"][:, -1].copy()).to(dev)
    geo = radfoam.cell_geometry(points, adj, off)
    inside = density > tau
    triangles, edge = radfoam.cell_surface(points, adj, off, inside)
    mass = (density[inside].double() * geo.volume[inside]).sum()
    log(f"{int(inside.sum())} of {num_points} cells above tau = {tau}: volume {float(geo.volume[inside].sum()):.4f}, "
        f"mass {float(mass):.4f}, {triangles.size(0)} triangles over {int(torch.unique(edge).numel())} faces")
    return triangles


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--tau", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="foam_surface.ply")
    args = ap.parse_args()
    triangles = extract(args.points, args.tau, args.seed)
    write_ply(args.out, triangles.cpu().numpy())
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
