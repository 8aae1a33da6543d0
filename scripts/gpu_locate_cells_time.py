"""Time of radfoam.locate_cells (the kernel of rf_nearest.hip) on a GPU Triangulation, beside the nearest-site search it
stands in for: N points uniform in [-1,1]^3 (seed 0; default 2 M), 2^21 queries on a regular 128^3 grid over [-1,1]^3, in
grid order and shuffled.  HIP events, 3 warm-up calls, median (min, max) of 7, a line each for: locate_cells seeded from
1024 sites, from given starts (the cell of the previous query of the same order), with seeds=0 (every walk from site 0),
nearest_point_tree on the same queries (the yardstick, same run), and Triangulation.locate with nearest="tree" and
nearest="walk".  Then the hop histogram of every mode, and the number of queries whose cell differs from the tree's fp32
answer.

One step, a process of its own under its own ``timeout -k 10``.

    python scripts/gpu_locate_cells_time.py [--points 2000000]      # a JSON line per order as measured, then one with all
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def gpu_step(n):
    import numpy as np
    import torch

    import radfoam
    from radfoam_amd.scene_ops import nearest_point_tree

    dev = "cuda:0"
    pts = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)).to(dev)
    tri = radfoam.Triangulation(pts)
    p = pts[tri.permutation().to(torch.int64)].contiguous()
    adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
    tri.locate(p[:64])                                                  # builds and keeps the tree and the tetrahedra
    tree = tri._tree
    axis = torch.linspace(-1, 1, 128, dtype=torch.float32, device=dev)
    grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3).contiguous()
    shuffled = grid[torch.randperm(grid.size(0), generator=torch.Generator().manual_seed(1)).to(dev)].contiguous()

    def stats(out):
        return [round(float(np.median(out)), 4), round(float(min(out)), 4), round(float(max(out)), 4)]

    def timed(fn, reps=7):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return stats(out)

    def hop_stats(hops):
        hops = hops.to(torch.int64)
        return {"hops_mean": round(float(hops.double().mean()), 3), "hops_max": int(hops.max()),
                "hop_histogram": torch.bincount(hops).tolist()}

    res = {"points": n, "adjacency_entries": adj.numel(), "queries": grid.size(0)}
    for name, q in (("grid", grid), ("shuffled", shuffled)):
        seeded = radfoam.locate_cells(p, adj, off, q)
        previous = torch.cat([seeded.cell[:1], seeded.cell[:-1]])      # the cell of the query before, in this order
        given = radfoam.locate_cells(p, adj, off, q, start=previous)
        tree_site = nearest_point_tree(p, tree, q).view(torch.int32).to(torch.int64)
        differ = seeded.cell != tree_site
        by_tree, by_walk = tri.locate(q, nearest="tree"), tri.locate(q, nearest="walk")
        res[name] = {
            "differ_from_tree_fp32": int(differ.sum()),
            "given_differs_from_seeded": int((given.cell != seeded.cell).sum()),      # exact ties alone depend on the start
            "located_tet_differs_between_starts": int((by_tree.tet != by_walk.tet).sum()),
            "seeded": hop_stats(seeded.hops), "given_previous_cell": hop_stats(given.hops),
            "locate_cells_seeded_ms": timed(lambda: radfoam.locate_cells(p, adj, off, q)),
            "locate_cells_given_ms": timed(lambda: radfoam.locate_cells(p, adj, off, q, start=previous)),
            "nearest_point_tree_ms": timed(lambda: nearest_point_tree(p, tree, q)),
            "locate_tree_ms": timed(lambda: tri.locate(q, nearest="tree")),
            "locate_walk_ms": timed(lambda: tri.locate(q, nearest="walk")),
            "locate_tets_hops_from_tree_mean": round(float(by_tree.hops.double().mean()), 3),
            "locate_tets_hops_from_walk_mean": round(float(by_walk.hops.double().mean()), 3)}
        print(json.dumps({name: res[name]}), flush=True)               # (the slow mode comes last: keep what is measured)
        site0 = radfoam.locate_cells(p, adj, off, q, seeds=0)
        res[name]["site0_differs_from_seeded"] = int((site0.cell != seeded.cell).sum())
        res[name]["site0"] = hop_stats(site0.hops)
        res[name]["locate_cells_site0_ms"] = timed(lambda: radfoam.locate_cells(p, adj, off, q, seeds=0))
    print(json.dumps(res), flush=True)


def main():
    n = arg("--points", "2000000")
    if "--stage" in sys.argv:
        return gpu_step(int(n))
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--stage", "gpu", "--points", n]
    rc = subprocess.run(cmd).returncode
    if rc:
        sys.exit(f"the step ended with status {rc}")


if __name__ == "__main__":
    main()
