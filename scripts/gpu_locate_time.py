"""Time of Triangulation.locate / radfoam.locate_tets / interpolate / interpolate_grad (the kernels of rf_locate.hip) on a GPU
Triangulation: N points uniform in [-1,1]^3 (seed 0; default 2 M), 2^21 queries on a regular 128^3 grid over [-1,1]^3, in
grid order and shuffled.  HIP events, 3 warm-up calls, median (min, max) of 7, a line each for: the nearest-site stage
(nearest_point_tree and the gather of vert_to_tet), the walk from those starts, interpolate and interpolate_grad (one
channel), and for scale the torch restatement of interpolate on the device and Triangulation.rebuild(incremental=True).
Then the hop histogram of either order, and on the first 2^14 queries of either order the host build of the walk
(tests/host_harness) with its count of predicates that left the fp64 filter, and the numpy walk on 2^12 of them.

One step, a process of its own under its own ``timeout -k 10``.

    python scripts/gpu_locate_time.py [--points 2000000]      # prints one JSON line
"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def gpu_step(n):
    import numpy as np
    import torch

    import radfoam
    from radfoam_amd import locate as L
    from radfoam_amd.scene_ops import nearest_point_tree
    from tests.host_harness import locate_host as H

    dev = "cuda:0"
    pts = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)).to(dev)
    tri = radfoam.Triangulation(pts)
    p = pts[tri.permutation().to(torch.int64)].contiguous()
    tets, adjacency, vert_to_tet = tri.tets(), tri.tet_adjacency(), tri.vert_to_tet()
    tri.locate(p[:64])                                                  # builds and keeps the tree
    tree = tri._tree
    axis = torch.linspace(-1, 1, 128, dtype=torch.float32, device=dev)
    grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3).contiguous()
    shuffled = grid[torch.randperm(grid.size(0), generator=torch.Generator().manual_seed(1)).to(dev)].contiguous()
    values = p.norm(dim=1).contiguous()

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

    def nearest_stage(q):
        near = nearest_point_tree(p, tree, q).view(torch.int32).to(torch.int64)
        return vert_to_tet.view(torch.int32)[near]

    res = {"points": n, "tets": tets.size(0), "queries": grid.size(0)}
    for name, q in (("grid", grid), ("shuffled", shuffled)):
        start = nearest_stage(q)
        where = radfoam.locate_tets(p, tets, adjacency, q, start=start)
        again = tri.locate(q)
        assert torch.equal(where.tet, again.tet) and torch.equal(where.hops, again.hops)
        up = torch.ones(q.size(0), dtype=torch.float64, device=dev)
        hops = where.hops.to(torch.int64)
        host_n = 2 ** 14
        host = H.walk(p.cpu().numpy(), tets.cpu().numpy(), adjacency.cpu().numpy(), q[:host_n].cpu().numpy(),
                      start[:host_n].cpu().numpy())
        assert np.array_equal(host["tet"], where.tet[:host_n].cpu().numpy())
        t0 = time.time()
        H.walk(p.cpu().numpy(), tets.cpu().numpy(), adjacency.cpu().numpy(), q[:host_n].cpu().numpy(), start[:host_n].cpu().numpy())
        host_s = time.time() - t0
        cpu = [x.cpu() for x in (p, tets, adjacency, q[:2 ** 12], start[:2 ** 12])]
        t0 = time.time()
        slow = radfoam.locate_tets(cpu[0], cpu[1], cpu[2], cpu[3], start=cpu[4])
        numpy_s = time.time() - t0
        assert torch.equal(slow.tet, where.tet[:2 ** 12].cpu())
        res[name] = {
            "outside": int((where.tet < 0).sum()), "hops_max": int(hops.max()), "hops_mean": round(float(hops.double().mean()), 3),
            "hop_histogram": torch.bincount(hops).tolist(),
            "nearest_site_ms": timed(lambda: nearest_stage(q)),
            "walk_ms": timed(lambda: radfoam.locate_tets(p, tets, adjacency, q, start=start)),
            "triangulation_locate_ms": timed(lambda: tri.locate(q)),
            "interpolate_ms": timed(lambda: radfoam.interpolate(p, tets, values, q, where.tet)),
            "interpolate_torch_ms": timed(lambda: radfoam.interpolate(p, tets, values, q, where.tet, backend="torch")),
            "interpolate_grad_ms": timed(lambda: radfoam.interpolate_grad(p, tets, values, q, where.tet, up)),
            "interpolate_grad_torch_ms": timed(lambda: radfoam.interpolate_grad(p, tets, values, q, where.tet, up, backend="torch")),
            "host_walk_queries": host_n, "host_walk_seconds_with_table_copies": round(host_s, 3),
            "host_predicates": host["predicates"], "host_predicates_past_fp64_filter": host["exact"],
            "numpy_walk_queries": 2 ** 12, "numpy_walk_seconds": round(numpy_s, 3)}
    res["rebuild_incremental_ms"] = timed(lambda: tri.rebuild(p, incremental=True), reps=3)
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
