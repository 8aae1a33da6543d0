"""Time of radfoam.delaunay_tets (the kernels of rf_tets.hip, the scans and the face sort in torch) on the lists of a GPU
Triangulation: N points uniform in [-1,1]^3 (seed 0; default 2 M).  HIP events, 3 warm-up calls, median (min, max) of 7:
the operator without and with ``adjacency``, every stage of a call (events at the marks of radfoam_amd/tets.py: the count
kernel, the scans with the first read-back, the emit kernel, the match kernel, the sums with the second read-back, the
face sort, the pairing kernel and its read-back), and radfoam.isosurface on these kd-ordered rows (the gyroid of
scripts/gpu_isosurface_time.py at level 0).  ``--parent`` then runs what the getter was before on the same points --
Qhull on the host, once, a process of its own without the GPU -- and adds its seconds.

Two steps, each a process of its own under its own ``timeout -k 10``.  Nothing runs after a step that fails.

    python scripts/gpu_tets_time.py [--points 2000000] [--parent]      # prints one JSON line per step
"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def gpu_step(n, path):
    import numpy as np
    import torch

    import radfoam
    from radfoam_amd import tets as T

    dev = "cuda:0"
    pts = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)).to(dev)
    tri = radfoam.Triangulation(pts)
    p = pts[tri.permutation().to(torch.int64)].contiguous()
    adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
    if path:
        np.save(path, p.cpu().numpy())

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

    def stages(adjacency, reps=7):
        """median (min, max) between consecutive marks of a call"""
        runs = []
        for r in range(3 + reps):
            marks = []

            def hook(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))

            T.stage_hook = hook
            try:
                radfoam.delaunay_tets(p, adj, off, adjacency=adjacency)
            finally:
                T.stage_hook = None
            torch.cuda.synchronize()
            if r >= 3:
                runs.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(marks, marks[1:])})
        return {name: stats([run[name] for run in runs]) for name in runs[0]}

    mesh = radfoam.delaunay_tets(p, adj, off, adjacency=True)
    again = radfoam.delaunay_tets(p, adj, off, adjacency=True)
    assert all(torch.equal(a, b) for a, b in zip(mesh[:3], again[:3])) and mesh.hull_faces == again.hull_faces
    k = 8.0
    x, y, z = (k * p).unbind(1)
    v = (torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)).contiguous()
    iso = radfoam.isosurface(p, mesh.tets, v, 0.0)
    res = {"points": n, "adjacency_entries": adj.numel(), "tets": mesh.tets.size(0), "hull_faces": mesh.hull_faces,
           "max_degree": int((off.to(torch.int64)[1:] - off.to(torch.int64)[:-1]).max()),
           "iso_triangles": iso.triangles.size(0), "iso_vertices": iso.vertices.size(0),
           "delaunay_tets_ms": timed(lambda: radfoam.delaunay_tets(p, adj, off)),
           "delaunay_tets_adjacency_ms": timed(lambda: radfoam.delaunay_tets(p, adj, off, adjacency=True)),
           "stages_ms": stages(True),
           "isosurface_kd_rows_ms": timed(lambda: radfoam.isosurface(p, mesh.tets, v, 0.0)),
           "rebuild_incremental_ms": timed(lambda: tri.rebuild(p, incremental=True), reps=3)}
    print(json.dumps(res), flush=True)


def parent_step(path):
    import numpy as np
    from scipy.spatial import Delaunay

    pts = np.load(path)
    t0 = time.time()
    simplices = Delaunay(pts.astype(np.float64)).simplices
    print(json.dumps({"parent_getter_qhull_seconds": round(time.time() - t0, 1), "tets": len(simplices)}), flush=True)


def main():
    n = arg("--points", "2000000")
    if "--stage" in sys.argv:
        return gpu_step(int(n), arg("--data", "")) if arg("--stage", "") == "gpu" else parent_step(arg("--data", ""))
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "points.npy")
        steps = [("gpu", "600")] + ([("parent", "900")] if "--parent" in sys.argv else [])
        for stage, limit in steps:
            cmd = ["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--stage", stage, "--points", n,
                   "--data", data]
            rc = subprocess.run(cmd).returncode
            if rc:
                sys.exit(f"the {stage} step ended with status {rc}; nothing is run after it")


if __name__ == "__main__":
    main()
