"""Time of radfoam.isosurface (the kernels of rf_isosurface.hip, the scan and the welding in torch) and of
isosurface_vertices_grad next to their torch restatement on the same device: N points uniform in [-1,1]^3 (seed 0), their
Delaunay tetrahedra from Qhull on the host, values = the gyroid sin(kx)cos(ky) + sin(ky)cos(kz) + sin(kz)cos(kx), k = 8,
level 0 (a surface that fills the cube, about one tetrahedron in fourteen crossed).  The default is 2 M points: Qhull
takes 50 to 90 s for them on the host, 500 k take 20 s.  HIP events around the Python calls, 3
warm-up calls, median (min, max) of 7.  isosurface is also timed stage by stage (its own internal steps, called in its
order): count, the scan with its one read-back, emit, the weld (torch.unique over the packed keys), the vertices; then
the backward operator, and forward plus backward of a sphere loss through isosurface_vertices.  The two backends are
compared bit for bit before anything is timed.

Two steps, each a process of its own under its own ``timeout -k 10``: the host step draws the points and runs Qhull
(no GPU), the GPU step loads what it left and times.  Nothing runs after a step that fails.

    python scripts/gpu_isosurface_time.py [--points 2000000]      # prints one JSON line
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


def host_step(n, path):
    import numpy as np
    from scipy.spatial import Delaunay

    pts = np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)
    t0 = time.time()
    tets = np.ascontiguousarray(Delaunay(pts.astype(np.float64)).simplices, dtype=np.uint32)
    np.savez(path, points=pts, tets=tets, qhull_seconds=time.time() - t0)
    print("triangulated", n, len(tets), f"{time.time() - t0:.1f} s", flush=True)


def gpu_step(path):
    import importlib

    import numpy as np
    import torch

    import radfoam
    from radfoam_amd import _lib
    from radfoam_amd.scene_ops import _ptr, _stream

    I = importlib.import_module("radfoam_amd.isosurface")
    dev = "cuda:0"
    data = np.load(path)
    p = torch.from_numpy(data["points"]).to(dev)
    tets = torch.from_numpy(data["tets"].astype(np.int64)).to(dev).to(torch.uint32)
    k = 8.0
    x, y, z = (k * p).unbind(1)
    v = (torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)).contiguous()
    n, nt, level = p.size(0), tets.size(0), 0.0
    lib = _lib.load()

    def timed(fn, reps=7):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return [round(float(np.median(out)), 4), round(float(min(out)), 4), round(float(max(out)), 4)]

    mesh = radfoam.isosurface(p, tets, v, level)
    ref = radfoam.isosurface(p, tets, v, level, backend="torch")
    for a, b in zip(mesh, ref):
        assert torch.equal(a, b)
    sites, nv, nf = mesh.vertex_sites, mesh.vertices.size(0), mesh.triangles.size(0)
    g = torch.randn((nv, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
    gp, gv = radfoam.isosurface_vertices_grad(p, v, sites, level, g)
    wp, wv = radfoam.isosurface_vertices_grad(p, v, sites, level, g, backend="torch")
    rel = lambda a, b: float(((a - b).abs().reshape(n, -1).amax(1) / b.abs().reshape(n, -1).amax(1).clamp(min=1.0)).max())
    grad_gap = [rel(gp, wp), rel(gv, wv)]

    counts = torch.empty(nt, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    count = lambda: _lib.check(lib.rf_isosurface_count(_ptr(tets), 4, nt, _ptr(v), n, level, _ptr(counts), _ptr(bad),
                                                       _stream(dev)))
    count()
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    keys = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    tri_tet = torch.empty(nf, dtype=torch.int64, device=dev)
    emit = lambda: _lib.check(lib.rf_isosurface_emit(_ptr(tets), 4, nt, _ptr(p), _ptr(v), n, level, _ptr(counts), _ptr(ends),
                                                     nf, _ptr(keys), _ptr(tri_tet), _stream(dev)))
    emit()
    centre = torch.zeros(3, dtype=torch.float64, device=dev)

    def scan():
        e = torch.cumsum(counts, 0, dtype=torch.int64)
        torch.stack([e[-1], bad[0].to(torch.int64)]).tolist()

    def forward_backward(backend):
        q, w = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
        xs = radfoam.isosurface_vertices(q, w, sites, level, backend=backend)
        (((xs - centre).norm(dim=1) - 0.8) ** 2).mean().backward()

    tets64 = tets.to(torch.int64)
    res = {"points": n, "tets": nt, "qhull_seconds": round(float(data["qhull_seconds"]), 1), "triangles": nf, "vertices": nv,
           "crossed_tets": int((counts > 0).sum()), "grad_gap_points_values": grad_gap,
           "isosurface_hip_ms": timed(lambda: radfoam.isosurface(p, tets, v, level)),
           "isosurface_hip_int64_ms": timed(lambda: radfoam.isosurface(p, tets64, v, level)),
           "isosurface_torch_ms": timed(lambda: radfoam.isosurface(p, tets, v, level, backend="torch")),
           "count_ms": timed(count), "scan_and_readback_ms": timed(scan), "emit_ms": timed(emit),
           "extract_hip_ms": timed(lambda: I._extract_hip(p, tets, v, level)),
           "extract_torch_ms": timed(lambda: I._extract_torch(p, tets, v, level)),
           "weld_ms": timed(lambda: torch.unique(keys.reshape(-1), return_inverse=True)),
           "vertices_hip_ms": timed(lambda: I._vertices_hip(p, v, sites, level)),
           "vertices_torch_ms": timed(lambda: I._vertices_torch(p, v, sites, level)),
           "vertices_grad_hip_ms": timed(lambda: radfoam.isosurface_vertices_grad(p, v, sites, level, g)),
           "vertices_grad_torch_ms": timed(lambda: radfoam.isosurface_vertices_grad(p, v, sites, level, g, backend="torch")),
           "sphere_loss_forward_backward_hip_ms": timed(lambda: forward_backward("hip")),
           "sphere_loss_forward_backward_torch_ms": timed(lambda: forward_backward("torch"))}
    print(json.dumps(res))


def main():
    if "--stage" in sys.argv:
        return host_step(int(arg("--points", 2000000)), arg("--data", "")) if arg("--stage", "") == "host" else gpu_step(arg("--data", ""))
    n = arg("--points", "2000000")
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "foam.npz")
        for stage, limit in (("host", "900"), ("gpu", "600")):
            cmd = ["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--stage", stage, "--points", n, "--data", data]
            rc = subprocess.run(cmd).returncode
            if rc:
                sys.exit(f"the {stage} step ended with status {rc}; nothing is run after it")


if __name__ == "__main__":
    main()
