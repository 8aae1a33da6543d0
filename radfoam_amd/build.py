"""Builds libradfoam_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

Every source is compiled to its own object (in parallel, rebuilt only when it or a header is newer)
and the objects are linked into the shared library; the A/B scripts under scripts/ compile
variants of single sources the same way.
"""
from __future__ import annotations

import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
SOURCES = [os.path.join(_CSRC, n) for n in ("rf_kernels.hip", "rf_scene_ops.hip", "rf_adjacency.hip", "rf_grad_exchange.hip", "rf_delaunay.hip", "rf_tile_prior.hip")]
HEADERS = [os.path.join(_CSRC, n) for n in ("rf_math.hpp", "rf_foam.hpp", "rf_wave.hpp", "rf_host.hpp", "rf_star.hpp", "rf_tiles.hpp", "rf_epoch.hpp")] + [
    os.path.join(os.path.dirname(_HERE), "include", "radfoam_hip.h")]
# Built, linked and watched like SOURCES / HEADERS, but outside source_hash(): that hash names the tracer and triangulation
# kernels the committed hardware counters and ISA constants (profiles/) were measured on.  What is listed here runs
# beside them and changes none of their code, so adding or editing it must not turn that evidence stale.
EXTRA_SOURCES = [os.path.join(_CSRC, n) for n in ("rf_cell_geometry.hip", "rf_segments.hip", "rf_segments_grad.hip",
                                                      "rf_segments_rays_grad.hip", "rf_composite.hip",
                                                      "rf_cell_geometry_grad.hip", "rf_distortion.hip",
                                                      "rf_quantiles.hip", "rf_cell_reduce.hip", "rf_sh_entries.hip",
                                                      "rf_entry_weights.hip", "rf_face_area_grad.hip",
                                                      "rf_cell_mesh.hip", "rf_cell_moments.hip",
                                                      "rf_cell_moments_grad.hip", "rf_cell_box.hip",
                                                      "rf_cell_box_grad.hip", "rf_cell_box_moments.hip",
                                                      "rf_cell_box_moments_grad.hip",
                                                      "rf_cell_box_area_grad.hip", "rf_isosurface.hip", "rf_tets.hip",
                                                      "rf_locate.hip", "rf_nearest.hip")]
EXTRA_HEADERS = [os.path.join(_CSRC, n) for n in ("rf_clip.hpp", "rf_clip_grad.hpp", "rf_ray_sweep.hpp",
                                                      "rf_segments_face.hpp", "rf_clip_area_grad.hpp",
                                                      "rf_clip_mesh.hpp", "rf_clip_moments.hpp",
                                                      "rf_clip_moments_grad.hpp", "rf_clip_box.hpp",
                                                      "rf_clip_box_grad.hpp", "rf_clip_box_moments.hpp",
                                                      "rf_clip_box_moments_grad.hpp",
                                                      "rf_clip_box_area_grad.hpp", "rf_cell_wave.hpp",
                                                      "rf_cell_sweep.hpp", "rf_iso.hpp", "rf_tets.hpp",
                                                      "rf_locate.hpp", "rf_nearest.hpp")] + [
    os.path.join(os.path.dirname(_HERE), "include", n) for n in ("radfoam_hip_geometry.h", "radfoam_hip_segments.h",
                                                               "radfoam_hip_composite.h",
                                                               "radfoam_hip_geometry_grad.h",
                                                               "radfoam_hip_distortion.h",
                                                               "radfoam_hip_quantiles.h",
                                                               "radfoam_hip_cell_reduce.h",
                                                               "radfoam_hip_sh_entries.h",
                                                               "radfoam_hip_entry_weights.h",
                                                               "radfoam_hip_face_area_grad.h",
                                                               "radfoam_hip_mesh.h",
                                                               "radfoam_hip_moments.h",
                                                               "radfoam_hip_moments_grad.h",
                                                               "radfoam_hip_box.h",
                                                               "radfoam_hip_box_grad.h",
                                                               "radfoam_hip_box_moments.h",
                                                               "radfoam_hip_box_moments_grad.h",
                                                               "radfoam_hip_box_area_grad.h",
                                                               "radfoam_hip_isosurface.h",
                                                               "radfoam_hip_tets.h",
                                                               "radfoam_hip_locate.h",
                                                               "radfoam_hip_nearest.h")]
OBJ_DIR = os.path.join(_CSRC, "_obj")
OUTPUT = os.path.join(_HERE, "libradfoam_hip.so")

# -ffp-contract=off: the kernels spell out every FMA (csrc/rf_math.hpp); nothing else may fuse.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
               "-fno-fast-math", "-Wno-unused-result"]


def _hipcc() -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else "hipcc"


def _object(src: str) -> str:
    return os.path.join(OBJ_DIR, os.path.splitext(os.path.basename(src))[0] + ".o")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def source_hash() -> str:
    """sha256 over the kernel sources and headers, in a fixed order: what a set of hardware counters was measured on
    (profiles/counters.json records it; bench.py refuses to quote counters of another build).  EXTRA_SOURCES and
    EXTRA_HEADERS are deliberately not part of it: see above."""
    import hashlib

    h = hashlib.sha256()
    for path in sorted(SOURCES + HEADERS):
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def needs_build() -> bool:
    return _stale(OUTPUT, SOURCES + HEADERS + EXTRA_SOURCES + EXTRA_HEADERS)


def _run(cmd, verbose):
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd))
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed building libradfoam_hip.so")


def build_hip(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return OUTPUT
    os.makedirs(OBJ_DIR, exist_ok=True)
    sources, headers = SOURCES + EXTRA_SOURCES, HEADERS + EXTRA_HEADERS
    todo = [s for s in sources if force or _stale(_object(s), [s] + headers)]
    with ThreadPoolExecutor(max_workers=max(1, len(todo))) as pool:
        list(pool.map(lambda s: _run([_hipcc()] + HIPCC_FLAGS + ["-c", s, "-o", _object(s)], verbose), todo))
    _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUTPUT] + [_object(s) for s in sources],
         verbose)
    return OUTPUT


if __name__ == "__main__":
    import sys

    if "--source-hash" in sys.argv:
        print(source_hash())
    else:
        print(build_hip(force=True, verbose=True))
