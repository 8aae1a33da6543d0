"""radfoam_amd -- MI355X-native differentiable Voronoi ray tracer (drop-in for radfoam's tracing path).

Public surface = the reference's ``radfoam`` module (torch_bindings/radfoam/__init__.py.in:29
re-exporting torch_bindings): ``create_pipeline`` and ``Pipeline.trace_forward /
trace_backward / trace_benchmark`` run hand-written HIP kernels for gfx950 behind the C-ABI of
include/radfoam_hip.h; everything else the reference module exports is a torch/scipy shim
(radfoam_amd/shims.py).  ``import radfoam`` resolves to this package through the alias
package ``radfoam/`` at the repo root.
"""
from .cells import CellEntries, cell_entries, gather_cells, reduce_entries
from .geometry import (BoxedCellGeometry, BoxedCellMoments, CellGeometry, CellMoments, cell_geometry,
                       cell_geometry_grad, cell_geometry_in_box, cell_geometry_in_box_grad, cell_moments,
                       cell_moments_grad, cell_moments_in_box, cell_moments_in_box_grad, cell_surface,
                       differentiable_cell_geometry, differentiable_cell_geometry_in_box, differentiable_cell_moments,
                       differentiable_cell_moments_in_box, face_area_grad, face_area_in_box_grad)
from .isosurface import IsoMesh, isosurface, isosurface_vertices, isosurface_vertices_grad
from .locate import FieldSamples, TetLocation, interpolate, interpolate_grad, locate_tets
from .nearest import CellLocation, locate_cells
from .mesh import CellMesh, cell_mesh, mesh_vertices, mesh_vertices_grad
from .pipeline import Pipeline, create_pipeline, invalidate_caches
from .scene_ops import pack_attributes
from .segments import (composite_entries, composite_segments, entry_weights, ray_distortion, ray_quantiles,
                       segment_points_grad, segment_rays_grad)
from .sh_entries import sh_entries
from .tets import DelaunayTets, delaunay_tets
from .shims import (BatchFetcher, Triangulation, TriangulationFailedError, Viewer, build_aabb_tree,
                    farthest_neighbor, nn, run_with_viewer)

__all__ = [
    "Pipeline", "create_pipeline", "Triangulation", "TriangulationFailedError", "build_aabb_tree",
    "nn", "farthest_neighbor", "BatchFetcher", "Viewer", "run_with_viewer", "pack_attributes",
    "invalidate_caches", "CellGeometry", "cell_geometry", "cell_surface", "composite_segments",
    "segment_points_grad", "segment_rays_grad", "composite_entries", "cell_geometry_grad",
    "differentiable_cell_geometry", "ray_distortion", "ray_quantiles", "CellEntries", "cell_entries",
    "gather_cells", "reduce_entries", "sh_entries", "entry_weights", "face_area_grad", "CellMesh", "cell_mesh",
    "mesh_vertices", "mesh_vertices_grad", "CellMoments", "cell_moments", "cell_moments_grad",
    "differentiable_cell_moments", "BoxedCellGeometry", "cell_geometry_in_box",
    "cell_geometry_in_box_grad", "differentiable_cell_geometry_in_box", "BoxedCellMoments", "cell_moments_in_box",
    "cell_moments_in_box_grad", "differentiable_cell_moments_in_box", "face_area_in_box_grad", "IsoMesh", "isosurface",
    "isosurface_vertices", "isosurface_vertices_grad", "DelaunayTets", "delaunay_tets",
    "TetLocation", "locate_tets", "FieldSamples", "interpolate", "interpolate_grad", "CellLocation", "locate_cells",
]
