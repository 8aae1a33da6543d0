"""Experiment (RF_EXPERIMENT_SECTIONS build): where the waves of the trail replay spend their time.
WORKLOAD=train-batch (default): the training-shaped batch of bench.py, backward mode 4; WORKLOAD=north-star: the 1080p
frame, backward mode 3.  Prints the wave clocks summed per section as shares of the walk."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import radfoam  # noqa: E402
from radfoam_amd import foam  # noqa: E402

dev = torch.device("cuda:0")
workload = os.environ.get("WORKLOAD", "train-batch")
sh = int(os.environ.get("SH", "3" if workload == "train-batch" else "2"))
def gpu_triangulation(raw):      # as bench.py: no cached Qhull lists on a fresh clone, and Qhull takes minutes
    from radfoam_amd import triangulation
    _, sorted_pts = triangulation.kd_order(torch.from_numpy(raw).to(dev))
    adj_, off_, _ = triangulation.delaunay_adjacency(sorted_pts)
    return sorted_pts.cpu().numpy(), off_.cpu().numpy(), adj_.cpu().numpy()


fm = foam.make_synthetic_foam(2_000_000, sh, 5, cache_dir=foam.default_cache_dir(), triangulate=gpu_triangulation)
if os.environ.get("EMPTY_DENSITY"):     # every segment lit: bench.py --empty-density
    fm = dict(fm)
    fm["attributes"] = fm["attributes"].copy()
    fm["attributes"][:, -1] = np.maximum(fm["attributes"][:, -1], np.float32(os.environ["EMPTY_DENSITY"]))
if workload == "train-batch":
    rays_np, start_np = bench.training_batch(fm, 1_000_000, 105)
else:
    cam = bench.orbit_camera(1920, 1080, 0)
    rays_np = foam.camera_rays(cam)
    start_np = np.full(rays_np.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=np.uint32)
rays, start = torch.from_numpy(rays_np).to(dev), torch.from_numpy(start_np).to(dev)
p, a = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
adj, off = torch.from_numpy(fm["point_adjacency"]).to(dev), torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
g = torch.randn(rays.shape[:-1] + (4,), generator=torch.Generator().manual_seed(1234)).to(dev)
pipe = radfoam.create_pipeline(sh)
pipe.record_trail = True
for _ in range(3):
    f = pipe.trace_forward(p, a, adj, off, rays, start)
    pipe.trace_backward(p, a, adj, off, rays, start, f["rgba"], g)
torch.cuda.synchronize()
stats = torch.zeros(48, dtype=torch.int64, device=dev)   # the image backward writes slots 8..39
pipe.experiment_stats = stats
f = pipe.trace_forward(p, a, adj, off, rays, start)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
pipe.trace_backward(p, a, adj, off, rays, start, f["rgba"], g)
e1.record()
torch.cuda.synchronize()
s = stats.cpu().tolist()
tot = s[12]
third, fourth = ("tables", "colour_rows_out") if workload == "train-batch" else ("merge_and_cache_updates", "epoch_barriers_and_flush")
flush = {}
if workload != "train-batch" and s[17]:
    # the image backward's epochs (backward_replay_cached_kernel): the three parts of "epoch_barriers_and_flush", and the
    # rows a block evicts per epoch (a block has four waves; each counts its own epochs and the rows it owns)
    block_epochs = s[17] / 4
    flush = {"share_epoch_first_barrier": round(s[14] / tot, 3), "share_epoch_flush_body": round(s[15] / tot, 3),
             "share_epoch_closing_barrier": round(s[16] / tot, 3), "block_epochs": int(block_epochs),
             "clocks_per_wave_epoch": round((s[14] + s[15] + s[16]) / s[17], 1),
             "evicted_rows_per_block_epoch": round((s[18] + s[19]) / block_epochs, 2),
             "evicted_wide_rows_per_block_epoch": round(s[18] / block_epochs, 2),
             "evicted_narrow_rows_per_block_epoch": round(s[19] / block_epochs, 2),
             "bypass_lane_adds_per_block_epoch": round(s[20] / block_epochs, 3), "bypass_lane_adds": s[20]}
    # the first barrier's wait split two ways: the wave still had a live lane in the epoch (live) or had finished
    # (done); the block added colour or point gradients in the epoch (lit) or density sums only (dens).  Shares of the
    # walk's wave clocks, wave-epochs, and the rows resident after the flush per kind of block-epoch
    kinds = ("live_lit", "live_dens", "done_lit", "done_dens")
    flush["first_barrier_split"] = {k: {"share": round(s[21 + i] / tot, 4), "wave_epochs": s[25 + i],
                                        "clocks_per_wave_epoch": round(s[21 + i] / max(s[25 + i], 1), 1)} for i, k in enumerate(kinds)}
    flush["resident_rows_after_flush"] = {
        "lit": {"block_epochs": s[33], "mean": round(s[29] / max(s[33], 1), 2), "max": s[31]},
        "dens": {"block_epochs": s[34], "mean": round(s[30] / max(s[34], 1), 2), "max": s[32]}}
    flush["long_block_epochs"] = s[35]
    # the segment section split by the kind of wave-step: "all_empty" = every lane that has a segment is in a cell of
    # density exactly 0 (what the empty-run memo can serve), "other" = the rest (wave-steps without any segment
    # included); took_memo_path = the all-empty wave-steps that skipped the functor (0 in a build without the memo)
    flush["segment_split"] = {
        "all_empty": {"wave_steps": s[37], "share_of_walk": round(s[36] / tot, 4), "share_of_segment_section": round(s[36] / max(s[9], 1), 4),
                      "clocks_per_wave_step": round(s[36] / max(s[37], 1), 1), "took_memo_path": s[38]},
        "other": {"wave_steps": s[13] - s[37], "share_of_walk": round((s[9] - s[36]) / tot, 4),
                  "share_of_segment_section": round((s[9] - s[36]) / max(s[9], 1), 4),
                  "clocks_per_wave_step": round((s[9] - s[36]) / max(s[13] - s[37], 1), 1), "without_any_segment": s[39]}}
print(json.dumps({"lib": os.path.basename(os.environ.get("RADFOAM_HIP_LIB", "libradfoam_hip.so")), "workload": workload, "sh_degree": sh, "empty_density": os.environ.get("EMPTY_DENSITY"), "backward_ms": round(e0.elapsed_time(e1), 3), "wave_steps": s[13],
                  "clocks_per_wave_step": round(tot / max(s[13], 1), 1),
                  "share_wait_records_and_face_hit": round(s[8] / tot, 3), "share_segment_colour_row_and_math": round(s[9] / tot, 3),
                  "share_" + third: round(s[10] / tot, 3), "share_" + fourth: round(s[11] / tot, 3),
                  "share_other": round(1 - (s[8] + s[9] + s[10] + s[11]) / tot, 3), **flush}))
