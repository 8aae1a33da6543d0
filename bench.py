#!/usr/bin/env python
"""bench.py -- Mrays/s of the HIP Voronoi tracer on synthetic foams (BASELINE.json metric).

Contract (driver): ``python bench.py --gpus N --steps K --warmup W`` prints ONE JSON line on rank 0.
With N > 1 and no launcher environment (RANK unset) it starts the N ranks itself (re-executes under
``python -m torch.distributed.run --nproc-per-node N`` on 127.0.0.1); launched by the driver under
torch.distributed.run it reads RANK / LOCAL_RANK / WORLD_SIZE as usual.  One rank per GPU, RCCL.

Default workload = the north-star point of SURVEY.md 8(d) ("Mrays/s fwd+bwd @1080p, 2M-pt foam"):
N = 2,000,000 seeded uniform points (kd-ordered, Qhull CSR, empty shell beyond r = 0.8), SH degree 2
(A = 28), fp32 attributes, ONE 1080x1920 pinhole frame, default trace settings (weight_threshold 1e-3,
max_intersections 1024), upstream gradient ~ N(0,1).  ``--workload`` selects the other BASELINE configs
(c2, c5) and the labelled stand-ins for the two that need datasets (render = C3, train-batch = C4).

One "step" = foam geometry packing (cell records + fp16 face offsets: what the reference's
prefetch_adjacent_diff redoes inside both of its calls; the adjacency-derived links are packed once,
before the timed region, like the CSR they come from) + trace_forward + trace_backward through the
radfoam boundary + -- for N > 1 -- the gradient exchange.

Multi-GPU (north star: "a full image's rays shard by row across the GPUs of one node"): STRONG scaling
by default -- the SAME frame, rows cut into N contiguous blocks of equal measured cost
(radfoam_amd.dist.ShardedTracer.rebalance, from the warm-up steps' num_intersections), foam replicated,
partial gradients summed by the sparse row exchange (dist.SparseGradExchange; ``--exchange dense`` = one
all-reduce of the flat buffer).  value = frame rays / max-over-ranks step time.  ``--weak`` keeps round 1's
mode: one frame per rank (rank r's camera orbits by r*45 degrees), dense all-reduce.

All inputs are resident in HBM before the timed region.  The JSON carries, per SURVEY 8(d) and the judge's
round-1 review: the walk kernels' average launch durations (HIP events on the launch stream inside the timed
region), ``roofline`` for the dominant kernel -- its real bound (VALU issue, from the SQ counters committed
under profiles/), measured HBM traffic against both peaks and against a compulsory-traffic floor, and the
8(d) algorithmic-bytes figure as a throughput, not a fraction -- and ``cpu_baseline``: the C oracle (a port:
the reference has no CPU tracer) on a bounded sample of the same rays on the host cores, with the full
gradient parity of that sample next to it.

A plain run does only what the headline figure needs: set-up, the warm-up steps, the ``--steps`` timed steps and the
JSON line (``ms_per_step`` = wall time of one timed step).  Everything else it measures or checks -- the repeated frame,
the triangulation timings, ``roofline``, ``cpu_baseline`` and, on the default line, ``other_workloads`` -- runs only
with ``--full``.  ``--dump-outputs DIR`` writes what the last timed step returned to its caller (forward outputs and
gradients, or the rendered frame) as ``DIR/<name>.npy``, float32 (float64 for integer outputs); an output too large for
the 60 MB budget is written as a fixed, seeded sample of its rows (rays or points).  With the same arguments the inputs
are the same in every run, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_SPEC_GBS = 8000.0      # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_MEASURED_GBS = 6290.0  # achievable streaming copy, same guide
NUM_SIMDS = 256 * 4             # 256 CUs x 4 SIMDs
NUM_XCDS = 8                    # GRBM_GUI_ACTIVE is reported summed over the 8 XCDs' GRBM instances
FP32_VECTOR_PEAK_TFLOPS = 157.3  # 256 CUs x 128 FMA lanes x 2 flop x 2.4 GHz (same guide)
# Irreducible work of the forward walk, read off the ISA of the shipped kernel by scripts/isa_stats.py --constants
# (profiles/isa_constants.json, with the sha256 of the sources it was compiled from): the face scan
# issues SCAN_VALU_PER_4_FACES VALU instructions per block of four faces (SCAN_FLOP_PER_4_FACES fp32 flops among them),
# a hop -- link, next cell record, trail entry, loop bookkeeping -- HOP_VALU_PER_LANE, a composited segment
# COMPOSITE_VALU_PER_LANE more (SH degree 2: colour row, exp).  useful_valu_frac below = the wave-instructions these
# would take with every lane busy on a real (unpadded) face / hop / segment, over the wave-instructions the launch
# actually issued (SQ_INSTS_VALU): issue-slot EFFICIENCY, next to valu_issue_frac, which is issue-slot UTILISATION.
# The literals are what the committed file holds; isa_constants() refuses to quote them when the file disagrees or was
# made from other sources.
SCAN_VALU_PER_4_FACES = 67
SCAN_FLOP_PER_4_FACES = 92
HOP_VALU_PER_LANE = 84      # (round 5 quoted 92: it counted the statically inlined preamble of the contested cells' rescan)
COMPOSITE_VALU_PER_LANE = 61


def isa_constants():
    """(constants or None, why not): the committed ISA figures, only if they describe the sources that are running and
    equal the literals above."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "isa_constants.json")))
    except (OSError, ValueError):
        return None, "profiles/isa_constants.json missing"
    from radfoam_amd import build as hip_build
    if rec.get("csrc_sha256") != hip_build.source_hash():
        return None, "profiles/isa_constants.json was made from other kernel sources: python scripts/isa_stats.py --constants"
    want = {"scan_valu_per_4_faces": SCAN_VALU_PER_4_FACES, "scan_flop_per_4_faces": SCAN_FLOP_PER_4_FACES,
            "hop_valu_per_lane": HOP_VALU_PER_LANE, "composite_valu_per_lane": COMPOSITE_VALU_PER_LANE}
    got = {k: rec.get(k) for k in want}
    if got != want:
        return None, f"bench.py's ISA constants {want} disagree with profiles/isa_constants.json {got}"
    return got, None


# name -> (points, seed, sh_degree, width, height, forward_only, kind, label)
WORKLOADS = {
    "north-star": dict(points=2_000_000, seed=5, sh=2, width=1920, height=1080, forward_only=False, kind="image",
                       label="north-star"),
    "c2": dict(points=500_000, seed=1, sh=2, width=1920, height=1080, forward_only=False, kind="image",
               label="BASELINE config 2"),
    "c5": dict(points=4_000_000, seed=4, sh=3, width=3840, height=2160, forward_only=True, kind="image",
               label="BASELINE config 5"),
    # stand-ins for the two configs that need a dataset / trained checkpoint; labelled as such
    "train-batch": dict(points=2_000_000, seed=5, sh=3, width=0, height=0, forward_only=False, kind="batch",
                        rays=1_000_000, label="stand-in for BASELINE config 4 (training batch)"),
    # the same batch through the foam as TRAINING sees it: the scene's density is a softplus, never exactly 0, and the
    # reference sets empty cells to raw -1 -> 4.5e-6 > 1e-6 (scene.py:202-217,459): every segment is "lit" (fetches its
    # colour row, emits a gradient row).  The synthetic foam's exact-zero shell (16 % lit) is the easy case.
    "train-batch-lit": dict(points=2_000_000, seed=5, sh=3, width=0, height=0, forward_only=False, kind="batch",
                            rays=1_000_000, empty_density=4.5e-6,
                            label="stand-in for BASELINE config 4 (training batch, every segment lit as the scene's "
                                  "softplus density makes it)"),
    "render": dict(points=1_000_000, seed=2, sh=3, width=1557, height=1038, forward_only=True, kind="render",
                   label="stand-in for BASELINE config 3 (benchmark.py render path)"),
    # BASELINE config 4 as a LOOP: the reference's unmodified RadFoamScene driven as train.py:162-270 drives it
    # (examples/train_loop.py); --steps = iterations (default 300), value = iterations per second
    "train-loop": dict(points=2_000_000, seed=5, sh=3, width=1920, height=1080, forward_only=False, kind="loop",
                       rays=1_000_000, label="stand-in for BASELINE config 4 (full training loop)"),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 10; train-loop: 300 iterations)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="north-star")
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--sh-degree", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--quantiles", type=int, default=0,
                    help="depth quantiles per ray (train.py:176-180 draws 2 per ray, sorted descending, and backpropagates "
                         "through the depths); 0 = the headline configuration of SURVEY 8(d)")
    ap.add_argument("--backward-mode", type=int, default=0)
    ap.add_argument("--weak", action="store_true", help="N>1: one frame per rank instead of one frame cut by rows")
    ap.add_argument("--exchange", choices=["sparse", "dense"], default="sparse")
    ap.add_argument("--no-rebalance", action="store_true", help="N>1: keep the even row split")
    ap.add_argument("--tile-order", default=None,
                    help="image workloads: Pipeline.tile_order_mode (default: the pipeline's own)")
    ap.add_argument("--empty-density", type=float, default=None,
                    help="raise the foam's zero densities to this value (4.5e-6 = activation_scale * softplus(-1, beta=10), "
                         "what the reference's scene gives its empty cells, scene.py:459): every segment is then 'lit' "
                         "(> 1e-6), as in real training, where softplus never returns exactly 0")
    ap.add_argument("--strict-scan", action="store_true",
                    help="Pipeline.strict_reference_scan: every face of every cell divided, the way the reference writes its scan "
                         "(tracing_utils.cuh:43-67; rf_launch_opts.forward_mode 3) in forward and render -- same results as "
                         "the default filtered scan (the bitwise comparison with the oracle holds for both), slower")
    ap.add_argument("--forward-mode", type=int, default=None,
                    help="Pipeline.forward_mode (experiments): 1 blocks, 2 eager, 3 = --strict-scan, 4 persistent waves with refill, "
                         "5 eager behind the block-level LDS cell table (auto for sorted flat batches)")
    ap.add_argument("--grad-pitch", default=None, help="Pipeline.gradient_row_pitch: auto (default), dense, or floats")
    ap.add_argument("--full", action="store_true",
                    help="also run the untimed extras: repeated frame, triangulation timings, roofline, cpu_baseline and, "
                         "on the default line, other_workloads (a plain run times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, 60 MB at most: "
                         "larger outputs as a fixed, seeded sample of their rows)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--repeat-frame", action="store_true",
                    help="time the steps on ONE frame / batch traced over and over (what rounds 1-4 reported) instead of on "
                         "rays that are new in every step; the default line reports this as detail.value_repeated_frame")
    ap.add_argument("--no-repeated-frame", action="store_true",
                    help="skip the extra (untimed for the metric) repeated-frame measurement: profiling runs, whose "
                         "per-kernel averages should be those of the fresh-ray steps alone")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="default line only: skip the untimed `other_workloads` record (c2, c5, render, train-batch)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU-baseline sample time")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (gloo: CPU test of the launcher)")
    args = ap.parse_args(argv)
    if args.steps is None:
        args.steps = 300 if args.workload == "train-loop" else 10
    return args


def resolve_workload(args):
    w = dict(WORKLOADS[args.workload])
    for key, arg in (("points", args.points), ("seed", args.seed), ("sh", args.sh_degree), ("width", args.width),
                     ("height", args.height)):
        if arg is not None:
            w[key] = arg
            w["custom"] = True
    if args.forward_only:
        w["forward_only"] = True
    w["name"] = args.workload
    w["nq"] = int(args.quantiles)
    return w


# ------------------------------------------------------------------------------------------------
# launcher


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """``python bench.py --gpus N`` without a launcher: start N ranks under torch.distributed.run."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.call(cmd, env=env)


# ------------------------------------------------------------------------------------------------
# inputs


def orbit_camera(width, height, rank):
    """Rank r looks at the foam centre from distance 3, rotated r*45deg about +y (rank 0 is the
    SURVEY 8(d) camera at (0,0,-3) looking +z)."""
    from radfoam_amd import foam

    cam = foam.default_camera(width, height)
    th = rank * math.pi / 4.0
    c, s = math.cos(th), math.sin(th)
    cam["position"] = np.array([-3.0 * s, 0.0, -3.0 * c], dtype=np.float32)
    cam["forward"] = np.array([s, 0.0, c], dtype=np.float32)
    cam["right"] = np.array([c, 0.0, -s], dtype=np.float32)
    return cam


VIEW_STEP_DEGREES = 0.05


def view_camera(width, height, rank, view):
    """The camera of step `view` of rank `rank`: orbit_camera(rank) moved on by 0.05 degrees per view (two pixels of the
    1080p frame) -- every ray of every step is new, as with benchmark.py:95-139's different camera per frame, while
    the steps stay the same work to within a percent (a path of 1.5 degrees per view was measured first: the cube's
    corners come into view and the frames get up to 20 % longer, which says nothing about the tracer).  View 0 is
    orbit_camera(rank) itself."""
    return orbit_camera(width, height, rank + view * (VIEW_STEP_DEGREES / 45.0))


def training_batch(fm, num_rays, seed):
    """C4 stand-in: rays drawn at random from the frames of 8 cameras around the foam (train.py:61 feeds the
    tracer shuffled rays of all training views), with each ray's entry cell."""
    from radfoam_amd import foam

    rng = np.random.default_rng(seed)
    per = (num_rays + 7) // 8
    rays, starts = [], []
    for k in range(8):
        cam = orbit_camera(1920, 1080, k)
        r = foam.camera_rays(cam).reshape(-1, 6)
        pick = rng.choice(r.shape[0], size=per, replace=False)
        rays.append(r[pick])
        starts.append(np.full(per, foam.nearest_point(fm["points"], cam["position"]), dtype=np.uint32))
    rays = np.concatenate(rays)[:num_rays]
    starts = np.concatenate(starts)[:num_rays]
    perm = rng.permutation(num_rays)
    return np.ascontiguousarray(rays[perm]), np.ascontiguousarray(starts[perm])


def algorithmic_bytes(stats, num_rays, attr_dim, c=4, nq=0, render=False):
    """logical bytes, no cache reuse credited, no padding, no zero atomics.  render: the benchmark
    kernel reads no ray and no start cell per pixel (camera by value) and writes one RGBA8 word."""
    cells, faces, hops = stats["cells_scanned"], stats["faces_scanned"], stats["hops"]
    seg, lit = stats["segments"], stats["segments_lit"]
    attr_read = c * (seg + (attr_dim - 1) * lit)          # density always, SH row only when lit
    walk = 8 * cells + 8 * faces + (4 + 12) * hops
    fwd = num_rays * (4 if render else (24 + 4 + 4 * c + 4 + 12 * nq)) + walk + attr_read
    bwd = num_rays * (24 + 4 + 8 * c + 12 * nq) + walk + attr_read + attr_read + 12 * seg
    return fwd, bwd


def load_counters(workload_name, custom):
    """Per-launch hardware counters of the walk kernels on this workload, from the committed rocprofv3 passes
    (profiles/counters.json, written by scripts/update_profiles.py from separate --pmc runs: a process
    cannot read its own PMC counters)."""
    if custom:
        return None
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "counters.json")))
        entry = tj.get(workload_name)
    except (OSError, ValueError):
        return None
    if entry is None:
        return None
    # the counters describe ONE build of the kernels: quote them only for the same sources
    from radfoam_amd import build as hip_build
    entry = dict(entry)
    entry["stale"] = entry.get("csrc_sha256") != hip_build.source_hash()
    return entry


DUMP_BUDGET_BYTES = 60_000_000   # --dump-outputs writes at most this much in all
DUMP_SAMPLE_SEED = 20240


def dump_outputs(directory, arrays):
    """--dump-outputs: ``arrays`` = [(name, tensor or ndarray, number of leading dims that index rays / points)], written
    as ``directory/<name>.npy``: floating outputs as float32 (float64 stays float64), integer outputs as float64 (exact).
    The budget is shared out smallest output first; an output larger than its share keeps a sample of its rows, drawn
    with a fixed seed from the row count alone, in ascending order -- the same rows in every run of the same arguments."""
    os.makedirs(directory, exist_ok=True)
    host = []
    for name, a, lead in arrays:
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        if a.dtype.kind == "f":
            a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        else:
            a = a.astype(np.float64)
        host.append((name, a, lead))
    left, todo = DUMP_BUDGET_BYTES, len(host)
    for name, a, lead in sorted(host, key=lambda x: x[1].nbytes):
        share = left // todo
        if a.nbytes > share:
            rows = a.reshape((int(np.prod(a.shape[:lead], dtype=np.int64)),) + a.shape[lead:])
            row_bytes = max(rows.nbytes // max(rows.shape[0], 1), 1)
            keep = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(rows.shape[0], share // row_bytes,
                                                                         replace=False))
            a = rows[keep]
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a))
        left, todo = left - a.nbytes, todo - 1


# ------------------------------------------------------------------------------------------------


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Test hook (tests/test_bench_launcher.py only): a Pipeline-shaped object on CPU tensors, so that the
    # launcher, the row sharding and the exchange of this file run under gloo on a box without GPUs.  It is
    # never set by the driver; a run that uses it says so in its JSON and measures nothing.
    test_factory = os.environ.get("RF_BENCH_TEST_PIPELINE")
    on_gpu = test_factory is None
    if on_gpu:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the tracer has no CPU path")
        ndev = torch.cuda.device_count()
        if local_rank >= ndev and args.backend == "nccl":
            raise SystemExit(f"bench.py: rank {local_rank} has no GPU of its own ({ndev} visible); RCCL needs one device per "
                             "rank (--backend gloo shares them: a functional run, not a measurement)")
        dev = torch.device("cuda", local_rank % ndev)
        torch.cuda.set_device(dev)     # before the process group: RCCL binds its communicator to the current device
    else:
        dev = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        kw = {"device_id": dev} if (on_gpu and args.backend == "nccl") else {}
        dist.init_process_group(backend=args.backend, rank=rank, world_size=world, **kw)

    env = dict(torch=torch, dist=dist, world=world, rank=rank, dev=dev, on_gpu=on_gpu, test_factory=test_factory,
               shared_gpus=bool(on_gpu and world > torch.cuda.device_count()))
    W = resolve_workload(args)
    result = run_train_loop(args, W, env) if W["kind"] == "loop" else run_workload(args, W, env)
    if result is not None and on_gpu and world == 1 and args.workload == "north-star" and not W.get("custom") and \
            args.full and not args.forward_only and not args.quantiles and not args.no_other_workloads and \
            not args.no_cpu_baseline:
        # one --full run also observes the other BASELINE configurations (untimed extras of the
        # north-star line; each is what `--workload <name> --full` prints, with fewer steps and a smaller CPU sample,
        # reduced to the figures a reader checks first)
        result["other_workloads"] = other_workloads(args, env)
    if result is not None:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


def run_train_loop(args, W, env):
    """--workload train-loop: examples/train_loop.py.  One JSON line in the same shape as the others; `value` is iterations
    per second.  ``--gpus N``: BASELINE config 4 as the north star states it -- the same loop on every rank, every batch's
    rays split over the ranks (radfoam.BatchFetcher(rank=, world_size=)), gradients exchanged inside trace_backward
    (radfoam_amd.dist.DataParallelPipeline), identical Adam step and rebuild on every rank: strong scaling of the batch."""
    if not env["on_gpu"]:
        raise SystemExit("--workload train-loop needs GPUs (tests/test_dist_training.py covers the step on CPU ranks)")
    torch, dist, dev, world, rank = env["torch"], env["dist"], env["dev"], env["world"], env["rank"]
    from examples import train_loop
    from radfoam_amd import foam

    def gpu_triangulation(raw):
        from radfoam_amd import triangulation
        _, sorted_pts = triangulation.kd_order(torch.from_numpy(raw).to(dev))
        adj, off, _ = triangulation.delaunay_adjacency(sorted_pts)
        return sorted_pts.cpu().numpy(), off.cpu().numpy(), adj.cpu().numpy()

    t0 = time.time()
    if world > 1 and rank != 0:
        dist.barrier()      # rank 0 triangulates (or loads) first, so the cache is written once
    fm = foam.make_synthetic_foam(W["points"], W["sh"], W["seed"], cache_dir=foam.default_cache_dir(),
                                  triangulate=gpu_triangulation)
    if world > 1 and rank == 0:
        dist.barrier()
    kept = {}
    its, detail = train_loop.run(args, env, fm, sh_degree=W["sh"], iterations=args.steps, rays_per_batch=W["rays"],
                                 width=W["width"], height=W["height"], densify_at=max(1, args.steps // 2), keep=kept)
    if args.dump_outputs and rank == 0:     # what the loop hands its caller: the trained scene
        m = kept.pop("model")
        dump_outputs(args.dump_outputs, [(k, getattr(m, k), 1) for k in ("primal_points", "density", "att_dc", "att_sh")])
    if world > 1:           # the slowest rank's clock (the ranks meet in every step's exchange: they agree to a step)
        t = torch.tensor([detail["wall_seconds"]], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        its = args.steps / float(t.item())
        detail["wall_seconds_slowest_rank"] = round(float(t.item()), 2)
        if rank != 0:
            return None
    detail["setup_and_loop_seconds"] = round(time.time() - t0, 1)
    per = detail["ms_per_iteration"]
    tracer = per["tracer_forward"] + per["tracer_backward"]
    detail["tracer_share_of_wall"] = round(tracer / detail["wall_ms_per_iteration"], 4)
    return {
        "metric": f"training iterations/s, {W['label']}",
        "value": round(its, 3), "unit": "it/s", "n_gpus": world, "steps": args.steps, "warmup": 0,
        "ms_per_step": detail["wall_ms_per_iteration"], "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32",
        "data": "synthetic" if not env.get("shared_gpus") else
                "synthetic (the ranks SHARE GPUs under gloo: a functional run of the data-parallel loop, not a measurement)",
        "config": {
            "workload": f"{W['label']}: the reference's unmodified RadFoamScene + TraceRays (radfoam_model/scene.py, "
                        f"render.py) on a synthetic {W['points']}-point foam (seed {W['seed']}), SH degree {W['sh']}, "
                        f"{W['rays']}-ray shuffled batches from 8 synthetic 1080p views, 2 depth quantiles per ray, Adam, "
                        f"update_triangulation on the schedule of train.py:243-248, one densification at iteration "
                        f"{max(1, args.steps // 2)} (collect_error_map + prune_and_densify + full rebuild)",
            "num_points": W["points"], "sh_degree": W["sh"], "rays_per_step": W["rays"],
            "weight_threshold": 1e-3, "max_intersections": 1024,
            "parallelism": "1 GPU" if world == 1 else
                           f"data parallel over {world} GPUs: every batch's rays split by index ({W['rays'] // world} per rank), "
                           "foam and optimiser replicated, gradients averaged inside trace_backward (one all-reduce of the "
                           "flat [points_grad | attr_grad] buffer), every rank rebuilds its own identical triangulation",
        },
        "mrays_per_second_through_the_loop": round(its * W["rays"] / 1e6, 2),
        "detail": detail,
    }


OTHER_WORKLOADS = ("c2", "c5", "render", "train-batch", "train-batch-lit")


def other_workloads(args, env):
    torch = env["torch"]
    out = {}
    for name in OTHER_WORKLOADS:
        sub = argparse.Namespace(**vars(args))
        sub.workload, sub.steps, sub.warmup = name, 5, 3
        sub.cpu_seconds = min(args.cpu_seconds, 6.0)
        sub.dump_outputs = None     # the outputs written are the north-star line's own
        t0 = time.time()
        try:
            r = run_workload(sub, resolve_workload(sub), env)
            cb, rf, det = r.get("cpu_baseline") or {}, r.get("roofline") or {}, r["detail"]
            out[name] = {
                "workload": r["config"]["workload"], "metric": r["metric"], "value": r["value"], "unit": r["unit"],
                "steps": sub.steps, "warmup": sub.warmup, "ms_per_step": r["ms_per_step"],
                "forward_ms": det.get("forward_ms"), "backward_ms": det.get("backward_ms"),
                "rays": det.get("rays"), "value_repeated_frame": det.get("value_repeated_frame"),
                "foam_pack_ms": det.get("foam_pack_ms"), "foam_csr": det.get("foam_csr"),
                "matches_gpu_bitwise": cb.get("matches_gpu_bitwise"),
                "literal_reference_scan": ({k: (cb.get("literal_reference_scan") or {}).get(k) for k in
                                            ("matches_gpu_bitwise", "rays", "share_of_the_step", "error")
                                            if k in (cb.get("literal_reference_scan") or {})} or None),
                "points_grad_rel_l2": cb.get("points_grad_rel_l2"), "attr_grad_rel_l2": cb.get("attr_grad_rel_l2"),
                "grads_within_1e-3": (None if "points_grad_within_1e-3" not in cb else
                                      bool(cb["points_grad_within_1e-3"] and cb["attr_grad_within_1e-3"])),
                "cpu_baseline": {k: cb.get(k) for k in ("value", "unit", "cores", "kind", "sample", "error") if k in cb},
                "roofline": {k: rf.get(k) for k in ("bound", "kernel", "frac", "achieved", "peak", "traffic",
                                                    "avg_launch_ms", "algorithmic_GBps", "counters_stale")},
                "seconds": None,
            }
        except Exception as exc:  # noqa: BLE001  (an extra must never take the north-star line down)
            out[name] = {"error": repr(exc)}
        out[name]["seconds"] = round(time.time() - t0, 1)
        torch.cuda.empty_cache()
    return out


def run_workload(args, W, env):
    """One workload measured as the module docstring says; returns the JSON record on rank 0, None elsewhere."""
    torch, dist, world, rank, dev = env["torch"], env["dist"], env["world"], env["rank"], env["dev"]
    on_gpu, test_factory = env["on_gpu"], env["test_factory"]
    from radfoam_amd import dist as rdist
    from radfoam_amd import foam

    strong = world > 1 and not args.weak and W["kind"] in ("image", "batch")
    sh_degree = W["sh"]

    # ---- inputs (resident before timing) -------------------------------------------------------
    t_setup = time.time()
    cache = foam.default_cache_dir()
    if world > 1 and rank != 0:
        dist.barrier()      # rank 0 triangulates (or loads) first, so the cache is written once
    tri_ms = {}

    def gpu_triangulation(raw):
        # no cached Qhull lists for this foam (a fresh clone): the GPU triangulation builds them in under a second
        # instead of minutes of Qhull; tests/test_delaunay.py holds its lists equal to Qhull's on the cached foams
        from radfoam_amd import triangulation
        t0 = time.perf_counter()
        _, sorted_pts = triangulation.kd_order(torch.from_numpy(raw).to(dev))
        adj, off, _ = triangulation.delaunay_adjacency(sorted_pts)
        torch.cuda.synchronize(dev)
        tri_ms["triangulation_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        return sorted_pts.cpu().numpy(), off.cpu().numpy(), adj.cpu().numpy()

    fm = foam.make_synthetic_foam(W["points"], sh_degree, W["seed"], cache_dir=cache,
                                  triangulate=gpu_triangulation if dev.type == "cuda" else None)
    if world > 1 and rank == 0:
        dist.barrier()
    attr_dtype = torch.float16 if W["kind"] == "render" else torch.float32
    empty_density = args.empty_density if args.empty_density is not None else W.get("empty_density")
    if empty_density is not None:
        fm = dict(fm)
        fm["attributes"] = fm["attributes"].copy()
        fm["attributes"][:, -1] = np.maximum(fm["attributes"][:, -1], np.float32(empty_density))
        if args.empty_density is not None:
            W["custom"] = True
            W["label"] += f", empty cells at density {args.empty_density:g} (every segment lit)"
    base_view = rank if (world > 1 and not strong) else 0

    def make_view(k):
        """Rays of view k: k = 0 is the frame / batch every untimed extra refers to; the timed steps take k = 1, 2, ..."""
        if W["kind"] == "batch":
            r_np, s_np = training_batch(fm, W["rays"], W["seed"] + 100 + k)
            return None, r_np, s_np
        c = view_camera(W["width"], W["height"], base_view, k)
        r_np = foam.camera_rays(c)
        return c, r_np, np.full(r_np.shape[:-1], foam.nearest_point(fm["points"], c["position"]), dtype=np.uint32)

    cam, rays_np, start_np = make_view(0)
    setup_s = time.time() - t_setup

    points = torch.from_numpy(fm["points"]).to(dev)
    attributes = torch.from_numpy(fm["attributes"]).to(attr_dtype).to(dev)
    adjacency = torch.from_numpy(fm["point_adjacency"]).to(dev)
    offsets = torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
    rays = torch.from_numpy(rays_np).to(dev)
    start = torch.from_numpy(start_np).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(1234 + (rank if (world > 1 and not strong) else 0))
    grad_rgba = torch.randn(rays.shape[:-1] + (4,), generator=gen).to(dev)
    frame_rays = rays.numel() // 6
    nq = int(args.quantiles) if W["kind"] != "render" else 0
    quantiles = depth_grad = None
    if nq:
        quantiles = torch.rand(rays.shape[:-1] + (nq,), generator=gen).sort(dim=-1, descending=True).values.to(dev)
        depth_grad = torch.randn(rays.shape[:-1] + (nq,), generator=gen).to(dev)

    if on_gpu:
        import radfoam
        pipe = radfoam.create_pipeline(sh_degree, attr_dtype)
        pipe.backward_mode = args.backward_mode
        pipe.record_trail = not W["forward_only"]   # trace_backward is driven by hand on plain tensors
        if args.tile_order is not None:
            pipe.tile_order_mode = None if args.tile_order == "static" else args.tile_order
        if args.forward_mode is not None:
            pipe.forward_mode = args.forward_mode
        if args.strict_scan:
            pipe.strict_reference_scan = True
            W["custom"] = True
            W["label"] += ", every face divided (forward_mode 3)"
        if args.grad_pitch is not None:
            pipe.gradient_row_pitch = args.grad_pitch if args.grad_pitch in ("auto", "dense") else int(args.grad_pitch)
    else:
        mod, fn = test_factory.split(":")
        pipe = getattr(importlib.import_module(mod), fn)(sh_degree)
    A = pipe.attribute_dim()

    exchange = args.exchange if (strong and W["kind"] == "image") else "dense"
    tracer = rdist.ShardedTracer(pipe, exchange=exchange)
    sync = (lambda: torch.cuda.synchronize()) if on_gpu else (lambda: None)

    class _NoEvent:
        def record(self):
            pass

    ev = (lambda: torch.cuda.Event(enable_timing=True)) if on_gpu else (lambda: _NoEvent())
    pack_ev, fwd_ev, bwd_ev, exch_ev = [], [], [], []
    last = {}

    render_out = render_diff = None
    if W["kind"] == "render":
        render_diff = pipe.build_adjacent_diff(points, adjacency, offsets)
        render_out = torch.zeros((W["height"], W["width"]), dtype=torch.uint32, device=dev)

    def device_view(c, r_dev, s_dev):
        v = {"rays": r_dev, "start": s_dev}
        if W["kind"] == "render":
            v["cam"] = {k: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x) for k, x in c.items()}
            v["cam_start"] = s_dev.reshape(-1)[:1].contiguous()
        return v

    view0 = device_view(cam, rays, start)
    # The timed steps trace rays that are NEW in every step -- a camera path for frames and renders (benchmark.py:95-139
    # renders a different test camera per frame), another shuffled batch per step for flat batches (train.py:61) -- so
    # that nothing the pipeline learns from a trace (block order of the forward, ray order, hop trail) is learnt on the
    # very rays it is then timed on; what a backward takes from ITS forward it may keep.  All views resident before timing.
    fresh = []
    if not args.repeat_frame:
        for k in range(1, min(args.warmup + args.steps, 24) + 1):
            c, r_np, s_np = make_view(k)
            fresh.append(device_view(c, torch.from_numpy(r_np).to(dev), torch.from_numpy(s_np).to(dev)))
    # (24 views at most are resident; a run with more steps cycles through them, and a view met again would find the ray
    # order / tile order the pipeline keyed on its tensors: the per-ray caches are dropped at every wrap, so that a
    # re-used view is traced like a new one -- ADVICE r5)
    view_of_step = (lambda i: fresh[i % len(fresh)]) if fresh else (lambda i: view0)

    def forget_rays_at_wrap(i):
        if fresh and i >= len(fresh) and i % len(fresh) == 0 and on_gpu:
            pipe._order = None
            pipe._trail = None
            pipe._tile_sets.clear()
            pipe._tiles = None

    def step(record, view):
        rays, start = view["rays"], view["start"]
        if W["kind"] == "render":
            # benchmark.py's loop: the foam is static, the packed tables are cached after the first frame
            e0, e1 = ev(), ev()
            if record:
                e0.record()
            pipe.trace_benchmark(points, attributes, adjacency, offsets, render_diff, view["cam"], view["cam_start"],
                                 render_out, weight_threshold=0.05)
            if record:
                e1.record()
                fwd_ev.append((e0, e1))
            return
        # points / attributes are "updated by the optimizer" every step while the triangulation stays (the
        # reference rebuilds it every ~100 iterations): the geometry half of the packed foam is rebuilt once
        # per step; links and padded offsets, which depend on the adjacency alone, are kept
        if on_gpu:
            pipe._cache.invalidate_geometry()
        ep, e0, e1, e2, e3 = ev(), ev(), ev(), ev(), ev()
        if record:
            ep.record()
        if on_gpu:
            pipe.prepare_foam(points, attributes, adjacency, offsets)
        if record:
            e0.record()
        if strong:
            out = tracer.forward(points, attributes, adjacency, offsets, rays, start, depth_quantiles=quantiles)
        else:
            out = pipe.trace_forward(points, attributes, adjacency, offsets, rays, start, depth_quantiles=quantiles)
        if record:
            e1.record()
        res = None
        if not W["forward_only"]:
            if strong:
                g_local = rdist.shard_rows(grad_rgba, rank, world, bounds=tracer.bounds)
                res = tracer.pipeline.trace_backward(points, attributes, adjacency, offsets, tracer._shard(rays),
                                                     tracer._shard(start), out["rgba"], g_local,
                                                     tracer._shard(quantiles), out.get("depth_indices"),
                                                     tracer._shard(depth_grad))
            else:
                res = pipe.trace_backward(points, attributes, adjacency, offsets, rays, start, out["rgba"], grad_rgba,
                                          quantiles, out.get("depth_indices"), depth_grad)
            if record:
                e2.record()
            if world > 1:
                if tracer.sparse is not None:
                    tracer.sparse.reduce(res)
                else:
                    rdist.all_reduce_gradients(res)
                if record:
                    e3.record()
        if record:
            pack_ev.append((ep, e0))
            fwd_ev.append((e0, e1))
            if res is not None:
                bwd_ev.append((e1, e2))
                if world > 1:
                    exch_ev.append((e2, e3))
        last["out"], last["res"] = out, res

    # ---- warm-up (untimed); the first warm-up step also measures the rows' cost for the row cut ----
    bounds = None
    for i in range(args.warmup):
        step(False, view_of_step(i))
        sync()   # lets the pipeline see the longest ray of the batch before the next step sizes its hop trail
        if i == 0 and strong and W["kind"] == "image" and not args.no_rebalance:
            bounds = tracer.rebalance(last["out"]["num_intersections"], rays.shape[0])
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        forget_rays_at_wrap(args.warmup + i)
        step(True, view_of_step(args.warmup + i))
    sync()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        if W["kind"] == "render":
            dumped = [("rgba8", render_out, 2)]
        else:
            lead = last["out"]["rgba"].dim() - 1      # leading dims that index rays
            dumped = [(k, last["out"][k], lead) for k in ("rgba", "num_intersections", "depth", "depth_indices")
                      if k in last["out"]]
            if last["res"] is not None:     # (ray_grad is returned zero-filled: nothing to compare)
                dumped += [(k, last["res"][k], 1) for k in ("points_grad", "attr_grad")]
        dump_outputs(args.dump_outputs, dumped)

    mean_ms = lambda evs: float(np.mean([a.elapsed_time(b) for a, b in evs])) if (evs and on_gpu) else 0.0
    fwd_ms, bwd_ms, pack_ms, exch_ms = mean_ms(fwd_ev), mean_ms(bwd_ev), mean_ms(pack_ev), mean_ms(exch_ev)

    # per-rank kernel times (for the N>1 line: how well the row cut balanced the ranks)
    rank_ms = None
    if world > 1:
        mine = torch.tensor([fwd_ms, bwd_ms, exch_ms, pack_ms], dtype=torch.float64, device=dev)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rank_ms = [[round(float(x), 4) for x in r.tolist()] for r in allr]

    # ---- the same steps on ONE frame / batch traced over and over (untimed for the metric): what rounds 1-4 reported as
    # the value.  A repeated frame takes its forward's block order from its own previous trace.  Also leaves view 0's
    # outputs in `last` for the extras and checks below.
    repeated = None
    if args.full and fresh and on_gpu and not args.no_repeated_frame:
        timed_fwd, timed_bwd, timed_pack = list(fwd_ev), list(bwd_ev), list(pack_ev)
        del fwd_ev[:], bwd_ev[:], pack_ev[:], exch_ev[:]
        for _ in range(2):
            step(False, view0)
            sync()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step(True, view0)
        sync()
        rep = (time.perf_counter() - t1) / args.steps
        repeated = {"ms_per_step": round(rep * 1e3, 4), "forward_ms": round(mean_ms(fwd_ev), 4),
                    "backward_ms": round(mean_ms(bwd_ev), 4)}
        fwd_ev[:], bwd_ev[:], pack_ev[:] = timed_fwd, timed_bwd, timed_pack
    elif args.full and fresh:
        step(False, view0)
        sync()

    local_rays = (last["out"]["rgba"].numel() // 4) if last.get("out") is not None else frame_rays
    total_rays = frame_rays if (strong or world == 1) else frame_rays * world
    ms_per_step = elapsed / args.steps * 1e3
    value = total_rays / (elapsed / args.steps) / 1e6

    # ---- untimed extras: exact walk counters, compulsory-traffic floor, full pack -----------------
    detail = {"forward_ms": round(fwd_ms, 4), "backward_ms": round(bwd_ms, 4), "foam_pack_ms": round(pack_ms, 4),
              "setup_seconds": round(setup_s, 1), "foam_csr": fm["csr_source"]}
    # the scheduling of the launches' blocks, learnt in the warm-up steps from the step counts of the walk itself
    mode_name = getattr(pipe, "tile_order_mode", None) or "static"
    if mode_name == "auto":
        detail["tile_order"] = ("repeated frame: forward / render launches take the block order learnt on the previous trace "
                                "of the same rays, the backward the one its forward learnt" if not fresh else
                                "rays new in every step: forward / render launches run under the static dealing of tiles, "
                                "the backward under the order its own forward learnt (cheapest tiles last)")
    else:
        detail["tile_order"] = mode_name
    detail["rays"] = "one frame / batch traced over and over (--repeat-frame)" if not fresh else \
        f"new in every step ({len(fresh)} views resident: " + \
        ("a shuffled batch per step" if W["kind"] == "batch" else f"a camera path, {VIEW_STEP_DEGREES} degrees per step") + \
        ("" if args.warmup + args.steps <= len(fresh) else
         f"; {args.warmup + args.steps} steps cycle through them, the pipeline's per-ray caches dropped at every wrap") + ")"
    if repeated is not None:
        total = frame_rays if (strong or world == 1) else frame_rays * world
        repeated["value"] = round(total / (repeated["ms_per_step"] * 1e-3) / 1e6, 3)
        detail["value_repeated_frame"] = repeated["value"]
        detail["repeated_frame"] = repeated
    detail.update(tri_ms)
    if world > 1:
        detail["exchange_ms"] = round(exch_ms, 4)
        detail["per_rank_ms_fwd_bwd_exchange_pack"] = rank_ms
        detail["row_bounds"] = bounds
        detail["exchange"] = exchange if (tracer.sparse is None or tracer.sparse.last_counts is not None) else \
            "sparse requested; lists covered more than dense_fraction of the points, fell back to the dense all-reduce"
        if tracer.sparse is not None and tracer.sparse.last_counts is not None:
            pitch = tracer.sparse._pitch(A)
            detail["exchange_rows_per_rank"] = tracer.sparse.last_counts
            detail["exchange_bytes_in_per_rank"] = int((world - 1) * max(tracer.sparse.last_counts) * pitch * 4)
            detail["dense_allreduce_bytes_per_rank"] = int(2 * (world - 1) / world * points.shape[0] * (3 + A) * 4)
    if args.full and on_gpu and world == 1 and args.workload == "north-star" and not W.get("custom"):
        # what train.py:243-248 does between steps: the triangulation follows the points.  Untimed extra, beside the
        # metric: the foam's own lists rebuilt on the GPU from scratch (and compared with the lists the frame was traced
        # through: Qhull's, when they came from the cache), then an incremental rebuild after a 3 %-of-the-spacing move.
        from radfoam_amd import triangulation

        def timed_ms(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(dev)
            return out, (time.perf_counter() - t0) * 1e3

        triangulation.delaunay_adjacency(points)   # warm-up (module load, allocator)
        tree, tree_ms = timed_ms(lambda: triangulation.build_aabb_tree(points))
        (t_adj, t_off, t_stats), full_ms = timed_ms(lambda: triangulation.delaunay_adjacency(points, tree))
        g = torch.Generator(device=dev).manual_seed(7)
        moved = points + 0.03 * (8.0 / points.shape[0]) ** (1.0 / 3.0) * torch.randn(points.shape, device=dev, generator=g)
        tree2 = triangulation.build_aabb_tree(moved)
        (m_adj, m_off, _), inc_ms = timed_ms(lambda: triangulation.delaunay_adjacency(moved, tree2, (t_adj, t_off)))
        detail["triangulation"] = {
            "points": int(points.shape[0]), "aabb_tree_ms": round(tree_ms, 3), "from_scratch_ms": round(full_ms, 1),
            "incremental_ms": round(inc_ms, 1),
            "equals_traced_lists": bool(torch.equal(t_adj.view(torch.int32), adjacency.view(torch.int32)) and
                                        torch.equal(t_off.view(torch.int32), offsets.view(torch.int32))),
            "traced_lists_from": fm["csr_source"], "second_pass_stars": t_stats["large_stars"],
            "tree_nodes_per_point": round(t_stats["tree_nodes_visited"] / points.shape[0], 1),
            "lists_changed_by_the_move": bool(m_adj.numel() != t_adj.numel() or
                                              not torch.equal(m_adj.view(torch.int32), t_adj.view(torch.int32))),
        }
        del tree, tree2, t_adj, t_off, m_adj, m_off, moved
    roofline = None
    if args.full and on_gpu and rank == 0:
        my_rays = tracer._shard(rays) if strong else rays
        my_start = tracer._shard(start) if strong else start
        is_render = W["kind"] == "render"
        cbytes = 2 if attr_dtype == torch.float16 else 4
        # render: the camera's rays through the statistics instance of trace_forward (same walk, same threshold; the
        # render kernel itself casts them from the camera and keeps no counters)
        stats = pipe.walk_statistics(points, attributes, adjacency, offsets, my_rays, my_start, visit_marks=True,
                                     weight_threshold=0.05 if is_render else None)
        visited = stats.pop("visited")
        bytes_fwd, bytes_bwd = algorithmic_bytes(stats, local_rays, A, c=cbytes, nq=nq, render=is_render)
        deg = (offsets[1:].to(torch.int64) - offsets[:-1].to(torch.int64))
        padded = (deg + 3) // 4 * 4
        n_vis = int(visited.sum())
        lit = visited & (attributes[:, -1] > 1e-6)
        sh_bytes = cbytes * (A - 1) * int(lit.sum())
        trail_bytes = 4 * stats["hops"] + 4 * local_rays if not W["forward_only"] else 0
        per_ray_io = 4 if is_render else (24 + 4 + 4 * cbytes + 4)    # render: camera by value, one RGBA8 word out
        comp_fwd = 16 * n_vis + 6 * int(padded[visited].sum()) + 12 * n_vis + sh_bytes + local_rays * per_ray_io \
            + trail_bytes
        comp_bwd = None
        if last.get("res") is not None:
            res = last["res"]
            if world == 1:
                touched = int(((res["points_grad"] != 0).any(dim=1) | (res["attr_grad"] != 0).any(dim=1)).sum())
            else:
                touched = None
            if touched is not None:
                comp_bwd = 16 * n_vis + sh_bytes + trail_bytes + local_rays * (24 + 4 + 16 + 16) + touched * (3 + A) * 4
        pipe._cache.clear()
        ef0, ef1 = ev(), ev()
        ef0.record()
        pipe.prepare_foam(points, attributes, adjacency, offsets)
        ef1.record()
        torch.cuda.synchronize()
        detail.update({
            "foam_full_pack_ms": round(float(ef0.elapsed_time(ef1)), 4),
            "algorithmic_bytes_fwd": int(bytes_fwd), "algorithmic_bytes_bwd": int(bytes_bwd),
            "walk": stats, "distinct_cells_visited": n_vis,
            "mean_cells_per_ray": round(stats["cells_scanned"] / max(local_rays, 1), 2),
            "mean_faces_per_cell": round(stats["faces_scanned"] / max(stats["cells_scanned"], 1), 2),
        })
        roofline = build_roofline(W, world, fwd_ms, bwd_ms, bytes_fwd, bytes_bwd, comp_fwd, comp_bwd, stats)

    if rank != 0:
        return None

    mode = "forward only" if W["forward_only"] else "forward+backward"
    if W["kind"] == "image":
        shape = f"{W['height']}x{W['width']} pinhole frame"
    elif W["kind"] == "render":
        shape = f"{W['height']}x{W['width']} trace_benchmark frame, fp16 attributes, weight_threshold 0.05"
    else:
        shape = f"{W['rays']} shuffled rays from 8 cameras"
    if world == 1:
        par = "1 GPU"
    elif strong:
        par = (f"the frame's rows cut into {world} contiguous blocks of equal measured cost, foam replicated, "
               f"{exchange} gradient exchange") if W["kind"] == "image" else \
              f"the batch split by index over {world} GPUs, foam replicated, dense all-reduce"
    else:
        par = f"one frame per GPU ({world} frames), foam replicated" + ("" if W["forward_only"] else ", dense all-reduce")
    metric = "Mrays/s fwd+bwd @1080p, 2M-pt foam; achieved HBM GB/s vs peak" if W["name"] == "north-star" and not \
        W.get("custom") and not W["forward_only"] and not nq else f"Mrays/s {mode}, {W['label']}" + \
        (f", {nq} depth quantiles per ray" if nq else "")
    result = {
        "metric": metric,
        "value": round(value, 3),
        "unit": "Mrays/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak" if (world > 1 and not strong) else "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": f"{W['label']}: synthetic {W['points']}-point foam (seed {W['seed']}), SH degree {sh_degree} "
                        f"(A={A}), {'fp16' if attr_dtype == torch.float16 else 'fp32'} attrs, {shape}, {mode}"
                        + (f", {nq} depth quantiles per ray with depth gradients (as train.py:176-180)" if nq else ""),
            "num_points": W["points"], "sh_degree": sh_degree, "rays_per_step": total_rays,
            "weight_threshold": 0.05 if W["kind"] == "render" else 1e-3, "max_intersections": 1024,
            "parallelism": par,
            "backward_mode": args.backward_mode,
        },
        "detail": detail,
    }
    if W["kind"] == "render":
        result["detail"]["frames_per_second"] = round(1e3 / ms_per_step * (world if world > 1 else 1), 2)
    if roofline is not None:
        result["roofline"] = roofline
    if not on_gpu:
        result["data"] = "synthetic (launcher self-test on CPU tensors through " + test_factory + ": not a measurement)"

    # ---- CPU baseline: the oracle on a bounded sample of the same rays --------------------------
    if args.full and on_gpu and not args.no_cpu_baseline and world == 1:
        try:
            if W["kind"] == "render":
                result["cpu_baseline"] = cpu_baseline_render(W, fm, cam, start_np, render_out, args.strict_scan)
            else:
                result["cpu_baseline"] = cpu_baseline(args, W, pipe, fm, rays_np, start_np, last, grad_rgba,
                                                      (points, attributes, adjacency, offsets), quantiles, depth_grad)
        except Exception as exc:  # the baseline must never take the bench line down
            result["cpu_baseline"] = {"error": repr(exc)}
    return result


def build_roofline(W, world, fwd_ms, bwd_ms, bytes_fwd, bytes_bwd, comp_fwd, comp_bwd, walk=None):
    """What bounds the walk kernels, from numbers that bound something (judge's review of round 1):

    * ``valu_issue`` -- the kernels are instruction-issue bound: busy fraction of the VALU issue slots
      = 4 * SQ_ACTIVE_INST_VALU (quad-cycles) / (1024 SIMDs * GRBM_GUI_ACTIVE / 8 cycles), both from the same
      rocprofv3 pass of this workload committed under profiles/ (profiles/counters.json names the files);
    * ``hbm`` -- measured traffic (PMC FETCH_SIZE / WRITE_SIZE passes, gfx950 correction per the guide) over the
      live launch time, against the 8.0 TB/s spec and the 6.29 TB/s achievable peak, and against the compulsory
      floor (every distinct cell record, face list and colour row the frame touches read once + rays + outputs
      + the hop trail): measured / floor is the re-read factor;
    * ``algorithmic_GBps`` -- SURVEY 8(d)'s logical bytes (no cache credit) / launch time: a throughput that
      may exceed the HBM peak because the walk is served from L1/L2, NOT a fraction of anything.
    """
    counters = load_counters(W["name"], W.get("custom") or W.get("nq")) if world == 1 else None
    stale = bool(counters and counters.get("stale"))
    if stale:
        # profiles/counters.json was measured on other kernel sources than the ones that just ran: nothing derived from
        # it is quoted (frac = null); the live figures (launch times, algorithmic and compulsory bytes) stay
        counters = {"source": counters.get("source"), "kernels": {}}
    per_kernel = {}
    isa, isa_why = isa_constants()
    legs = [("forward_kernel", fwd_ms, bytes_fwd, comp_fwd)]
    if bwd_ms > 0:
        bwd_name = "backward_replay_direct_kernel" if W["kind"] == "batch" else "backward_replay_cached_kernel"
        legs.append((bwd_name, bwd_ms, bytes_bwd, comp_bwd))
    for name, ms, alg, comp in legs:
        k = {"avg_launch_ms": round(ms, 4), "algorithmic_bytes_per_launch": int(alg),
             "algorithmic_GBps": round(alg / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
             "compulsory_bytes_per_launch": int(comp) if comp is not None else None}
        if name == "forward_kernel" and walk and ms > 0 and isa:   # live: the scan's arithmetic over the launch time
            tf = isa["scan_flop_per_4_faces"] / 4.0 * walk["faces_scanned"] / (ms * 1e-3) / 1e12
            k["scan_fp32_TFLOPs"] = round(tf, 2)
            k["fp32_frac_of_peak"] = round(tf / FP32_VECTOR_PEAK_TFLOPS, 4)
        c = (counters or {}).get("kernels", {}).get(name)
        if c:
            if c.get("SQ_ACTIVE_INST_VALU") and c.get("GRBM_GUI_ACTIVE"):
                cycles = c["GRBM_GUI_ACTIVE"] / NUM_XCDS          # shader-clock cycles of the launch
                k["valu_issue_frac"] = round(4.0 * c["SQ_ACTIVE_INST_VALU"] / (NUM_SIMDS * cycles), 4)
                k["valu_insts_per_launch"] = int(c.get("SQ_INSTS_VALU", 0))
                k["effective_clock_GHz_profiled"] = round(cycles / c["duration_ns"], 3) if c.get("duration_ns") else None
                if name == "forward_kernel" and walk and c.get("SQ_INSTS_VALU") and isa:
                    scan = isa["scan_valu_per_4_faces"] / 4.0 * walk["faces_scanned"] / 64.0
                    k["useful_scan_valu_frac"] = round(scan / c["SQ_INSTS_VALU"], 4)   # the face tests alone
                    k["useful_scan_share_of_issue_capacity"] = round(k["useful_scan_valu_frac"] * k["valu_issue_frac"], 4)
                    if W["sh"] == 2:      # hop / segment counts are those of the SH-degree-2 fp32 instance
                        useful = scan + (isa["hop_valu_per_lane"] * walk["hops"] +
                                         isa["composite_valu_per_lane"] * walk["segments_lit"]) / 64.0
                        k["useful_valu_frac"] = round(useful / c["SQ_INSTS_VALU"], 4)
                        k["useful_share_of_issue_capacity"] = round(k["useful_valu_frac"] * k["valu_issue_frac"], 4)
            if c.get("hbm_bytes") is not None and ms > 0:
                gbps = c["hbm_bytes"] / (ms * 1e-3) / 1e9
                k["hbm_bytes_per_launch"] = int(c["hbm_bytes"])
                k["hbm_measured_GBps"] = round(gbps, 1)
                k["hbm_frac_of_spec_peak"] = round(gbps / HBM_PEAK_SPEC_GBS, 4)
                k["hbm_frac_of_measured_peak"] = round(gbps / HBM_PEAK_MEASURED_GBS, 4)
                if comp:
                    k["hbm_traffic_over_compulsory"] = round(c["hbm_bytes"] / comp, 3)
        per_kernel[name] = k
    dom = max(legs, key=lambda l: l[1])[0]
    d = per_kernel[dom]
    # which limit the dominant kernel actually sits at: VALU issue (the image-shaped walks), HBM (the gathers of a
    # sparse batch's forward), or neither -- the direct-atomics backward of sparse batches waits on the memory-side
    # atomic units and on dependent gathers with both fractions low; it is labelled as what it is
    vf, hf = d.get("valu_issue_frac"), d.get("hbm_frac_of_measured_peak")
    if vf is None and hf is None:
        bound = None                  # no committed counters for this workload (or stale ones): nothing is assumed
    elif (vf or 0.0) >= 0.7 and (vf or 0.0) >= (hf or 0.0):
        bound = "valu_issue"
    elif (hf or 0.0) >= 0.5:
        bound = "hbm"
    else:
        # (a kernel whose issue slots are half busy is not issue-bound: the flat-batch replay at 0.51 waits in its serial
        # row emission and its LDS compare-and-swap rounds)
        bound = "latency (serial row emission / LDS and memory-side atomics / dependent gathers): neither VALU issue nor HBM bandwidth is near its peak"
    frac = hf if bound == "hbm" else vf
    out = {
        "bound": bound,
        "kernel": dom,
        "achieved": (d.get("hbm_measured_GBps") if bound == "hbm" else vf),
        "peak": (None if bound is None else HBM_PEAK_MEASURED_GBS if bound == "hbm" else 1.0),
        "unit": ("GB/s of measured HBM traffic against the achievable 6290 GB/s" if bound == "hbm" else
                 "fraction of VALU issue cycles busy = 4*SQ_ACTIVE_INST_VALU quad-cycles / (1024 SIMDs * GRBM_GUI_ACTIVE/8 cycles)"),
        "frac": frac,
        "traffic": d.get("hbm_bytes_per_launch"),
        "avg_launch_ms": d["avg_launch_ms"],
        "hbm": {"measured_GBps": d.get("hbm_measured_GBps"), "frac_of_spec_peak_8000": d.get("hbm_frac_of_spec_peak"),
                "frac_of_measured_peak_6290": d.get("hbm_frac_of_measured_peak"),
                "compulsory_bytes_per_launch": d.get("compulsory_bytes_per_launch"),
                "traffic_over_compulsory": d.get("hbm_traffic_over_compulsory")},
        "algorithmic_GBps": d["algorithmic_GBps"],
        "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"],
        "kernels": per_kernel,
        "counters_source": (counters or {}).get("source"),
        "counters_stale": stale,
        "isa_constants": isa if isa else {"unusable": isa_why},
        "useful_valu_frac": per_kernel.get("forward_kernel", {}).get("useful_valu_frac"),
        "useful_scan_valu_frac": per_kernel.get("forward_kernel", {}).get("useful_scan_valu_frac"),
        "fp32_frac_of_peak": per_kernel.get("forward_kernel", {}).get("fp32_frac_of_peak"),
        "note": ("no committed hardware counters describe this workload on these kernel sources: bound / achieved / frac "
                 "/ traffic are null; avg_launch_ms, algorithmic and compulsory figures are live." if bound is None else
                 "achieved / frac / traffic come from the committed rocprofv3 --pmc passes of this same workload on these "
                 "same kernel sources (counters_source); avg_launch_ms, algorithmic and compulsory figures are live.  "
                 "The image-shaped walks are served from L1/L2 and bound by VALU issue, not by HBM (DESIGN.md section 4)."),
    }
    return out


def cpu_baseline(args, W, pipe, fm, rays_np, start_np, last, grad_rgba, foam_dev, quantiles=None, depth_grad=None):
    """Oracle (kind 'port') on a strided sample of the same rays, all host cores; the sample's rgba must equal
    the GPU's bit for bit and its gradients must match a HIP backward of the same sample within the north
    star's 1e-3 (per element, tests/helpers.grad_close) -- over the WHOLE frame when the sample is the frame."""
    import torch
    from oracle import oracle as O
    from tests.helpers import grad_close

    sh_degree = W["sh"]
    cores = len(os.sched_getaffinity(0))      # every logical core this process may run on: one OpenMP thread each
    image = W["kind"] == "image"
    diff = O.build_adjacent_diff(fm["points"], fm["point_adjacency"], fm["point_adjacency_offsets"], pad=32)
    foam_args = (sh_degree, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    g_np = grad_rgba.cpu().numpy()
    q_np = None if quantiles is None else quantiles.cpu().numpy()
    dg_np = None if depth_grad is None else depth_grad.cpu().numpy()
    total = rays_np.size // 6

    def sample(stride):
        if image:
            sl = (slice(None, None, stride), slice(None, None, stride))
        else:
            sl = (slice(None, None, stride * stride),)
        cut = lambda a: None if a is None else np.ascontiguousarray(a[sl])
        return cut(rays_np), cut(start_np), cut(g_np), sl, cut(q_np), cut(dg_np)

    contested = {}

    def run(stride):
        r, s, g, sl, q, dg = sample(stride)
        # the scan evaluated the way the kernels evaluate it (tournament on products + certificate + dividing fallback:
        # the same function as the reference's evaluation, tests/test_oracle.py, and twice as fast on these cores)
        with O.scan_mode("filtered") as mode:
            t0 = time.perf_counter()
            f = O.trace_forward(*foam_args, r, s, depth_quantiles=q, diff=diff, num_threads=cores)
            t1 = time.perf_counter()
            contested["cells"] = mode.contested      # cells whose certificate failed (the dividing scan decided)
            contested["scans"] = int(f["num_intersections"].sum())
            b = None
            if not W["forward_only"]:
                b = O.trace_backward(*foam_args, r, s, f["rgba"], g, depth_quantiles=q,
                                     depth_indices=f.get("depth_indices"), depth_grad_in=dg, diff=diff, num_threads=cores)
            t2 = time.perf_counter()
        return r.size // 6, t1 - t0, t2 - t1, f, b, (r, s, g, sl, q, dg)

    stride = 24
    # one thread per logical core, or one per physical core pair: whichever the pilot sample finishes sooner
    n, tf, tb, f, b, smp = run(stride)
    n, tf, tb, f, b, smp = run(stride)          # (the first pass pays for thread start-up and page faults)
    if cores >= 4:
        full = cores
        cores = full // 2
        n2, tf2, tb2, f2, b2, smp2 = run(stride)
        if tf2 + tb2 < tf + tb:
            n, tf, tb, f, b, smp = n2, tf2, tb2, f2, b2, smp2
        else:
            cores = full
    for _ in range(2):   # the pilot is dominated by thread start-up: size the sample in two passes
        if tf + tb >= 0.6 * args.cpu_seconds or stride == 1:
            break
        rate = n / max(tf + tb, 1e-6)
        want = max(n, int(rate * args.cpu_seconds))
        new_stride = max(1, int(math.sqrt(total / want)))
        if new_stride >= stride:
            break
        stride = new_stride
        n, tf, tb, f, b, smp = run(stride)
    r, s, g, sl, q, dg = smp
    gpu_rgba = last["out"]["rgba"].cpu().numpy()[sl]
    same = bool(np.array_equal(f["rgba"].view(np.uint32), gpu_rgba.view(np.uint32)))
    if q is not None:   # depths and the cells they fall in are forward outputs too: bit for bit
        same = same and bool(np.array_equal(f["depth"].view(np.uint32), last["out"]["depth"].cpu().numpy()[sl].view(np.uint32)))
        same = same and bool(np.array_equal(f["depth_indices"].view(np.uint32).reshape(-1),
                                            last["out"]["depth_indices"].cpu().numpy()[sl].view(np.uint32).reshape(-1)))
    # The timed comparison above runs the oracle's "filtered" mode -- the CPU mirror of the kernels' own evaluation.  The
    # link to the reference's LITERAL loop (every face divided, running minimum of the rounded quotients) is made here as
    # well, untimed: a forward of at least every 3rd row and column (11 %) of the same frame / every 9th ray of the batch,
    # more when the cores are fast enough, in the oracle's default mode against the same GPU output (VERDICT r5 weak #1b).
    literal = None
    try:
        per_ray = tf / max(n, 1) * 2.0                    # the literal loop is about twice the filtered one on these cores
        lit_stride = next((k for k in (1, 2, 3) if per_ray * total / (k * k) <= 8.0), 3)
        r_l, s_l, _, sl_l, q_l, _ = sample(lit_stride)
        t_l = time.perf_counter()
        f_l = O.trace_forward(*foam_args, r_l, s_l, depth_quantiles=q_l, diff=diff, num_threads=cores)
        t_l = time.perf_counter() - t_l
        gpu_l = last["out"]["rgba"].cpu().numpy()[sl_l]
        same_l = bool(np.array_equal(f_l["rgba"].view(np.uint32), gpu_l.view(np.uint32)))
        if last["out"].get("num_intersections") is not None:
            same_l = same_l and bool(np.array_equal(f_l["num_intersections"].reshape(-1),
                                                    last["out"]["num_intersections"].cpu().numpy()[sl_l].view(np.uint32).reshape(-1)))
        n_l = r_l.size // 6
        literal = {"scan": "the reference's loop as written (tracing_utils.cuh:43-67): every face divided, strict '<' on the "
                           "rounded quotients -- oracle scan_cell_reference, the oracle's default mode",
                   "rays": int(n_l), "share_of_the_step": round(n_l / total, 4),
                   "sample": "the whole frame / batch" if lit_stride == 1 else
                             (f"every {lit_stride}th row and column" if image else f"every {lit_stride * lit_stride}th ray"),
                   "matches_gpu_bitwise": same_l, "seconds": round(t_l, 2)}
    except Exception as exc:  # noqa: BLE001
        literal = {"error": repr(exc)}
    out = {
        "value": round(n / (tf + tb) / 1e6, 5),
        "unit": "Mrays/s",
        "cores": cores,
        "kind": "port",
        "sample": (f"every {stride}th row and column of the same frame" if image else f"every {stride * stride}th ray of the same batch")
                  + f" ({n} rays = {100.0 * n / total:.1f}% of the step), oracle/rf_oracle.c with OpenMP on {cores} threads "
                    f"(every logical core this process may use; the box has {os.cpu_count()}), rays dealt to the threads in "
                    f"chunks of 64, gradients summed in thread-local write-combining tables merged at the end (no atomic "
                    f"in the walk, BASELINE.md section 3), the scan evaluated as the kernels evaluate it; forward {tf:.2f}s"
                  + ("" if b is None else f" + backward {tb:.2f}s") + "; fp16 face table prebuilt (excluded)",
        "matches_gpu_bitwise": same,
        "matches_gpu_bitwise_scan_mode": "filtered: the oracle's mirror of the kernels' evaluation (tournament on products, "
                                         "certificate, fail-safe, dividing fallback) -- the timed run",
        "literal_reference_scan": literal,
        # how often the filtered scan's certificate fails on this workload (the same evaluation the kernels run)
        "scan_contested_cells": contested.get("cells"), "scan_cells": contested.get("scans"),
        "scan_contested_rate": (round(contested["cells"] / max(contested["scans"], 1), 7) if contested else None),
    }
    try:
        env = reference_source_envelope(W, fm)
        if env is not None:
            out["reference_source_envelope"] = env
    except Exception as exc:  # noqa: BLE001  (context, never the bench line's fate)
        out["reference_source_envelope"] = {"error": repr(exc)}
    if b is not None:
        if stride == 1:
            res = last["res"]          # the gradients of the last timed step: the whole frame
            where = "whole frame, the last timed step's gradients"
        else:
            dev = foam_dev[0].device
            tr, ts = torch.from_numpy(r).to(dev), torch.from_numpy(s).to(dev)
            tq = None if q is None else torch.from_numpy(q).to(dev)
            tdg = None if dg is None else torch.from_numpy(dg).to(dev)
            fo = pipe.trace_forward(*foam_dev, tr, ts, depth_quantiles=tq)
            res = pipe.trace_backward(*foam_dev, tr, ts, fo["rgba"], torch.from_numpy(g).to(dev), tq,
                                      fo.get("depth_indices"), tdg)
            where = "a HIP forward+backward of the same sampled rays and upstream gradients"
        out["grad_checked_on"] = where
        for key in ("points_grad", "attr_grad"):
            ok, rel, worst = grad_close(res[key].cpu().numpy(), b[key])
            out[f"{key}_rel_l2"] = float(f"{rel:.3e}")
            out[f"{key}_within_1e-3"] = bool(ok)
    return out


def cpu_baseline_render(W, fm, cam, start_np, render_out, strict_scan=False):
    """The render path's CPU baseline: the oracle's restatement of the benchmark kernel (pipeline.cu:472-544 + cast_ray +
    make_rgba8) on the SAME camera, whole frame, all host cores; its RGBA8 words against the frame the GPU just wrote."""
    from oracle import oracle as O

    cores = len(os.sched_getaffinity(0))
    half_attrs = fm["attributes"].astype(np.float16)     # what benchmark.py feeds the fp16 pipeline (benchmark.py:36)
    diff = O.build_adjacent_diff(fm["points"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    start = np.uint32(np.asarray(start_np).reshape(-1)[0])
    with O.scan_mode("filtered"):
        t0 = time.perf_counter()
        ref = O.trace_benchmark(W["sh"], fm["points"], half_attrs, fm["point_adjacency"], fm["point_adjacency_offsets"],
                                diff, cam, start, weight_threshold=0.05, num_threads=cores)
        dt = time.perf_counter() - t0
    got = render_out.cpu().numpy().view(np.uint32).reshape(ref.shape)
    n = int(ref.size)
    differ = int((got != ref).sum())
    return {
        "value": round(n / dt / 1e6, 5), "unit": "Mrays/s", "cores": cores, "kind": "port",
        "sample": f"the whole {W['height']}x{W['width']} frame of the same camera ({n} pixels), oracle/rf_oracle.c "
                  f"rfo_trace_benchmark with OpenMP on {cores} threads of {os.cpu_count()} logical cores, {dt:.2f}s; "
                  "fp16 face table prebuilt (excluded), as the caller's is for the GPU",
        "frames_per_second": round(1.0 / dt, 3),
        "matches_gpu_bitwise": differ == 0,
        "rgba8_words_that_differ": differ,
    }


def reference_source_envelope(W, fm):
    """VERDICT r2 #1, outside every timed region: every 6th row and column of this frame through the reference's OWN
    kernel source compiled for the CPU without and with FMA contraction (oracle/_ref/libref.so, libref_fma.so: prebuilt
    in the build container by oracle/Makefile.ref, they travel with the snapshot) and through the oracle -- which the GPU
    output of this run equals bit for bit (matches_gpu_bitwise) --, forward and backward: rays on another path, rays
    beyond 1e-4 / 1e-5 in rgba, gradient distances overall / on same-path rays / carried by the flipped rays, the oracle
    against both builds next to the reference against itself (oracle/parity_envelope.py has the reasoning and the bar;
    profiles/r05/parity_baseline_scale.json the committed record)."""
    if W["kind"] != "image" or W.get("custom") or W.get("nq") or W["name"] not in ("north-star", "c2"):
        return None
    from oracle import parity_envelope as PE
    from oracle import refsrc as Rf

    if not (os.path.exists(Rf.LIB_PATH) and os.path.exists(Rf.LIB_PATH_FMA)):
        return None
    rec = PE.measure(fm, W["sh"], width=W["width"], height=W["height"], stride=6)
    rec["violations_of_the_bar"] = PE.check(rec)
    return rec


if __name__ == "__main__":
    main()
