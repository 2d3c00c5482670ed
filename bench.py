#!/usr/bin/env python
"""Headline benchmark: SDF (value + gradient) queries/sec -- BASELINE.json configs[1] ("C2"):
CachedSDF at 0.01 m voxels on the YCB power drill, 1M query points per GPU per step.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

One "step" = one pass of the hot path over one batch: a single `pvamd_cached_query` C-ABI call (one kernel launch)
over the rank's 1,048,576 resident query points, writing sdf_val [P] and sdf_grad [P,3].  Inputs are in HBM before
the timed region.  `--gpus N` with N > 1 and no torchrun environment re-launches itself as N ranks (one process per
GPU, RCCL); under torchrun it uses the ranks it was given.  The headline line is weak scaling (every rank its own
1M-point batch, no data-path collective); the `legs` object carries the configs BASELINE.json names for multi-GPU:
C4 (RobotSDF, 200 configurations x 262,144 points) strong-scaled over points with the results left sharded and with
the RCCL all-gather in the timed step, and C5 (chamfer, 2M points -> 99,500 triangles) with its B-float all-reduce.

The LAST stdout line (rank 0) is the contract line: compact JSON, < 4 KB (tests/test_bench_launch.py asserts the size),
built by `compact_line()` from the long record.  The long record (every leg's detail, latency percentiles, README legs) is
written to `bench_detail.json` (--detail PATH) and to stderr, never to the contract line.  `value` / `ms_per_step` are the
wall time of one timed region of exactly the K steps asked for.  `--dump-outputs DIR` writes what the last timed step
returned on rank 0 (sdf_val, sdf_grad) as DIR/<name>.npy; the inputs are seeded, so two builds compare output for output.
`roofline` is the dominant kernel (pvamd::cached_query_direct at 1M points), 28 B/query over its per-launch duration: `frac` is THIS run's (HIP events on the launch stream around a separate >= 2000-launch hipGraph of the
same call, so it does not depend on K); `frac_rocprof` is the committed rocprofv3 kernel-trace average of this command
(profiles/rNN_kernel_stats.json), `frac_wall` the contract's own timed region.  `cpu_baseline` = the restatements on the host cores.
"""
import argparse
import gc
import json
import os
import socket
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_legs import (BYTES_PER_QUERY, HBM_PEAK_GBS, LegSkipped, call_latency, capture_graph, graph_ms_per_launch, leg_c1,  # noqa: E402
                        leg_c3, leg_c4, leg_c5, leg_cache_build, leg_readme, build_robot, profile_path, time_calls, time_eager_kernel,
                        valu_model)

KERNEL_GRAPH_LAUNCHES = 2000
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all .npy files together, headers included


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--points", type=int, default=1 << 20, help="query points per GPU per step")
    ap.add_argument("--no-graph", action="store_true", help="time eager launches instead of one hipGraph of K steps")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-large", action="store_true", help="skip the secondary 64M-point (cache-exceeding) run")
    ap.add_argument("--no-legs", action="store_true", help="skip the C4 / C5 legs")
    ap.add_argument("--small-legs", action="store_true", help="functional test: C4 with 8 x 16,384 and C5 with 65,536 points")
    ap.add_argument("--cpu-seconds", type=float, default=4.0, help="wall budget of the CPU baseline samples (both figures)")
    ap.add_argument("--detail", default=os.path.join(ROOT, "bench_detail.json"), help="where rank 0 writes the long record")
    ap.add_argument("--latency-calls", type=int, default=20_000, help="calls per entry of the call-latency leg")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL over xGMI)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="functional test on a 1-GPU box: every rank uses cuda:0 and collectives go through gloo")
    ap.add_argument("--force-pg", action="store_true",
                    help="test hook: create the process group and run the gather / all-reduce legs even with ONE rank "
                         "(exercises the RCCL calls on a 1-GPU box)")
    ap.add_argument("--legs-deadline", type=float, default=420.0,
                    help="seconds after which a multi-rank run stops waiting for its legs: rank 0 prints the line with the legs "
                         "it has and every rank exits (a rank lost INSIDE a collective must not cost the headline)")
    ap.add_argument("--hang-rank", type=int, default=-1, help="test hook: this rank sleeps forever inside --fail-leg, after its gate")
    ap.add_argument("--fail-rank", type=int, default=-1, help="test hook: this rank raises while preparing --fail-leg")
    ap.add_argument("--fail-leg", default="", help="test hook: see --fail-rank")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write rank 0's outputs of the last one as DIR/<name>.npy (float32, <= 64 MB)")
    ap.add_argument("--launch-check", action="store_true",
                    help="no GPU work: start the ranks, all-reduce over gloo, print the rank count (CPU test of --gpus N)")
    return ap.parse_args()


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks_if_needed(args):
    """`python bench.py --gpus N` outside torchrun: become `torch.distributed.run --nproc-per-node N bench.py ...`."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this driver
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


def launch_check(args, rank, world):
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        t = torch.ones(1)
        dist.all_reduce(t)
        ranks = int(t.item())
        dist.destroy_process_group()
    else:
        ranks = 1
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "ranks_seen_by_all_reduce": ranks,
                          "gpus_requested": args.gpus}))


def dump_outputs(torch, np, directory, arrays):
    """--dump-outputs: `arrays` ({name: [P, ...] float32 tensor}, all with the same leading P) -> DIR/<name>.npy.  When they
    would exceed DUMP_LIMIT_BYTES together, every array keeps the same fixed, seeded sample of rows (ascending order)."""
    os.makedirs(directory, exist_ok=True)
    rows = next(iter(arrays.values())).shape[0]
    row_bytes = sum(a[:1].numel() * a.element_size() for a in arrays.values())
    keep = max(1, (DUMP_LIMIT_BYTES - 4096 * len(arrays)) // max(row_bytes, 1))
    index = None
    if rows > keep:
        index = torch.randperm(rows, generator=torch.Generator().manual_seed(0))[:keep].sort().values
    for name, a in arrays.items():
        host = a.detach().cpu()
        if index is not None:
            host = host[index]
        np.save(os.path.join(directory, name + ".npy"), host.numpy().astype(np.float32, copy=False))
    return {"dir": directory, "arrays": sorted(arrays), "rows": rows, "rows_written": rows if index is None else keep,
            "sample": None if index is None else "torch.randperm(rows, seed 0)[:rows_written], ascending"}


class Timer:
    """barrier + synchronize on both sides of the timed call; MAX over ranks; the device wait is an event-query spin
    followed by the synchronize (hipDeviceSynchronize alone adds tens of us of host wake-up to a ~0.1 ms region)."""

    def __init__(self, torch, dist, world):
        self.torch, self.dist, self.world = torch, dist, world

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()

    def __call__(self, fn):
        torch = self.torch
        done = torch.cuda.Event()
        self.barrier()
        torch.cuda.synchronize()
        # CPython's generation-2 collector walks torch's ~170k objects for 20-40 ms whenever its allocation counter trips
        # (profiles/r04_stall.txt): one such pass inside a 20-call timed region reads as 1 ms per call.  Not in the timed span.
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            t0 = time.perf_counter()
            fn()
            done.record()
            while not done.query():
                pass
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
        finally:  # a leg that raises inside the timed span must not leave the collector off for the legs after it
            if was_enabled:
                gc.enable()
        self.barrier()
        if self.world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            elapsed = t.item()
        return elapsed


def cpu_baseline(torch, np, cached, pts, seconds):
    """The reference's CPU path for this workload, restated (the reference cannot be imported: third-party packages absent), on
    the host cores with the threads pinned (OMP_PROC_BIND=close, OMP_PLACES=cores: set in main() before either runtime starts).
    `value` = `baseline_opforop`: the op-for-op torch restatement of sdf.py:535-571 (oracle/torch_opforop.py: the ~25 stock ops
    and their intermediates -- what a reference user runs on CPU); `baseline_fused` = the one-pass C / OpenMP restatement
    (oracle/pvamd_oracle.c), faster than anything the reference executes.  Each figure is the MEDIAN of 3 samples of whole
    passes; 60 % of the budget goes to the first, 40 % to the second.  Only reached after every GPU timing is done."""
    from oracle import oracle
    from oracle.torch_opforop import CachedOpForOp
    from tests import helpers as H
    og = H.oracle_grid_from_cached(cached)
    host_pts = pts.cpu().numpy()
    n_pts = len(host_pts)

    def samples(fn, budget, count=3):
        fn()  # warm: thread pools up, pages touched
        per, t0 = [], time.perf_counter()
        for _ in range(count):
            a, passes = time.perf_counter(), 0
            while passes == 0 or time.perf_counter() - a < budget / (count + 1):
                fn()
                passes += 1
            per.append(n_pts * passes / (time.perf_counter() - a))
        return float(np.median(per)), float(np.min(per)), float(np.max(per)), len(per), time.perf_counter() - t0

    packed = cached._packed.cpu()
    view = cached._view
    ref = CachedOpForOp(packed[:, 0].reshape(view.shape).contiguous(), packed[:, 1:4].contiguous(), view.min, view.max,
                        cached.bb.cpu())
    tp = pts.cpu()
    o_med, o_min, o_max, o_n, o_t = samples(lambda: ref(tp), seconds * 0.6)
    f_med, f_min, f_max, f_n, f_t = samples(lambda: oracle.cached_query(og, host_pts), seconds * 0.4)
    pin = {k: os.environ.get(k) for k in ("OMP_PROC_BIND", "OMP_PLACES", "OMP_NUM_THREADS")}
    return {"value": o_med, "unit": "queries/s", "cores": torch.get_num_threads(), "kind": "port",
            "baseline_opforop": o_med, "baseline_fused": f_med, "value_is": "baseline_opforop",
            "sample": f"median of {o_n} samples of whole passes over the same {n_pts} points, {o_t:.1f} s wall",
            "spread": {"min": o_min, "max": o_max, "samples": o_n},
            "host_cpus": os.cpu_count(), "thread_pinning": pin,
            "opforop_source": "oracle/torch_opforop.py (sdf.py:535-571 op for op, torch CPU)",
            "fused_port": {"value": f_med, "unit": "queries/s", "cores": oracle.num_threads(), "kind": "port",
                           "source": "oracle/pvamd_oracle.c (one fused pass per point, C + OpenMP)",
                           "sample": f"median of {f_n} samples of whole passes over {n_pts} points, {f_t:.1f} s wall",
                           "spread": {"min": f_min, "max": f_max, "samples": f_n}}}


def oracle_pins(np):
    """What the oracle is pinned to: the booleans tests/golden/make_golden.py wrote into the committed vectors (False = the
    vectors were generated over a shim of that third-party package, i.e. parity unpinned there)."""
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", "reference_lifted.npz"))
        return {k: bool(z[f"pinned/{k}"]) for k in ("view", "transform", "embree")}
    except Exception:
        return {"view": False, "transform": False, "embree": False}


class Gate:
    """Every leg calls its gate ONCE, after its set-up and before its first collective: one tiny all-reduce tells every rank
    whether all ranks got there.  A rank whose set-up raised reports that instead (main's handler), so the others skip the
    leg together rather than wait in a barrier for a rank that will never arrive."""

    def __init__(self, torch, dist, active):
        self.torch, self.dist, self.active, self.passed = torch, dist, active, False

    def agree(self, ok):
        if not self.active:
            return ok
        t = self.torch.tensor([1 if ok else 0], dtype=self.torch.int32, device="cuda")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return bool(t.item())

    def __call__(self):
        self.passed = True
        if not self.agree(True):
            raise LegSkipped()


def read_traffic(P):
    """HBM-side bytes per launch from the committed PMC passes (NOT measured in this run: rocprofv3 --pmc cannot run inside the
    benchmark); FETCH_SIZE x2 is the gfx950 correction of MI355X_MICROARCH.md."""
    path = profile_path("traffic.json")
    if path:
        try:
            tj = json.load(open(path))
            if tj.get("points") == P:
                return tj.get("hbm_bytes_per_launch"), f"profiles/{os.path.basename(path)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes)"
        except Exception:
            pass
    return None, None


def cached_query_kernel_name(P):
    """The kernel pvamd_cached_query launches for P points (csrc/cached.hip cq_kind, include/pvamd.h PVAMD_CQ_KERNEL_*)."""
    from pytorch_volumetric_amd import _lib
    names = {0: "pvamd::cached_query_scalar", 1: "pvamd::cached_query_direct<1 point per lane, 8 waves>",
             2: "pvamd::cached_query_direct<2 points per lane, 4 waves>", 3: "pvamd::cached_query_direct<2 points per lane, 16 waves>",
             4: "pvamd::cached_query_direct<4 points per lane, 4 waves>", 5: "pvamd::cached_query_wave",
             6: "pvamd::cached_query_wave (streaming)"}
    return names[int(_lib.load().pvamd_cached_query_kernel(P))]


def read_rocprof_kernel_us(P):
    """Average duration of the dominant kernel's launches at this point count in the committed rocprofv3 --kernel-trace of the
    driver-shaped command (tools/profile_bench.sh -> profiles/rNN_kernel_stats.json)."""
    path = profile_path("kernel_stats.json")
    try:
        row = json.load(open(path))["dominant"]
        if row.get("points") == P:
            return row["avg_us"], int(row["calls"]), f"profiles/{os.path.basename(path)}", row.get("by_context")
    except Exception:
        pass
    return None, None, None, None


# ------------------------------------------------------------------------------------------------ legs: C4 and C5
COMPACT_LIMIT = 4096  # bytes: the driver reads the tail of stdout; the contract line must fit it whole


def sig(x, digits=5):
    """floats to `digits` significant digits (the contract line carries numbers, not 17-digit reprs)"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        if x != x or x in (float("inf"), float("-inf")):
            return None
        return float(f"{x:.{digits}g}")
    if isinstance(x, dict):
        return {k: sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [sig(v, digits) for v in x]
    return x


def pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_leg(name, leg):
    """One number set per leg: ms_per_step, value, roofline.frac (+ the multi-rank facts of a gathered leg)."""
    if not isinstance(leg, dict):
        return None
    if "error" in leg or "skipped" in leg:
        return {"error": str(leg.get("error", "skipped"))[:80], **pick(leg, "ranks_without_a_result")}
    if name == "cache_build":
        return {k: {**pick(b, "ms", "gpu_ms", "value", "frac_8d", "exact_pairs"),
                    **({"util_valu": b["roofline"]["util_valu"]} if isinstance(b.get("roofline"), dict) and b["roofline"].get("util_valu") else {})}
                for k, b in leg.get("builds", {}).items()}
    if name.startswith("readme"):
        return pick(leg, "ms_per_call", "configure_plus_query_graph_ms", "published_ms")
    body = leg.get("sharded", leg)
    out = pick(body, "ms_per_step", "value", "frac_8d", "prepared_sorted_ms", "prepared_caller_ms")
    roof = body.get("roofline")
    if isinstance(roof, dict) and roof.get("util_valu") is not None:
        out["util_valu"] = roof["util_valu"]
    if "exact_pairs_per_step" in body:
        out["exact_pairs_per_step"] = body["exact_pairs_per_step"]
    g = leg.get("gathered")
    if isinstance(g, dict) and "self_check" in g:
        c = g["self_check"]
        out["gathered"] = {"ranks": c["ranks"], "backend": c["backend"], "bytes_received_per_rank": g["bytes_received_per_rank"],
                           "kernel_only_ms": c["kernel_only_ms"], "gathered_ms": c["gathered_ms"],
                           "equals_unsharded_call": g["equals_unsharded_call"], "ok": c["ok"]}
    gc_ = leg.get("gathered_by_configs")
    if isinstance(gc_, dict):
        out["gathered_by_configs_ms"] = gc_.get("ms_per_step")
    if leg.get("collective"):
        out["collective"] = leg["collective"][:60]
    if "rel_err_vs_analytic" in leg:
        out["rel_err_vs_analytic"] = leg["rel_err_vs_analytic"]
    return out


def compact_line(d, detail_name):
    """The contract line (the task's bench contract) from the long record `d`."""
    roof, cfg = d["roofline"], d["config"]
    line = pick(d, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data")
    line["config"] = pick(cfg, "workload", "points_per_gpu", "oob_fraction", "ranks", "backend", "gather", "launch")
    line["roofline"] = pick(roof, "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "kernel",
                            "launch_us", "launch_source", "frac_rocprof", "frac_wall", "copy_same_bytes_us")
    cpu = d.get("cpu_baseline")
    if cpu:
        line["cpu_baseline"] = pick(cpu, "value", "unit", "cores", "kind", "sample", "host_cpus", "baseline_opforop", "baseline_fused")
        line["cpu_baseline"]["fused_port"] = pick(cpu.get("fused_port", {}), "value", "cores")
    par = d.get("parity")
    if par:
        line["parity"] = pick(par, "checked_points", "max_abs_val_err_vs_oracle", "grad_mismatches_vs_oracle", "parity_unpinned")
    if "legs" in d:
        line["legs"] = {k: compact_leg(k, v) for k, v in d["legs"].items()}
    for key in ("all_in_range_batch", "mid_batch", "large_batch", "p1e8_batch"):
        if key in d:
            b = d[key]
            line[key] = {"ms": b.get("ms_per_launch", b.get("kernel_ms_median")), "frac_of_8TBs": b["frac_of_8TBs"],
                         **pick(b, "x_torch_copy")}
    if "torch_copy" in d:
        line["torch_copy_GBs"] = d["torch_copy"]["GBs"]
    if "latency" in d and "cached(points)" in d["latency"]:
        line["latency_us"] = {"cached_p50": d["latency"]["cached(points)"]["p50_us"], "cached_p99": d["latency"]["cached(points)"]["p99_us"]}
    # one row per run, the same keys at every N: the driver's 1 / 2 / 4 / 8 runs concatenate into the scaling table
    row = {"n": d["n_gpus"], "value": d["value"], "frac_hbm": roof.get("frac")}
    c4 = d.get("legs", {}).get("c4") if isinstance(d.get("legs"), dict) else None
    if isinstance(c4, dict) and isinstance(c4.get("sharded"), dict):
        row["c4_kernel_only_ms"] = c4["sharded"].get("ms_per_step")
        g = c4.get("gathered")
        row["c4_gathered_ms"] = g.get("ms_per_step") if isinstance(g, dict) else None
    line["scaling_table"] = [row]
    if "legs_aborted" in d:
        line["legs_aborted"] = d["legs_aborted"][:100]
    line["detail"] = detail_name
    return line


def compact_text(d, detail_name):
    """json text of the contract line, guaranteed under COMPACT_LIMIT: optional blocks are dropped, least important first, if
    a run (many failing legs with long messages) should ever push it over."""
    line = sig(compact_line(d, detail_name))
    text = json.dumps(line, separators=(",", ":"))
    for drop in ("latency_us", "torch_copy_GBs", "all_in_range_batch", "mid_batch", "p1e8_batch", "large_batch", "legs", "parity"):
        if len(text) < COMPACT_LIMIT:
            break
        line.pop(drop, None)
        line["dropped_for_size"] = line.get("dropped_for_size", []) + [drop]
        text = json.dumps(line, separators=(",", ":"))
    return text


def main():
    args = parse_args()
    spawn_ranks_if_needed(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.launch_check:
        launch_check(args, rank, world)
        return

    # the CPU baseline's threads (OpenMP in the C oracle, and torch's own pool) stay where they start: set before either
    # runtime is loaded (round 3's unpinned 4-second sample swung 3.6x between runs)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    import numpy as np
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X visible to PyTorch-ROCm (no CPU path exists)")
    if args.share_gpu:
        local_rank, backend = 0, "gloo"
    else:
        backend = args.backend
        if world > torch.cuda.device_count():
            raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} GPU(s) visible "
                             "(one process per GPU; --share-gpu is the 1-GPU functional test)")
    torch.cuda.set_device(local_rank)
    use_pg = world > 1 or args.force_pg
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        import datetime
        # longer than --legs-deadline: the deadline (which keeps the headline) must fire before the watchdog tears the job down
        limit = datetime.timedelta(seconds=args.legs_deadline + 120)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=limit)
        else:
            dist.init_process_group(backend, timeout=limit)
    import pytorch_volumetric_amd as pv
    import workloads as Wk
    timer = Timer(torch, dist, world if not args.force_pg else max(world, 2))  # force-pg: barriers / all-reduce run too

    cached = Wk.build_c2_cache()
    pts = Wk.c2_points(cached, args.points, seed=1234 + rank)
    P = pts.shape[0]
    val = torch.empty((P,), dtype=torch.float32, device="cuda")
    grad = torch.empty((P, 3), dtype=torch.float32, device="cuda")

    def step():
        cached.query_into(pts, val, grad)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    graph = None
    if not args.no_graph:
        # the launch-bound inner loop (a ~6 us kernel) captured once: K launches, one replay
        graph = capture_graph(torch, step, args.steps)
        # untimed: the first replay uploads the graph; a back-to-back burst lets the clocks settle (MI355X DVFS needs a few
        # thousand of these ~6 us launches, MI355X_MICROARCH.md) when the caller asks for a short K / W.  A burst of
        # un-synchronised replays leaves the HIP runtime with housekeeping that the NEXT launch call pays for (measured,
        # tools/k20_probe.py: that call returns after ~200 us instead of ~15 us), so the burst is followed by three
        # synchronised replays that absorb it.  The timed region below is still exactly K steps.
        for _ in range(max(1, -(-3000 // max(args.steps, 1)))):
            graph.replay()
        torch.cuda.synchronize()
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()

    def k_steps():
        if graph is not None:
            graph.replay()
        else:
            for _ in range(args.steps):
                step()

    # The contract's timed region -- barrier + synchronize | exactly K steps | synchronize + barrier, MAX over ranks -- run
    # once: --steps is the number of timed steps.  (A 20-step region is 0.13 ms of GPU work, so one host hiccup shows in a
    # short K; a longer K averages it out.)
    elapsed = timer(k_steps)
    dumped = None
    if args.dump_outputs and rank == 0:
        # untimed: val / grad still hold the last timed step's outputs (everything after this reuses them)
        dumped = dump_outputs(torch, np, args.dump_outputs, {"sdf_val": val, "sdf_grad": grad})

    # ---- the dominant kernel's per-launch duration, independent of K: events around a separate >=2000-launch graph ----
    kg_n = max(KERNEL_GRAPH_LAUNCHES, args.steps)
    kgraph = capture_graph(torch, step, kg_n)
    kgraph.replay()
    torch.cuda.synchronize()
    k_ms, k_ms_best = graph_ms_per_launch(torch, kgraph, kg_n, reps=5, stats=True)
    del kgraph
    # yardstick, timed the same way: a plain device-to-device copy that moves the same bytes (14 MB read + 14 MB written for
    # the 1M-point launch; torch's own copy kernel) -- what the chip does with 28 MB per launch, launch ramp included
    half = BYTES_PER_QUERY * P // 2 // 4
    c_src, c_dst = torch.empty(half, dtype=torch.float32, device="cuda"), torch.empty(half, dtype=torch.float32, device="cuda")
    cgraph = capture_graph(torch, lambda: c_dst.copy_(c_src), kg_n)
    cgraph.replay()
    torch.cuda.synchronize()
    copy_ms = graph_ms_per_launch(torch, cgraph, kg_n, reps=3)
    del cgraph, c_src, c_dst
    e_mean, e_med, e_min = time_eager_kernel(torch, np, step, 200)
    # the drop-in call itself -- what a user of the reference writes: val, grad = sdf(points) (sdf.py:535-591), outputs allocated
    d_call, d_sync = time_calls(torch, np, lambda: cached(pts), reps=400)

    out = None
    if rank == 0:
        qps = world * P * args.steps / elapsed
        algo = BYTES_PER_QUERY * P
        ev_gbs = algo / (k_ms * 1e-3) / 1e9
        traffic, traffic_source = read_traffic(P)
        rocprof_us, rocprof_calls, rocprof_source, rocprof_ctx = read_rocprof_kernel_us(P)
        # `frac` is THIS run's: HIP events on the launch stream around a >= 2000-launch hipGraph of the same call (VERDICT r5 weak
        # 3: round 5 printed the committed rocprofv3 average whenever the live figure was within 20 % of it, so a regression of
        # that size left `frac` unchanged).  The committed kernel trace stays beside it as `frac_rocprof`, the wall figure of the
        # contract's own timed region as `frac_wall`.
        launch_us = k_ms * 1e3
        achieved = ev_gbs
        out = {
            "metric": "SDF (val+grad) queries/sec", "value": qps, "unit": "queries/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"C2: CachedSDF 0.01 m voxels (37x33x40) on YcbPowerDrill, {P} uniform points per GPU per step",
                       "points_per_gpu": P, "index_dtype": "f64" if cached._view.index_f64 else "f32",
                       "out_of_range": "BOUNDING_BOX fallback, fused",
                       "launch": ("one hipGraph of the K steps; one timed region" if graph is not None
                                  else "eager; one timed region"),
                       "timed_region": "barrier + sync | exactly K steps | event spin + sync | barrier; max over ranks",
                       "gather": False, "parallelism": f"points x{world}", "ranks": world,
                       "backend": (dist.get_backend() if use_pg else None), "gpus_requested": args.gpus},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": cached_query_kernel_name(P), "algorithmic_bytes_per_launch": algo,
                         "launch_us": launch_us, "launch_source": "hip events (this run)",
                         "frac_is": f"28 B x P / mean launch duration, HIP events around a hipGraph of {kg_n} launches, this run",
                         "rocprof_launch_us": rocprof_us, "rocprof_calls": rocprof_calls, "rocprof_source": rocprof_source,
                         "frac_rocprof": None if rocprof_us is None else algo / (rocprof_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                         # the same trace by what preceded each launch (tools/profile_bench.sh): "queued" = nodes of a graph replay, whose
                         # traced duration is the launch-to-launch period that `launch_us` measures; "paced" / "isolated" = eager calls
                         "rocprof_by_context": None if not rocprof_ctx else {
                             k: {"calls": v["calls"], "avg_us": v["avg_us"], "median_us": v["median_us"],
                                 "frac": algo / (v["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS}
                             for k, v in rocprof_ctx.items() if v},
                         "frac_wall": algo / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                         "frac_events": ev_gbs / HBM_PEAK_GBS, "launch_us_events": k_ms * 1e3,
                         "launch_us_events_best_replay": k_ms_best * 1e3,
                         "frac_events_best_replay": algo / (k_ms_best * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "events": f"HIP events around a separate hipGraph of {kg_n} launches of the same call, / {kg_n}, mean of 5 replays",
                         "eager_launch_ms": {"mean": e_mean, "median": e_med, "min": e_min},
                         "dropin_call": {"call": "val, grad = cached(points)  # CachedSDF.__call__, outputs allocated per call",
                                         "ms_per_call": d_call, "queries_per_s": P / (d_call * 1e-3),
                                         "ms_per_call_synchronized_each": d_sync,
                                         "timing": "400 calls back to back + one synchronize; median of 200 synchronized calls"},
                         "copy_same_bytes_us": copy_ms * 1e3, "copy_same_bytes_GBs": algo / (copy_ms * 1e-3) / 1e9,
                         "copy_is": "torch d2d copy moving the same bytes, same hipGraph timing; Infinity-Cache resident, not an HBM figure",
                         "timed_steps": args.steps, "timed_region_ms": elapsed * 1e3},
            "valu_model": valu_model(),
        }
        if dumped is not None:
            out["dump_outputs"] = dumped

    legs = {}
    emitted = threading.Lock()

    def emit(final):
        """rank 0: the long record -> --detail file and stderr; the compact contract line, LAST on stdout (RCCL prints a version
        banner through C stdio, which would otherwise be flushed after Python's own buffer at exit)."""
        if not emitted.acquire(blocking=False):
            return
        if rank == 0:
            import ctypes
            long_text = json.dumps(final)
            try:
                with open(args.detail, "w") as f:
                    f.write(long_text + "\n")
            except OSError as exc:
                print(f"bench.py: could not write {args.detail}: {exc!r}", file=sys.stderr)
            print("bench_detail " + long_text, file=sys.stderr, flush=True)
            sys.stdout.flush()
            try:
                ctypes.CDLL(None).fflush(None)
            except Exception:
                pass
            print(compact_text(final, os.path.basename(args.detail)), flush=True)

    def on_deadline():
        # a rank is lost inside a leg's collective (the gate only covers failures BEFORE it): keep the headline
        if rank == 0:
            out["legs"] = dict(legs)
            out["legs_aborted"] = f"deadline of {args.legs_deadline:.0f} s passed inside the legs; listed: those finished on rank 0"
        emit(out)
        sys.stdout.flush()
        os._exit(0)

    guard = None
    if use_pg and not args.no_legs:
        guard = threading.Timer(args.legs_deadline, on_deadline)
        guard.daemon = True
        guard.start()
        if world > 1:
            # torchrun answers a worker that died (a crash inside a leg on another GPU) with SIGTERM to the others: rank 0 uses
            # it to print what it has.  The main thread may be blocked inside a collective, where a Python signal handler
            # would never run -- so SIGTERM is blocked in every thread and a helper thread waits for it.
            import signal
            signal.pthread_sigmask(signal.SIG_BLOCK, {signal.SIGTERM})

            def on_sigterm():
                signal.sigwait({signal.SIGTERM})
                on_deadline()

            threading.Thread(target=on_sigterm, daemon=True).start()
    if not args.no_legs:
        leg_steps = 20
        sm = args.small_legs
        robots = {}
        spec = [("c3", lambda g: leg_c3(torch, Wk, pv, timer, g, cached, rank, world, leg_steps, sm)),
                ("c4", lambda g: leg_c4(torch, dist, Wk, pv, timer, g, robots, rank, world, leg_steps, 0.1, True, sm, use_pg)),
                ("c4_readme_grid", lambda g: leg_c4(torch, dist, Wk, pv, timer, g, robots, rank, world, leg_steps, 1.0, False, sm)),
                ("c5", lambda g: leg_c5(torch, dist, Wk, pv, timer, g, rank, world, 5, sm, use_pg))]
        spec += [("cache_build", lambda g: leg_cache_build(torch, np, Wk, pv, g, world, sm))]
        if not sm:
            spec += [("c1", lambda g: leg_c1(torch, np, Wk, pv, g, world)),
                     ("readme_a20", lambda g: leg_readme(torch, np, Wk, pv, timer, g, robots, rank, world, 20)),
                     ("readme_a200", lambda g: leg_readme(torch, np, Wk, pv, timer, g, robots, rank, world, 200))]
        for name, fn in spec:
            gate = Gate(torch, dist, use_pg)
            try:
                if rank == args.fail_rank and name == args.fail_leg:
                    raise RuntimeError(f"--fail-rank {rank} --fail-leg {name}: forced failure before the leg's gate")
                if rank == args.hang_rank and name == args.fail_leg:
                    gate()
                    time.sleep(1e6)  # "lost inside the leg": the other ranks wait in its first collective
                legs[name] = fn(gate)
            except LegSkipped:
                legs[name] = {"skipped": "another rank failed while preparing this leg; every rank skipped it"}
            except Exception as exc:  # a failing leg must not take the headline line with it
                legs[name] = {"error": repr(exc)}
                if not gate.passed:
                    gate.agree(False)  # the other ranks are waiting at their gate: let them skip the leg
            torch.cuda.empty_cache()
    if use_pg and not args.no_legs:
        # rank 0 prints the line: let it say which legs some OTHER rank lost
        mine = torch.tensor([1 if ("error" in legs.get(n, {}) or "skipped" in legs.get(n, {})) else 0 for n, _ in spec],
                            dtype=torch.int32, device="cuda")
        dist.all_reduce(mine, op=dist.ReduceOp.SUM)
        for (n, _), k in zip(spec, mine.tolist()):
            if k and isinstance(legs.get(n), dict):
                legs[n]["ranks_without_a_result"] = int(k)
    if rank == 0:
        out["legs"] = legs

    if not args.no_large and rank == 0 and world == 1:
        # secondary: the same batch size with EVERY point inside the cached range (every query gathers a 16-B record)
        # (2048 points = one workgroup fewer than the headline batch: the same kernel of the size dispatch, and a kernel trace of
        # this command tells the two workloads apart by their grid sizes -- until round 6 the ~7 us launches of this leg were a
        # third of the "1M-point launches" that profiles/*_kernel_stats averaged, and pulled that average up by 0.45 us)
        Pin = P - 2048 if P > 4096 else P
        pin = Wk.c2_points(cached, Pin, seed=7, margin=-1e-4)
        vin, gin = val[:Pin], grad[:Pin]
        for _ in range(50):
            cached.query_into(pin, vin, gin)
        g2 = capture_graph(torch, lambda: cached.query_into(pin, vin, gin), 1000)
        g2.replay()
        torch.cuda.synchronize()
        t_in = graph_ms_per_launch(torch, g2, 1000)
        out["all_in_range_batch"] = {"points": Pin, "ms_per_launch": t_in, "queries_per_s": Pin / (t_in * 1e-3),
                                     "achieved_GBs": BYTES_PER_QUERY * Pin / (t_in * 1e-3) / 1e9,
                                     "frac_of_8TBs": BYTES_PER_QUERY * Pin / (t_in * 1e-3) / 1e9 / HBM_PEAK_GBS}
        del g2, pin, vin, gin
        # secondary: 8M points (235 MB of traffic: larger than every L2, just inside the 256 MB Infinity Cache) -- the size
        # at which launch ramp no longer matters and the kernel streams at its best
        PM = 1 << 23
        mid = Wk.c2_points(cached, PM, seed=98)
        mval = torch.empty((PM,), dtype=torch.float32, device="cuda")
        mgrad = torch.empty((PM, 3), dtype=torch.float32, device="cuda")
        for _ in range(100):
            cached.query_into(mid, mval, mgrad)
        gm = capture_graph(torch, lambda: cached.query_into(mid, mval, mgrad), 200)
        gm.replay()
        torch.cuda.synchronize()
        t_mid = graph_ms_per_launch(torch, gm, 200)
        out["mid_batch"] = {"points": PM, "ms_per_launch": t_mid, "queries_per_s": PM / (t_mid * 1e-3),
                            "achieved_GBs": BYTES_PER_QUERY * PM / (t_mid * 1e-3) / 1e9,
                            "frac_of_8TBs": BYTES_PER_QUERY * PM / (t_mid * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            "note": "working set inside the 256 MB Infinity Cache"}
        del gm, mid, mval, mgrad
        # secondary: a batch far beyond the 256 MB Infinity Cache, where the kernel is HBM- rather than launch-bound
        PL = 1 << 26
        big = Wk.c2_points(cached, PL, seed=99)
        bval = torch.empty((PL,), dtype=torch.float32, device="cuda")
        bgrad = torch.empty((PL, 3), dtype=torch.float32, device="cuda")
        for _ in range(60):  # the chip needs ~20 launches of this size to settle its clocks (DVFS ramp)
            cached.query_into(big, bval, bgrad)
        _, m, mn = time_eager_kernel(torch, np, lambda: cached.query_into(big, bval, bgrad), 40)
        out["large_batch"] = {"points": PL, "kernel_ms_median": m, "kernel_ms_min": mn,
                              "queries_per_s": PL / (m * 1e-3),
                              "achieved_GBs": BYTES_PER_QUERY * PL / (m * 1e-3) / 1e9,
                              "frac_of_8TBs": BYTES_PER_QUERY * PL / (m * 1e-3) / 1e9 / HBM_PEAK_GBS}
        del big, bval, bgrad
        # yardstick for the streaming regime ("against both datasheet peak and measured-copy peak"): torch's
        # device-to-device copy moving the same 1.88 GB (940 MB read + 940 MB written), timed the same way
        cbytes = BYTES_PER_QUERY * PL // 2
        csrc = torch.empty(cbytes // 4, dtype=torch.float32, device="cuda")
        cdst = torch.empty(cbytes // 4, dtype=torch.float32, device="cuda")
        for _ in range(20):
            cdst.copy_(csrc)
        _, cm, _ = time_eager_kernel(torch, np, lambda: cdst.copy_(csrc), 20)
        copy_gbs = 2 * cbytes / (cm * 1e-3) / 1e9
        out["torch_copy"] = {"bytes_moved": 2 * cbytes, "ms_median": cm, "GBs": copy_gbs, "frac_of_8TBs": copy_gbs / HBM_PEAK_GBS,
                                "what": "torch d2d copy of 940 MB, events per launch, median of 20; a yardstick, not a ceiling (tools/membw: 6.5 TB/s)"}
        out["large_batch"]["x_torch_copy"] = out["large_batch"]["achieved_GBs"] / copy_gbs
        del csrc, cdst
        torch.cuda.empty_cache()
        # secondary: the P = 1e8 launch SURVEY.md 8(d) asks for (2.8 GB of algorithmic traffic)
        PH = 100_000_000
        huge = Wk.c2_points(cached, PH, seed=100)
        hval = torch.empty((PH,), dtype=torch.float32, device="cuda")
        hgrad = torch.empty((PH, 3), dtype=torch.float32, device="cuda")
        for _ in range(30):
            cached.query_into(huge, hval, hgrad)
        _, m, mn = time_eager_kernel(torch, np, lambda: cached.query_into(huge, hval, hgrad), 30)
        out["p1e8_batch"] = {"points": PH, "kernel_ms_median": m, "kernel_ms_min": mn, "queries_per_s": PH / (m * 1e-3),
                             "achieved_GBs": BYTES_PER_QUERY * PH / (m * 1e-3) / 1e9,
                             "frac_of_8TBs": BYTES_PER_QUERY * PH / (m * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "x_torch_copy": BYTES_PER_QUERY * PH / (m * 1e-3) / 1e9 / copy_gbs}
        del huge, hval, hgrad
        torch.cuda.empty_cache()

    if rank == 0 and world == 1 and not args.no_legs and not args.small_legs:
        # the tail of the drop-in calls (profiles/r04_stall.txt: the 20-40 ms step rounds 2-3 chased is CPython's generation-2
        # collector walking torch's ~170k objects; pv.warm_up() freezes them out of it and loads every code object up front)
        try:
            import gc
            _, spts = pv.get_coordinates_and_points_in_grid(0.01, np.array([[-1, 0.5], [0.02, 0.02], [-0.2, 0.8]]))
            spts = spts.cuda()
            robot20 = build_robot(Wk, robots, 1.0)
            robot20.set_joint_configuration(Wk.c4_joint_configs(20))
            n_calls = args.latency_calls
            cold = {"cached(points)": call_latency(torch, np, lambda: cached(spts), calls=max(1000, n_calls // 4))}
            t0 = time.perf_counter()
            pv.warm_up()
            warm_ms = (time.perf_counter() - t0) * 1e3
            out["latency"] = {"points": int(spts.shape[0]), "warm_up_ms": warm_ms,
                              "timing": "perf_counter around every call, queue drained every 256 calls; after pv.warm_up()",
                              "cached(points)": call_latency(torch, np, lambda: cached(spts), calls=n_calls),
                              "robot(points) A=20, README-size link grids": call_latency(torch, np, lambda: robot20(spts), calls=n_calls),
                              "before_warm_up": cold, "gc_frozen_objects": gc.get_freeze_count()}
        except Exception as exc:
            out["latency"] = {"error": repr(exc)}

    if rank == 0:
        # ---- everything below uses the oracle: only after all GPU timing ----
        from oracle import oracle
        from tests import helpers as H
        n_chk = min(P, 50_000)
        step()
        torch.cuda.synchronize()
        oval, ograd, ooob = oracle.cached_query(H.oracle_grid_from_cached(cached), pts[:n_chk].cpu().numpy())
        max_err = float(np.nanmax(np.abs(val[:n_chk].cpu().numpy() - oval)))
        grad_mismatch = int((~np.isclose(grad[:n_chk].cpu().numpy(), ograd, rtol=0, atol=0, equal_nan=True)).sum())
        out["config"]["oob_fraction"] = float(ooob.mean())
        out["parity"] = {"checked_points": n_chk, "max_abs_val_err_vs_oracle": max_err,
                         "grad_mismatches_vs_oracle": grad_mismatch,
                         "oracle": "oracle/pvamd_oracle.c (in-repo CPU restatement)", "oracle_pinned": oracle_pins(np),
                         "parity_unpinned": not all(oracle_pins(np).values())}
        if not args.no_cpu_baseline and world == 1:  # the CPU baseline is timed on rank 0 of the 1-GPU run only
            out["cpu_baseline"] = cpu_baseline(torch, np, cached, pts, args.cpu_seconds)
    if use_pg:
        dist.barrier()
    if guard is not None:
        guard.cancel()
    if use_pg:
        dist.destroy_process_group()
    emit(out)


if __name__ == "__main__":
    main()
