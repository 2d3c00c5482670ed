"""pvamd_redistance (csrc/redistance.hip) on 64^3, 128^3 and 256^3 lattices over [-2, 2)^3 metres, two scenes each with max_distance
infinite and 0.5 m:

  room   the TSDF tools/bench_tsdf.py fuses (eight 640 x 480 frames of a box room), its records redistanced with band = truncation
  ball   a ball of radius 0.2 m in the middle, analytic values clipped to +/-4 voxels: nearly all of the lattice is far from any
         crossing, the long-scan case

against, measured in the same run:

  edt    pvamd_distance_transform (signed) on the occupancy V < 0 of the same lattice: the route a caller had before
  cdist  at 64^3 only: the crossing points worked out with torch ops, then a chunked torch.cdist minimum over them

Timed with HIP events around the C entry points on buffers allocated beforehand: median over --calls calls after a warm-up.
Prints one JSON line per case and the markdown table of profiles/redistance.md (--out FILE writes it there too).

  python tools/bench_redistance.py [--sizes 64 128 256] [--calls 21] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402
import bench_tsdf  # noqa: E402

BALL_RADIUS = 0.2
LIMIT = 0.5  # metres


def median_ms(fn, calls, warm=2):
    times = []
    for i in range(calls + warm):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= warm:
            times.append(start.elapsed_time(stop))
    return statistics.median(times)


def room_records(size):
    """((n, 4) records of the fused room, resolution, band)."""
    vol = bench_tsdf.new_volume(size)
    depth, poses = bench_tsdf.room_frames(8)
    vol.integrate(depth, bench_tsdf.INTRINSICS, poses)
    return pv.TSDFField(vol)._records, vol.resolution, vol.truncation


def ball_records(size):
    res = 4.0 / size
    axis = -2.0 + torch.arange(size, dtype=torch.float64, device="cuda") * res - 0.3 * res  # the centre is off the lattice
    c = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1)
    norm = c.norm(dim=-1)
    band = 4 * res
    records = torch.cat(((norm - BALL_RADIUS).clamp(-band, band)[..., None], c / norm[..., None]), dim=-1)
    return records.float().reshape(-1, 4).contiguous(), res, band


def crossing_points(values):
    """(M, 3) float32 crossing positions in voxels of a (nx, ny, nz) field, by the contract's statements in torch ops."""
    points = []
    idx = torch.stack(torch.meshgrid(*(torch.arange(s, device=values.device, dtype=torch.float32) for s in values.shape),
                                     indexing="ij"), dim=-1)
    for k in range(3):
        a, b = values.narrow(k, 0, values.shape[k] - 1), values.narrow(k, 1, values.shape[k] - 1)
        cross = torch.isfinite(a) & torch.isfinite(b) & ((a < 0) != (b < 0))
        p = idx.narrow(k, 0, values.shape[k] - 1)[cross].clone()
        p[:, k] += (a / (a - b))[cross]
        points.append(p)
    return torch.cat(points)


def cdist_minimum(values, chunk=8192):
    """(n,) float32 distance in voxels from every voxel to the nearest crossing point: chunked torch.cdist."""
    sites = crossing_points(values)
    idx = torch.stack(torch.meshgrid(*(torch.arange(s, device=values.device, dtype=torch.float32) for s in values.shape),
                                     indexing="ij"), dim=-1).reshape(-1, 3)
    return torch.cat([torch.cdist(idx[i:i + chunk], sites).amin(dim=1) for i in range(0, idx.shape[0], chunk)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    rows = []
    for size in args.sizes:
        n = size ** 3
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        sites = torch.empty((n,), dtype=torch.int32, device="cuda")
        squared = torch.empty((n,), dtype=torch.float32, device="cuda")
        scratch = _lib.scratch_buffer(_lib.redistance_scratch_bytes(size, size, size), out.device)
        edt_squared = torch.empty((n,), dtype=torch.int32, device="cuda")
        edt_scratch = _lib.scratch_buffer(_lib.distance_transform_scratch_bytes(size, size, size, True), out.device)
        for scene, make in (("room", room_records), ("ball", ball_records)):
            records, res, band = make(size)
            occ = (records[:, 0] < 0).view(torch.uint8).contiguous()

            def edt():
                _lib.check(lib.pvamd_distance_transform(_lib.ptr(occ), size, size, size, res, 1, _lib.ptr(out), _lib.ptr(sites),
                                                        _lib.ptr(edt_squared), _lib.ptr(edt_scratch), _lib.stream_ptr()),
                           "pvamd_distance_transform")
            edt_ms = median_ms(edt, args.calls)
            cdist_ms = agreement = None
            if size == 64:
                values = records[:, 0].reshape(size, size, size)
                cdist_ms = median_ms(lambda: cdist_minimum(values), max(3, args.calls // 4), warm=1)
            for limit in (math.inf, LIMIT):
                def call():
                    _lib.check(lib.pvamd_redistance(_lib.ptr(records), size, size, size, res, band, limit, _lib.ptr(out),
                                                    _lib.ptr(sites), _lib.ptr(squared), _lib.ptr(scratch), _lib.stream_ptr()),
                               "pvamd_redistance")
                ms = median_ms(call, args.calls)
                torch.cuda.synchronize()
                kept, far = int((sites == _lib.REDIST_KEPT).sum()), int((sites == -1).sum())
                if size == 64 and limit == math.inf:
                    found = sites >= 0
                    agreement = float((squared[found].sqrt() - cdist_minimum(values)[found]).abs().max())
                row = {"lattice": f"{size}^3", "scene": scene, "max_distance_m": limit, "redistance_ms": ms, "kept": kept,
                       "out_of_range": far, "voxels": n, "mean_distance_voxels": float(squared[sites >= 0].sqrt().mean()),
                       "distance_transform_ms": edt_ms, "ratio_to_distance_transform": ms / edt_ms, "cdist_ms": cdist_ms,
                       "cdist_largest_difference_voxels": agreement if limit == math.inf else None}
                rows.append(row)
                print(json.dumps(row), flush=True)
    lines = ["| lattice | scene | max_distance | pvamd_redistance ms | kept / out of range / voxels | mean distance, voxels | "
             "pvamd_distance_transform ms | ratio | torch.cdist route ms | largest difference to it, voxels |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        limit = "none" if math.isinf(r["max_distance_m"]) else f"{r['max_distance_m']} m"
        cd = "not run" if r["cdist_ms"] is None else f"{r['cdist_ms']:.1f}"
        diff = "" if r["cdist_largest_difference_voxels"] is None else f"{r['cdist_largest_difference_voxels']:.1e}"
        lines.append(f"| {r['lattice']} | {r['scene']} | {limit} | {r['redistance_ms']:.3f} | {r['kept']} / {r['out_of_range']} / "
                     f"{r['voxels']} | {r['mean_distance_voxels']:.1f} | {r['distance_transform_ms']:.3f} | "
                     f"{r['ratio_to_distance_transform']:.1f} | {cd} | {diff} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
