"""OccupancyMap.integrate (csrc/ray_integrate.hip) on a depth image of a room: 640 x 480 rays into a 128^3 and a 256^3 map, from one
eye and with per-ray origins, against the restatement in torch a caller could write before it existed -- sample every ray each half
voxel, `free[samples] = 1`, `hit[endpoints] = 1`, a clamped log-odds step over the voxels.  NOT like for like: the sampled walk is
not exact (it skips cells a ray clips by less than half a voxel) and it moves 12 bytes per sample through memory.  The fused call is
timed with HIP events around the two C entry points, each scan on a fresh map state: median over --scans scans after a warm-up
of pvamd_ray_mark (traversal + hit launches), pvamd_occupancy_update, and both.  The split between the traversal and the hit launch
comes from a kernel trace of a --fused-only run.  Prints one JSON line per case and the markdown table of profiles/ray_integrate.md
(--out FILE writes the table there too).

  python tools/bench_ray_integrate.py [--sizes 128 256] [--scans 41] [--fused-only] [--out FILE]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402

WIDTH, HEIGHT = 640, 480
ROOM = torch.tensor([[-1.8, 1.8], [-1.8, 1.8], [-1.2, 1.2]])  # the walls, inside the map's range of [-2, 2)
EYE = torch.tensor([0.3, -0.2, 0.1])


def room_scan(per_ray_origins, seed=0):
    """(origins, endpoints) on the GPU: a pinhole camera in a box room, every pixel's ray ending on the wall it meets."""
    g = torch.Generator().manual_seed(seed)
    u = (torch.arange(WIDTH) + 0.5) / WIDTH * 2 - 1
    v = (torch.arange(HEIGHT) + 0.5) / HEIGHT * 2 - 1
    d = torch.stack((torch.ones(HEIGHT, WIDTH), u.expand(HEIGHT, WIDTH) * 0.9, -v[:, None].expand(HEIGHT, WIDTH) * 0.7), dim=-1)
    d = d / d.norm(dim=-1, keepdim=True)
    origins = EYE.expand(HEIGHT, WIDTH, 3)
    if per_ray_origins:  # a sensor that moved while it scanned: every ray has an eye of its own, a few centimetres apart
        origins = origins + (torch.rand((HEIGHT, WIDTH, 3), generator=g) - 0.5) * 0.1
    t_lo, t_hi = (ROOM[:, 0] - origins) / d, (ROOM[:, 1] - origins) / d
    t = torch.maximum(t_lo, t_hi).amin(dim=-1, keepdim=True)  # the origin is inside: the exit of the box
    endpoints = origins + t * d
    return (origins if per_ray_origins else EYE).cuda().contiguous(), endpoints.cuda().contiguous()


def map_range(size):
    res = 4.0 / size
    return res, [(-2.0, -2.0 + (size - 1) * res)] * 3


def new_map(size):
    omap = pv.OccupancyMap(*map_range(size), device="cuda")
    assert omap.shape == (size,) * 3
    return omap


def fused_ms(omap, origins, endpoints, scans):
    """Medians (ray_mark, update, both) in ms over `scans` scans, each on a reset map."""
    lib = _lib.load()
    desc = ctypes.byref(omap._grid.voxels._grid_desc())
    shared = int(origins.numel() == 3)
    origins, endpoints = origins.reshape(-1, 3), endpoints.reshape(-1, 3)
    R = endpoints.shape[0]
    n = omap.log_odds.numel()
    times = []
    for i in range(scans + 3):
        omap.reset()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(lib.pvamd_ray_mark(desc, _lib.ptr(origins), shared, _lib.ptr(endpoints), R, math.inf, _lib.ptr(omap._marks),
                                      _lib.stream_ptr()), "pvamd_ray_mark")
        ev[1].record()
        _lib.check(lib.pvamd_occupancy_update(_lib.ptr(omap._marks), n, omap.l_hit, omap.l_miss, omap.l_min, omap.l_max,
                                              _lib.ptr(omap.log_odds), _lib.ptr(omap._observed), _lib.stream_ptr()),
                   "pvamd_occupancy_update")
        ev[2].record()
        ev[2].synchronize()
        if i >= 3:  # the first three warm up
            times.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[0].elapsed_time(ev[2])))
    return tuple(statistics.median(t[k] for t in times) for k in range(3))


class TorchSampledMap:
    """What a caller would write with the containers alone: two bool VoxelGrids written through points and a torch update."""

    def __init__(self, omap, size):
        self.res, ranges = map_range(size)
        self.free = pv.VoxelGrid(self.res, ranges, dtype=torch.bool, device="cuda")
        self.hit = pv.VoxelGrid(self.res, ranges, dtype=torch.bool, device="cuda")
        self.log_odds = torch.zeros_like(omap.log_odds)
        self.constants = (omap.l_hit, omap.l_miss, omap.l_min, omap.l_max)

    def integrate(self, origins, endpoints, rays_per_chunk=1 << 16):
        """One scan; returns the classification it used, coded like pvamd_ray_mark's."""
        e = endpoints.reshape(-1, 3)
        o = origins.reshape(-1, 3).expand_as(e)
        v = e - o
        steps = int(math.ceil(v.norm(dim=-1).max().item() / (0.5 * self.res))) + 1
        t = torch.linspace(0.0, 1.0, steps, device=e.device)
        for a in range(0, e.shape[0], rays_per_chunk):
            samples = o[a:a + rays_per_chunk, None] + t[None, :, None] * v[a:a + rays_per_chunk, None]
            self.free[samples.reshape(-1, 3)] = 1
        self.hit[e] = 1
        hit, free = self.hit.get_voxel_values(), self.free.get_voxel_values()
        l_hit, l_miss, l_min, l_max = self.constants
        step = torch.where(hit, l_hit, torch.where(free, l_miss, 0.0))
        self.log_odds.copy_(torch.where(hit | free, (self.log_odds + step).clamp(l_min, l_max), self.log_odds))
        marks = hit.to(torch.uint8) * _lib.MARK_HIT + (free & ~hit).to(torch.uint8) * _lib.MARK_FREE
        hit.zero_()
        free.zero_()
        return marks


def torch_ms(sampled, origins, endpoints, scans):
    times = []
    for i in range(scans + 2):
        sampled.log_odds.zero_()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        sampled.integrate(origins, endpoints)
        stop.record()
        stop.synchronize()
        if i >= 2:
            times.append(start.elapsed_time(stop))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--scans", type=int, default=41)
    ap.add_argument("--fused-only", action="store_true", help="no baseline (for a kernel trace of the fused call)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for size in args.sizes:
        for per_ray in (False, True):
            origins, endpoints = room_scan(per_ray)
            omap = new_map(size)
            mark_ms, update_ms, both_ms = fused_ms(omap, origins, endpoints, args.scans)
            marks = pv.ray_marks(omap, origins, endpoints)
            row = {"map": f"{size}^3", "origins": "per ray" if per_ray else "one eye", "rays": WIDTH * HEIGHT,
                   "free_voxels": int((marks == _lib.MARK_FREE).sum()), "hit_voxels": int((marks == _lib.MARK_HIT).sum()),
                   "ray_mark_ms": mark_ms, "update_ms": update_ms, "integrate_ms": both_ms, "torch_ms": None,
                   "torch_same_class": None}
            if not args.fused_only:
                sampled = TorchSampledMap(omap, size)
                row["torch_same_class"] = float((sampled.integrate(origins, endpoints) == marks).float().mean())
                row["torch_ms"] = torch_ms(sampled, origins, endpoints, max(3, args.scans // 8))
            rows.append(row)
            print(json.dumps(row), flush=True)

    def cell(v, fmt):
        return "not run" if v is None else format(v, fmt)
    lines = ["| map | origins | voxels marked free / hit | pvamd_ray_mark ms | pvamd_occupancy_update ms | both ms | "
             "sampled rays in torch ms (not like for like) | voxels it classifies the same |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['map']} | {r['origins']} | {r['free_voxels']} / {r['hit_voxels']} | {r['ray_mark_ms']:.4f} | "
                     f"{r['update_ms']:.4f} | {r['integrate_ms']:.4f} | {cell(r['torch_ms'], '.2f')} | "
                     f"{cell(r['torch_same_class'], '.5f')} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
