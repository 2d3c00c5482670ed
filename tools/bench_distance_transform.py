"""pvamd_distance_transform (csrc/distance_transform.hip) against the two things a caller could do before it existed: a chunked
torch.cdist + argmin brute force on the same GPU (64^3 only: it is quadratic), and scipy.ndimage.distance_transform_edt on the host
(where scipy is importable; NOT like for like -- another machine part, float64, no gradient, no records -- it is there for scale).
Random occupancy at 1 % and 50 %, signed, 64^3 / 128^3 / 256^3; --structured adds three scenes with large empty regions per
size (a ball in the middle, one-voxel walls on the six faces, one corner voxel), where the outward scans run long.  The fused call is timed with HIP events around the C entry point
with its buffers allocated beforehand: median of --regions regions of --iters calls after a warm-up.  Prints one JSON line per
case and the markdown table of profiles/distance_transform.md (--out FILE writes the table there too).

  python tools/bench_distance_transform.py [--sizes 64 128 256] [--regions 21] [--iters 5] [--structured] [--fused-only] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_volumetric_amd import _lib  # noqa: E402

RESOLUTION = 0.02


def region_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def median_ms(fn, regions, iters):
    for _ in range(3):  # warm-up
        fn()
    torch.cuda.synchronize()
    return statistics.median(region_ms(fn, iters) for _ in range(regions))


def fused_call(occ):
    """(callable that enqueues one signed transform into fixed buffers, its squared-distance output)."""
    lib = _lib.load()
    nx, ny, nz = occ.shape
    n = occ.numel()
    dev = occ.device
    records = torch.empty((n, 4), dtype=torch.float32, device=dev)
    sites = torch.empty((n,), dtype=torch.int32, device=dev)
    squared = torch.empty((n,), dtype=torch.int32, device=dev)
    scratch = _lib.scratch_buffer(_lib.distance_transform_scratch_bytes(nx, ny, nz, True), dev)
    args = (_lib.ptr(occ), nx, ny, nz, RESOLUTION, 1, _lib.ptr(records), _lib.ptr(sites), _lib.ptr(squared), _lib.ptr(scratch))

    def call():
        _lib.check(lib.pvamd_distance_transform(*args, _lib.stream_ptr()), "pvamd_distance_transform")
    return call, squared


def torch_brute_force(occ, pairs_per_chunk=1 << 27):
    """Squared distance of every voxel to the nearest voxel of the other class: chunked torch.cdist + min / argmin, the sites too."""
    shape = occ.shape
    coords = torch.stack(torch.meshgrid(*[torch.arange(s, device=occ.device) for s in shape], indexing="ij"), dim=-1).reshape(-1, 3).float()
    flat = occ.reshape(-1) != 0
    squared = torch.empty((flat.numel(),), dtype=torch.int32, device=occ.device)
    sites = torch.empty((flat.numel(),), dtype=torch.int64, device=occ.device)
    for targets, others in ((~flat, flat), (flat, ~flat)):
        t_idx, s_idx = targets.nonzero().squeeze(1), others.nonzero().squeeze(1)
        if t_idx.numel() == 0 or s_idx.numel() == 0:
            continue
        s_xyz = coords[s_idx]
        chunk = max(1, pairs_per_chunk // s_idx.numel())
        for a in range(0, t_idx.numel(), chunk):
            d = torch.cdist(coords[t_idx[a:a + chunk]], s_xyz)
            best, arg = d.min(dim=1)
            squared[t_idx[a:a + chunk]] = torch.round(best * best).to(torch.int32)
            sites[t_idx[a:a + chunk]] = s_idx[arg]
    return squared, sites


def scipy_signed(occ_host):
    from scipy import ndimage
    t0 = time.perf_counter()
    outside = ndimage.distance_transform_edt(occ_host == 0)
    inside = ndimage.distance_transform_edt(occ_host != 0)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, np.rint(np.where(occ_host != 0, inside, outside) ** 2).astype(np.int64).reshape(-1)


def cases(size, structured):
    """(label, uint8 occupancy) of every case at one size."""
    rng = np.random.default_rng(size)
    for fraction in (0.01, 0.5):
        yield f"random {100 * fraction:.0f} %", (rng.random((size, size, size)) < fraction).astype(np.uint8)
    if structured:
        c = np.arange(size) - size / 2
        yield "ball of radius size / 12 in the middle", \
            (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2 <= (size / 12) ** 2).astype(np.uint8)
        walls = np.zeros((size,) * 3, np.uint8)
        walls[0] = walls[-1] = walls[:, 0] = walls[:, -1] = walls[:, :, 0] = walls[:, :, -1] = 1
        yield "one-voxel walls on the six faces", walls
        corner = np.zeros((size,) * 3, np.uint8)
        corner[0, 0, 0] = 1
        yield "one corner voxel", corner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--structured", action="store_true", help="also time three scenes with large empty regions per size")
    ap.add_argument("--fused-only", action="store_true", help="no baselines (for a kernel trace of the fused call)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    try:
        import scipy  # noqa: F401
        have_scipy = not args.fused_only
    except ImportError:
        have_scipy = False
    rows = []
    for size in args.sizes:
        for label, host in cases(size, args.structured):
            occ = torch.from_numpy(host).cuda()
            call, squared = fused_call(occ)
            row = {"grid": f"{size}^3", "case": label, "occupied": float(host.mean()), "voxels": size ** 3,
                   "fused_ms": median_ms(call, args.regions, args.iters), "torch_ms": None, "torch_agrees": None,
                   "scipy_host_ms": None, "scipy_agrees": None}
            if size == 64 and not args.fused_only:
                want, _ = torch_brute_force(occ)
                row["torch_agrees"] = bool(torch.equal(want, squared))
                row["torch_ms"] = median_ms(lambda: torch_brute_force(occ), 3, 1)
            if have_scipy:
                row["scipy_host_ms"], want = scipy_signed(host)
                row["scipy_agrees"] = bool(np.array_equal(want, squared.cpu().numpy()))
            rows.append(row)
            print(json.dumps(row), flush=True)

    def cell(v, fmt):
        return "not run" if v is None else format(v, fmt)
    lines = ["| grid | occupancy | fused transform ms | torch.cdist + argmin on the GPU ms | scipy on the host ms (not like for like) | "
             "same squared distances (torch / scipy) |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grid']} | {r['case']} | {r['fused_ms']:.4f} | {cell(r['torch_ms'], '.1f')} | "
                     f"{cell(r['scipy_host_ms'], '.0f')} | {cell(r['torch_agrees'], '')} / {cell(r['scipy_agrees'], '')} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
