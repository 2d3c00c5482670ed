"""TSDFVolume.integrate and pvamd_tsdf_records / to_sdf (csrc/tsdf.hip) on depth images of a room: 640 x 480 frames into a 128^3 and
a 256^3 volume, K = 1 and K = 8 frames per call, against the restatement in torch ops a caller could write before the kernel
existed -- voxel centres -> matmul -> gather -> `where` updates, one frame at a time.  That is the only comparison there is: the
capability did not exist.  The baseline is not bit-exact (its matmul and fused multiply-adds round differently) and the table says
how many voxels it updates differently.

Timed with HIP events around the C entry point (and around integrate() itself, host work included), every call on a reset volume:
median over --calls calls after a warm-up.  Per case also: the K = 1 pass as a fraction of HBM bandwidth at 16 bytes per updated
voxel and 8 per other voxel, and what K frames in one call save over K calls.  Prints one JSON line per case and the markdown
tables of profiles/tsdf.md (--out FILE writes them there too).

  python tools/bench_tsdf.py [--sizes 128 256] [--frames 1 8] [--calls 41] [--fused-only] [--out FILE]
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
from pytorch_volumetric_amd.tsdf import camera_from_volume  # noqa: E402

WIDTH, HEIGHT = 640, 480
INTRINSICS = (525.0, 525.0, 319.5, 239.5)  # a Kinect's
ROOM = torch.tensor([[-1.8, 1.8], [-1.8, 1.8], [-1.2, 1.2]], dtype=torch.float64)  # the walls, inside the volume's [-2, 2)
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def room_frames(K):
    """(depth (K, H, W) float32, poses (K, 4, 4) float64) on the GPU: a camera that walks a circle in a box room and looks
    outward and a little down; every pixel's depth is the z-depth of the wall its ray meets."""
    fx, fy, cx, cy = INTRINSICS
    cols = (torch.arange(WIDTH, dtype=torch.float64) - cx) / fx
    rows = (torch.arange(HEIGHT, dtype=torch.float64) - cy) / fy
    d_cam = torch.stack((cols.expand(HEIGHT, WIDTH), rows[:, None].expand(HEIGHT, WIDTH), torch.ones(HEIGHT, WIDTH, dtype=torch.float64)), -1)
    depth, poses = [], []
    for k in range(K):
        a = 2 * math.pi * k / max(K, 1) + 0.3
        eye = torch.tensor([0.5 * math.cos(a), 0.5 * math.sin(a), 0.1], dtype=torch.float64)
        z = torch.tensor([math.cos(a), math.sin(a), -0.2], dtype=torch.float64)
        z = z / z.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        pose = torch.eye(4, dtype=torch.float64)
        pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
        d = d_cam @ pose[:3, :3].T
        t = torch.maximum((ROOM[:, 0] - eye) / d, (ROOM[:, 1] - eye) / d).amin(dim=-1)  # the eye is inside: the exit of the box
        depth.append(t.float())  # d_cam has z = 1: the ray parameter is the z-depth
        poses.append(pose)
    return torch.stack(depth).cuda().contiguous(), torch.stack(poses).cuda()


def new_volume(size):
    res = 4.0 / size
    vol = pv.TSDFVolume(res, [(-2.0, -2.0 + (size - 1) * res)] * 3, truncation=4 * res, device="cuda")
    assert vol.shape == (size,) * 3
    return vol


def median_ms(fn, reset, calls, warm=3):
    times = []
    for i in range(calls + warm):
        reset()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= warm:
            times.append(start.elapsed_time(stop))
    return statistics.median(times)


def entry_point(vol, depth, inverse):
    """The pvamd_tsdf_integrate call integrate() makes, with everything it prepares on the host already prepared."""
    lib = _lib.load()
    desc = ctypes.byref(vol._grid.voxels._grid_desc())
    K, H, W = depth.shape

    def call():
        _lib.check(lib.pvamd_tsdf_integrate(desc, _lib.ptr(depth), K, H, W, _lib.ptr(inverse), *INTRINSICS, vol.truncation, math.inf,
                                            1.0, vol.max_weight, _lib.ptr(vol._state), _lib.stream_ptr()), "pvamd_tsdf_integrate")
    return call


class TorchTSDF:
    """What a caller would write with torch ops alone: the same statements, a frame at a time, over all voxels at once."""

    def __init__(self, vol):
        desc = vol._grid.voxels._grid_desc()
        axes = [desc.fmin[k] + torch.arange(desc.shape[k], dtype=torch.float32, device="cuda") * desc.fres[k] for k in range(3)]
        self.centres = torch.cartesian_prod(*axes)  # (n, 3)
        self.F = torch.zeros(self.centres.shape[0], device="cuda")
        self.W = torch.zeros_like(self.F)
        self.truncation, self.max_weight = vol.truncation, vol.max_weight

    def reset(self):
        self.F.zero_()
        self.W.zero_()

    def integrate(self, depth, inverse, weight=1.0):
        fx, fy, cx, cy = INTRINSICS
        _, H, W = depth.shape
        for k in range(depth.shape[0]):
            p = self.centres @ inverse[k, :, :3].T + inverse[k, :, 3]
            pz = p[:, 2]
            u = fx * (p[:, 0] / pz) + cx
            v = fy * (p[:, 1] / pz) + cy
            seen = (pz > 0) & (u >= -0.5) & (u < W - 0.5) & (v >= -0.5) & (v < H - 0.5)
            col = torch.floor(u + 0.5).clamp(0, W - 1).nan_to_num(0.0).long()
            row = torch.floor(v + 0.5).clamp(0, H - 1).nan_to_num(0.0).long()
            d = depth[k].reshape(-1)[row * W + col]
            sdf = d - pz
            seen &= (d > 0) & torch.isfinite(d) & (sdf >= -self.truncation)
            f = (sdf / self.truncation).clamp(max=1.0)
            Wn = self.W + weight
            self.F = torch.where(seen, (self.W * self.F + weight * f) / Wn, self.F)
            self.W = torch.where(seen, Wn.clamp(max=self.max_weight), self.W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=41)
    ap.add_argument("--fused-only", action="store_true", help="no baseline (for a kernel trace of the fused calls)")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows, record_rows = [], []
    for size in args.sizes:
        vol = new_volume(size)
        n = vol._state.numel() // 2
        for K in args.frames:
            depth, poses = room_frames(K)
            inverse = camera_from_volume(poses)
            kernel_ms = median_ms(entry_point(vol, depth, inverse), vol.reset, args.calls)
            call_ms = median_ms(lambda: vol.integrate(depth, INTRINSICS, poses), vol.reset, args.calls)
            single = [entry_point(vol, depth[k:k + 1].contiguous(), inverse[k:k + 1].contiguous()) for k in range(K)]
            apart_ms = median_ms(lambda: [c() for c in single], vol.reset, args.calls)
            vol.reset()
            vol.integrate(depth, INTRINSICS, poses)
            updated = int((vol.weight > 0).sum())
            row = {"volume": f"{size}^3", "frames": K, "updated_voxels": updated, "voxels": n, "entry_point_ms": kernel_ms,
                   "integrate_ms": call_ms, "one_call_per_frame_ms": apart_ms, "hbm_fraction": None, "torch_ms": None,
                   "torch_same_weight": None, "torch_max_tsdf_difference": None}
            if K == 1:
                row["hbm_fraction"] = (16 * updated + 8 * (n - updated)) / (kernel_ms * 1e-3) / HBM_BYTES_PER_S
            if not args.fused_only:
                base = TorchTSDF(vol)
                base.integrate(depth, inverse)
                same = base.W.reshape(vol.shape) == vol.weight
                row["torch_same_weight"] = float(same.float().mean())
                row["torch_max_tsdf_difference"] = float((base.F.reshape(vol.shape) - vol.tsdf)[same].abs().max())
                row["torch_ms"] = median_ms(lambda: base.integrate(depth, inverse), base.reset, max(3, args.calls // 4), warm=2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the records of the state the last case left, and the whole to_sdf (records, the bounding box's synchronisation, the
        # CachedSDF around them)
        lib = _lib.load()
        records = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        rec_ms = median_ms(lambda: _lib.check(lib.pvamd_tsdf_records(_lib.ptr(vol._state), size, size, size, vol.resolution,
                                                                     vol.truncation, 0.0, 1.0, _lib.ptr(records), _lib.stream_ptr()),
                                              "pvamd_tsdf_records"), lambda: None, args.calls)
        sdf_ms = median_ms(lambda: vol.to_sdf("scene"), lambda: None, max(3, args.calls // 4))
        rec = {"volume": f"{size}^3", "records_ms": rec_ms, "to_sdf_ms": sdf_ms, "records_hbm_fraction": 24 * n / (rec_ms * 1e-3) / HBM_BYTES_PER_S}
        record_rows.append(rec)
        print(json.dumps(rec), flush=True)

    def cell(v, fmt):
        return "not run" if v is None else format(v, fmt)
    lines = ["| volume | frames per call | voxels updated | pvamd_tsdf_integrate ms | integrate() ms, host work included | "
             "the same frames, one call each ms | fraction of 8 TB/s (K = 1) | torch ops ms | voxels with the same weight | "
             "largest tsdf difference there |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['volume']} | {r['frames']} | {r['updated_voxels']} of {r['voxels']} | {r['entry_point_ms']:.4f} | "
                     f"{r['integrate_ms']:.4f} | {r['one_call_per_frame_ms']:.4f} | {cell(r['hbm_fraction'], '.3f')} | "
                     f"{cell(r['torch_ms'], '.3f')} | {cell(r['torch_same_weight'], '.6f')} | {cell(r['torch_max_tsdf_difference'], '.2e')} |")
    lines += ["", "| volume | pvamd_tsdf_records ms | fraction of 8 TB/s at 24 B per voxel | to_sdf() ms |", "|---|---|---|---|"]
    for r in record_rows:
        lines.append(f"| {r['volume']} | {r['records_ms']:.4f} | {r['records_hbm_fraction']:.3f} | {r['to_sdf_ms']:.3f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
