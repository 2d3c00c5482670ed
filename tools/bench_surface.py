"""pvamd_surface_count / pvamd_surface_emit (csrc/surface.hip) on three volumes:

  room   the TSDF tools/bench_tsdf.py fuses (eight 640 x 480 frames of a box room) at 128^3 and 256^3, meshed with the weight mask
  ball   the 51^3 analytic ball of the tests (radius 0.3, 0.02 m voxels, values clipped to +/-0.06)

Per case: count, emit (with normals) and emit without normals, timed with HIP events around the C entry points on buffers allocated
beforehand; the end-to-end call (surface_of_records: allocations, count, the read of the two counts, emit) by the host's clock,
since it synchronises; the bytes the contract needs -- 16 B per voxel read (plus 1 B with a mask) and the rows written -- over the
count + emit time, against 8 TB/s; and the same mesh by torch ops a caller could write today (shifted slices, where, nonzero,
gathers; no normals), with whether it equals the fused result bit for bit.  Median over --calls calls after a warm-up.
Prints one JSON line per case and the markdown table of profiles/surface.md (--out FILE writes it there too).

  python tools/bench_surface.py [--sizes 128 256] [--calls 21] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import _lib, surface  # noqa: E402
import bench_tsdf  # noqa: E402
from bench_redistance import median_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def room(size):
    """(descriptor, (n, 4) records, (n,) uint8 mask) of the fused room."""
    vol = bench_tsdf.new_volume(size)
    depth, poses = bench_tsdf.room_frames(8)
    vol.integrate(depth, bench_tsdf.INTRINSICS, poses)
    return vol._grid.voxels._grid_desc(), pv.TSDFField(vol)._records, (vol.weight > 0).to(torch.uint8).reshape(-1).contiguous()


def ball():
    axis = torch.linspace(-0.5, 0.5, 51, dtype=torch.float64, device="cuda")
    c = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1)
    norm = c.norm(dim=-1)
    records = torch.cat(((norm - 0.3).clamp(-0.06, 0.06)[..., None], c / norm.clamp_min(1e-12)[..., None]), dim=-1)
    return surface.lattice_desc((51, 51, 51), 0.02, (-0.5, -0.5, -0.5)), records.float().reshape(-1, 4).contiguous(), None


def torch_nets(values, valid, fmin, fres):
    """(vertices (Nv, 3) float32, faces (Nf, 3) int32) by the contract's statements in whole-tensor torch ops, float32."""
    n = values.shape
    usable = torch.isfinite(values) if valid is None else torch.isfinite(values) & (valid != 0)
    negative = values < 0

    def corner(t, off):
        return t[off[0]:n[0] - 1 + off[0], off[1]:n[1] - 1 + off[1], off[2]:n[2] - 1 + off[2]]

    offsets = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    every = torch.stack([corner(usable, o) for o in offsets]).all(dim=0)
    negatives = torch.stack([corner(negative, o) for o in offsets]).sum(dim=0)
    active = every & (negatives > 0) & (negatives < 8)
    cells = active.shape
    S = torch.zeros(cells + (3,), dtype=torch.float32, device=values.device)
    m = torch.zeros(cells, dtype=torch.float32, device=values.device)
    for k in range(3):
        o0, o1 = [j for j in range(3) if j != k]
        for d0 in (0, 1):
            for d1 in (0, 1):
                low, high = [0, 0, 0], [0, 0, 0]
                low[o0] = high[o0] = d0
                low[o1] = high[o1] = d1
                high[k] = 1
                a, b = corner(values, low), corner(values, high)
                cross = active & (corner(negative, low) != corner(negative, high))
                offset = torch.zeros(cells + (3,), dtype=torch.float32, device=values.device)
                offset[..., k], offset[..., o0], offset[..., o1] = a / (a - b), float(d0), float(d1)
                S = torch.where(cross[..., None], S + offset, S)
                m = m + cross
    where = active.nonzero()
    ids = torch.full(cells, -1, dtype=torch.int32, device=values.device)
    ids[active] = torch.arange(where.shape[0], dtype=torch.int32, device=values.device)
    p = where.float() + S[active] / m[active][:, None]
    vertices = torch.tensor(fmin, dtype=torch.float32, device=values.device) + p * torch.tensor(fres, dtype=torch.float32,
                                                                                               device=values.device)
    keys, quads = [], []
    strides = (n[1] * n[2], n[2], 1)
    for k in range(3):
        p_, q_ = (k + 1) % 3, (k + 2) % 3
        lo = [0, 0, 0]
        lo[p_] = lo[q_] = 1

        def window(t, off, size):
            return t[tuple(slice(lo[j] + off[j], size[j] - 1 + off[j]) for j in range(3))]

        def shifted(dp, dq):
            off = [0, 0, 0]
            off[p_], off[q_] = -dp, -dq
            return window(ids, off, n)

        up = [0, 0, 0]
        up[k] = 1
        c0, c1, c2, c3 = shifted(1, 1), shifted(0, 1), shifted(0, 0), shifted(1, 0)
        inside = window(negative, (0, 0, 0), n)
        emit = (inside != window(negative, up, n)) & (c0 >= 0) & (c1 >= 0) & (c2 >= 0) & (c3 >= 0)
        a = emit.nonzero() + torch.tensor(lo, device=values.device)
        inside = inside[emit]
        v1, v3 = torch.where(inside, c1[emit], c3[emit]), torch.where(inside, c3[emit], c1[emit])
        keys.append((a[:, 0] * strides[0] + a[:, 1] * strides[1] + a[:, 2]) * 3 + k)
        quads.append(torch.stack((c0[emit], v1, c2[emit], c0[emit], c2[emit], v3), dim=1))
    order = torch.argsort(torch.cat(keys))
    return vertices, torch.cat(quads)[order].reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    rows = []
    for name, make in [(f"room {size}^3", lambda size=size: room(size)) for size in args.sizes] + [("ball 51^3", ball)]:
        desc, records, valid = make()
        shape = tuple(desc.shape)
        n = shape[0] * shape[1] * shape[2]
        scratch = _lib.scratch_buffer(_lib.surface_scratch_bytes(*shape), records.device)
        counts = torch.zeros((2,), dtype=torch.int64, device="cuda")

        def count():
            _lib.check(lib.pvamd_surface_count(ctypes.byref(desc), _lib.ptr(records), _lib.ptr(valid), 0.0, _lib.ptr(scratch),
                                               _lib.ptr(counts), _lib.stream_ptr()), "pvamd_surface_count")
        count_ms = median_ms(count, args.calls)
        nv, nf = counts.tolist()
        vertices = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        normals = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        faces = torch.empty((nf, 3), dtype=torch.int32, device="cuda")

        def emit(with_normals=True):
            _lib.check(lib.pvamd_surface_emit(ctypes.byref(desc), _lib.ptr(records), _lib.ptr(valid), 0.0, _lib.ptr(scratch), nv, nf,
                                              _lib.ptr(vertices), _lib.ptr(normals if with_normals else None), _lib.ptr(faces),
                                              _lib.stream_ptr()), "pvamd_surface_emit")
        emit_ms = median_ms(emit, args.calls)
        plain_ms = median_ms(lambda: emit(False), args.calls)

        def whole():
            torch.cuda.synchronize()
            start = time.perf_counter()
            surface.surface_of_records(desc, records, valid, 0.0, True)
            torch.cuda.synchronize()
            return (time.perf_counter() - start) * 1e3
        whole_ms = statistics.median([whole() for _ in range(args.calls + 2)][2:])
        values = records[:, 0].reshape(shape).contiguous()
        mask = None if valid is None else valid.reshape(shape)
        fmin, fres = [desc.fmin[k] for k in range(3)], [desc.fres[k] for k in range(3)]
        torch_ms = median_ms(lambda: torch_nets(values, mask, fmin, fres), max(3, args.calls // 4), warm=1)
        tv, tf = torch_nets(values, mask, fmin, fres)
        torch.cuda.synchronize()
        same_shape = tv.shape == vertices.shape and tf.shape == faces.shape
        bit_equal = bool(same_shape and torch.equal(tv.view(torch.int32), vertices.view(torch.int32)) and torch.equal(tf, faces))
        needed = 16 * n + (n if valid is not None else 0) + 24 * nv + 12 * nf
        row = {"case": name, "voxels": n, "vertices": nv, "triangles": nf, "count_ms": count_ms, "emit_ms": emit_ms,
               "emit_without_normals_ms": plain_ms, "end_to_end_ms": whole_ms, "needed_bytes": needed,
               "achieved_bytes_per_s": needed / ((count_ms + emit_ms) * 1e-3),
               "fraction_of_8_TB_per_s": needed / ((count_ms + emit_ms) * 1e-3) / HBM_BYTES_PER_S, "torch_ops_ms": torch_ms,
               "torch_ops_bit_equal": bit_equal, "torch_ops_over_fused": torch_ms / (count_ms + plain_ms)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    lines = ["| case | vertices / triangles | count ms | emit ms (without normals) | end to end ms | needed MB | achieved GB/s "
             "(of 8 TB/s) | torch ops ms | bit-equal | torch / (count + emit without normals) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['vertices']} / {r['triangles']} | {r['count_ms']:.3f} | {r['emit_ms']:.3f} "
                     f"({r['emit_without_normals_ms']:.3f}) | {r['end_to_end_ms']:.3f} | {r['needed_bytes'] / 1e6:.1f} | "
                     f"{r['achieved_bytes_per_s'] / 1e9:.0f} ({100 * r['fraction_of_8_TB_per_s']:.1f} %) | {r['torch_ops_ms']:.2f} | "
                     f"{'yes' if r['torch_ops_bit_equal'] else 'no'} | {r['torch_ops_over_fused']:.0f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
