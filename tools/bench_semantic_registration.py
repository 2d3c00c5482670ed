"""pvamd_semantic_normal_eq (csrc/registration.hip sem_partial_kernel) on the drill cache at 0.01 m, nearest and trilinear, for
B x N in {64 x 16,384, 1 x 2^20} -- the shapes of profiles/registration.md -- in three configurations:

  degenerate   no kinds, no targets, delta = inf (the sums of pvamd_chamfer_normal_eq bit for bit)
  mixed        kinds uniform in 0..3, targets uniform in +-0.02, delta = inf
  outliers     the same kinds and targets, delta at the 80th percentile of |r| over the first pose's active pairs

each next to two baselines: pvamd_chamfer_normal_eq (of this build, and of the library given with --parent-lib, a build of the
commit before the semantic kernels, called by address through its own handle), and the same sums written in torch ops on (B, N)
tensors (the package's generic path, run on the cache's own query).  HIP-event timings of graph replays after a warm-up, median
of --regions regions; one replay is the two launches of an evaluation into buffers allocated once.  The torch baseline is
timed eagerly between the same events (its index tensors are built from host lists, which a capture refuses): some thirty
launches over (B, N) float64 tensors, whose device time is what the figure mostly holds at these sizes.
Prints one JSON line per row and writes the markdown table to --out.

  python tools/bench_semantic_registration.py [--regions 21] [--iters 5] [--parent-lib libpvamd.so] [--out table.md]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workloads as W  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402
from pytorch_volumetric_amd import registration as reg  # noqa: E402
from bench_registration import graphed, median_ms  # noqa: E402

CASES = ((64, 16384), (1, 1 << 20))


def parent_evaluator(path, c, mode, W32, pts):
    """pvamd_chamfer_normal_eq of another build of the library, through a handle of its own."""
    lib = ctypes.CDLL(path)
    fn = lib.pvamd_chamfer_normal_eq
    fn.restype, fn.argtypes = _lib.SIGNATURES["pvamd_chamfer_normal_eq"]
    size = lib.pvamd_chamfer_normal_eq_scratch_bytes
    size.restype, size.argtypes = _lib.SIGNATURES["pvamd_chamfer_normal_eq_scratch_bytes"]
    B, N = W32.shape[0], pts.shape[0]
    sums = torch.empty((B, _lib.REG_SUMS), dtype=torch.float64, device=pts.device)
    counts = torch.empty((B,), dtype=torch.int64, device=pts.device)
    scratch = _lib.scratch_buffer(size(B, N), pts.device)
    desc = c._grid_desc()

    def run():
        _lib.check(fn(ctypes.byref(desc), mode, _lib.ptr(W32), B, _lib.ptr(pts), N, _lib.ptr(sums), _lib.ptr(counts),
                      _lib.ptr(scratch), _lib.stream_ptr()), "pvamd_chamfer_normal_eq (parent)")
    run.sums = sums
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libpvamd.so built from the commit before the semantic kernels")
    ap.add_argument("--out", default=None, help="also write the markdown table here (profiles/semantic_registration.md quotes it)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    caches = {"nearest": W.build_c2_cache(), "trilinear": W.build_c2_cache()}
    caches["trilinear"].interpolation = "trilinear"
    rows = []
    for B, N in CASES:
        pts = W.c2_points(caches["nearest"], N, seed=1)
        Wm = torch.eye(4).repeat(B, 1, 1)  # candidate poses around the identity: translations of up to 2 cm
        Wm[:, :3, 3] = (torch.rand(B, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1) * 0.02
        Wm = Wm.cuda()
        rng = np.random.default_rng(3)
        kinds = torch.from_numpy(rng.integers(0, 4, size=N).astype(np.uint8)).cuda()
        targets = torch.from_numpy(rng.uniform(-0.02, 0.02, size=N).astype(np.float32)).cuda()
        for mode_name, c in caches.items():
            mode = _lib.LEAF_MODES[mode_name]
            # delta for about a fifth of outliers: from the residuals of the first pose's active pairs
            x = torch.empty((1, N, 3), dtype=torch.float32, device=dev)
            _lib.check(_lib.load().pvamd_transform_points(_lib.ptr(Wm), 1, _lib.ptr(pts), N, _lib.ptr(x), _lib.stream_ptr()),
                       "pvamd_transform_points")
            r = c(x)[0].reshape(-1).double() - targets.double()
            active = (kinds == 0) | ((kinds == 1) & (r < 0)) | ((kinds == 2) & (r > 0))
            delta = float(torch.quantile(r[active].abs()[:1 << 20], 0.8))
            configs = {"degenerate": (None, None, math.inf), "mixed": (kinds, targets, math.inf),
                       "outliers": (kinds, targets, delta)}
            old = reg._Evaluator(c, mode, dev, pts, B)
            row = {"B": B, "N": N, "mode": mode_name, "delta": delta,
                   "chamfer_ms": median_ms(graphed(lambda: old(Wm)), args.regions, args.iters)}
            if args.parent_lib:
                parent = parent_evaluator(args.parent_lib, c, mode, Wm, pts)
                row["chamfer_parent_ms"] = median_ms(graphed(parent), args.regions, args.iters)
                old(Wm)
                torch.cuda.synchronize()
                row["parent_bits_equal"] = bool(torch.equal(parent.sums, old.sums))
            for name, (k, t, d) in configs.items():
                ev = reg._SemanticEvaluator(c, mode, dev, pts, B, k, t, d)
                ms = median_ms(graphed(lambda: ev(Wm)), args.regions, args.iters)
                torch.cuda.synchronize()
                counts = ev.counts.sum(0).tolist()
                generic = reg._SemanticEvaluator(c, None, dev, pts, B, k, t, d)
                torch_ms = median_ms(lambda: generic(Wm), args.regions, max(1, args.iters // 2))
                row[name] = {"ms": ms, "torch_ms": torch_ms, "active": sum(counts[1:4]), "outliers": counts[4],
                             "outlier_share_of_active": counts[4] / max(1, sum(counts[1:4]))}
                if name == "degenerate":
                    old(Wm)
                    torch.cuda.synchronize()
                    row["degenerate_bits_equal"] = bool(torch.equal(ev.sums, old.sums))
            rows.append(row)
            print(json.dumps(row))
    head = "| B x N | mode | chamfer ms |" + (" chamfer (parent build) ms |" if args.parent_lib else "")
    lines = [head + " degenerate ms | mixed ms | outliers ms | outlier share | x chamfer: degenerate / mixed / outliers | "
             "torch ops ms: degenerate / mixed / outliers |", "|---" * (head.count("|") - 1 + 6) + "|"]
    for r in rows:
        d, m, o = r["degenerate"], r["mixed"], r["outliers"]
        base = r["chamfer_ms"]
        lines.append(f"| {r['B']:,} x {r['N']:,} | {r['mode']} | {base:.4f} |"
                     + (f" {r['chamfer_parent_ms']:.4f} |" if args.parent_lib else "")
                     + f" {d['ms']:.4f} | {m['ms']:.4f} | {o['ms']:.4f} | {o['outlier_share_of_active']:.3f} | "
                     f"{d['ms'] / base:.2f} / {m['ms'] / base:.2f} / {o['ms'] / base:.2f} | "
                     f"{d['torch_ms']:.3f} / {m['torch_ms']:.3f} / {o['torch_ms']:.3f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
