"""chamfer_normal_equations and refine_poses (csrc/registration.hip) on the drill cache at 0.01 m, nearest and trilinear, for
B x N in {1 x 1M, 64 x 16K, 1024 x 512, 10,000 x 500}: HIP-event timings of graph replays after a warm-up, median of --regions
regions.  Next to them what a caller had before: one first-order evaluation, batch_chamfer_dist(...).sum().backward() with
W.requires_grad_() on the trilinear cache (eager: autograd is not captured).  The roofline figure is bench_legs.py's
bytes-per-pair one: the 12 B point read per (pose, point) pair -- nothing is written per pair -- against 8 TB/s.
Prints one JSON line per case and writes the markdown table to --out.

  python tools/bench_registration.py [--regions 21] [--iters 5] [--out table.md]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402
from bench_legs import HBM_PEAK_GBS  # noqa: E402
from bench_min_over_points import region_ms  # noqa: E402

BYTES_PER_PAIR = 12
CASES = ((1, 1 << 20), (64, 16384), (1024, 512), (10_000, 500))


def graphed(fn):
    """fn captured once (after a warm-up that builds descriptors and loads code objects); returns the replay."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def median_ms(fn, regions, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return statistics.median(region_ms(fn, iters) for _ in range(regions))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the markdown table here (profiles/registration.md quotes it)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    caches = {"nearest": W.build_c2_cache(), "trilinear": W.build_c2_cache()}
    caches["trilinear"].interpolation = "trilinear"
    rows = []
    for B, N in CASES:
        pts = W.c2_points(caches["nearest"], N, seed=1)
        Wm = torch.eye(4).repeat(B, 1, 1)  # candidate poses around the identity: translations of up to 2 cm
        Wm[:, :3, 3] = (torch.rand(B, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1) * 0.02
        Wm = Wm.cuda()
        row = {"B": B, "N": N}
        for mode, c in caches.items():
            ne = median_ms(graphed(lambda: pv.chamfer_normal_equations(Wm, pts, c)), args.regions, args.iters)
            lm = median_ms(graphed(lambda: pv.refine_poses(Wm, pts, c, iterations=10)), args.regions, max(1, args.iters // 2))
            row[mode] = {"normal_eq_ms": ne, "refine10_ms": lm, "normal_eq_GBs": BYTES_PER_PAIR * B * N / ne / 1e6,
                         "normal_eq_frac_of_hbm_peak": BYTES_PER_PAIR * B * N / ne / 1e6 / HBM_PEAK_GBS}

        def first_order():
            Wg = Wm.clone().requires_grad_()
            with torch.enable_grad():
                pv.batch_chamfer_dist(Wg, pts, obj_sdf=caches["trilinear"]).sum().backward()
        row["first_order_fwd_bwd_trilinear_ms"] = median_ms(first_order, args.regions, max(1, args.iters // 2))
        rows.append(row)
        print(json.dumps(row))
    lines = ["| B x N | normal eq nearest ms | normal eq trilinear ms | 12 B/pair GB/s (nearest) | share of 8 TB/s | "
             "refine x10 nearest ms | refine x10 trilinear ms | first-order fwd+bwd (trilinear, eager) ms |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        n, t = r["nearest"], r["trilinear"]
        lines.append(f"| {r['B']:,} x {r['N']:,} | {n['normal_eq_ms']:.4f} | {t['normal_eq_ms']:.4f} | {n['normal_eq_GBs']:.1f} | "
                     f"{n['normal_eq_frac_of_hbm_peak']:.4f} | {n['refine10_ms']:.3f} | {t['refine10_ms']:.3f} | "
                     f"{r['first_order_fwd_bwd_trilinear_ms']:.3f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
