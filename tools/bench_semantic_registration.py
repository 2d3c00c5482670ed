"""pvamd_semantic_normal_eq (csrc/registration.hip sem_partial_kernel) on the drill cache at 0.01 m, nearest and trilinear, for
B x N in {64 x 16,384, 1 x 2^20} -- the shapes of profiles/registration.md -- in three configurations:

  degenerate   no kinds, no targets, delta = inf (the sums of pvamd_chamfer_normal_eq bit for bit)
  mixed        kinds uniform in 0..3, targets uniform in +-0.02, delta = inf
  outliers     the same kinds and targets, delta at the 80th percentile of |r| over the first pose's active pairs

each next to two baselines: pvamd_chamfer_normal_eq of this build, and the same sums written in torch ops on (B, N) tensors (the
package's generic path, run on the cache's own query; --skip-torch leaves it out).  Every --parent-lib (the option repeats) names
another build of the library, a parent commit's say: its pvamd_chamfer_normal_eq and its pvamd_semantic_normal_eq in the three
configurations are called by address through a handle of their own in the same process, timed in regions that alternate with
this build's, and their sums compared bit for bit (parent_bits_equal).  Two builds of one source give the spread a difference has
to exceed.  HIP-event timings of graph replays after a warm-up, median of --regions regions; one replay is the two launches of an
evaluation into buffers allocated once.  The torch baseline is timed eagerly between the same events (its index tensors are
built from host lists, which a capture refuses): some thirty launches over (B, N) float64 tensors, whose device time is what
the figure mostly holds at these sizes.
Prints one JSON line per row and writes the markdown table to --out.

  python tools/bench_semantic_registration.py [--regions 21] [--iters 5] [--parent-lib libpvamd.so]... [--skip-torch] [--out table.md]
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
from bench_min_over_points import alternate, parent_library  # noqa: E402
from bench_registration import graphed, median_ms  # noqa: E402

CASES = ((64, 16384), (1, 1 << 20))


def parent_evaluator(path, c, mode, W32, pts, config=None):
    """pvamd_chamfer_normal_eq, or with config = (kinds, targets, delta) pvamd_semantic_normal_eq, of another build of the
    library, through a handle of its own."""
    name = "pvamd_chamfer_normal_eq" if config is None else "pvamd_semantic_normal_eq"
    lib = parent_library(path, (name, name + "_scratch_bytes"))
    fn, size = getattr(lib, name), getattr(lib, name + "_scratch_bytes")
    B, N = W32.shape[0], pts.shape[0]
    sums = torch.empty((B, _lib.REG_SUMS), dtype=torch.float64, device=pts.device)
    counts = torch.empty((B,) if config is None else (B, _lib.SEM_COUNTS), dtype=torch.int64, device=pts.device)
    scratch = _lib.scratch_buffer(size(B, N), pts.device)
    desc = c._grid_desc()
    extra = () if config is None else (_lib.ptr(config[0]), _lib.ptr(config[1]), config[2])

    def run():
        _lib.check(fn(ctypes.byref(desc), mode, _lib.ptr(W32), B, _lib.ptr(pts), N, *extra, _lib.ptr(sums), _lib.ptr(counts),
                      _lib.ptr(scratch), _lib.stream_ptr()), name + " (parent)")
    run.sums = sums
    return run


def against_parents(ev, parents, Wm, regions, iters):
    """(ms of ev, [ms of every parent], [its sums equal ev's bit for bit]), the regions of all of them alternating."""
    ms = alternate({"this": graphed(lambda: ev(Wm)), **{i: graphed(p) for i, p in enumerate(parents)}}, regions, iters)
    ev(Wm)
    for p in parents:
        p()
    torch.cuda.synchronize()
    return ms["this"], [ms[i] for i in range(len(parents))], [bool(torch.equal(p.sums, ev.sums)) for p in parents]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent-lib", action="append", default=[], help="another build of libpvamd.so to time side by side (repeats)")
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch-ops baseline out")
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
            old = reg._Evaluator(c, mode, dev, pts, B, plain=True)
            parents = [parent_evaluator(path, c, mode, Wm, pts) for path in args.parent_lib]
            row = {"B": B, "N": N, "mode": mode_name, "delta": delta}
            row["chamfer_ms"], row["chamfer_parent_ms"], row["parent_bits_equal"] = against_parents(old, parents, Wm, args.regions,
                                                                                                    args.iters)
            for name, (k, t, d) in configs.items():
                ev = reg._Evaluator(c, mode, dev, pts, B, k, t, d)
                parents = [parent_evaluator(path, c, mode, Wm, pts, (k, t, d)) for path in args.parent_lib]
                ms, parent_ms, equal = against_parents(ev, parents, Wm, args.regions, args.iters)
                counts = ev.counts.sum(0).tolist()
                row[name] = {"ms": ms, "parent_ms": parent_ms, "parent_bits_equal": equal, "active": sum(counts[1:4]),
                             "outliers": counts[4], "outlier_share_of_active": counts[4] / max(1, sum(counts[1:4]))}
                if not args.skip_torch:
                    generic = reg._Evaluator(c, None, dev, pts, B, k, t, d)
                    row[name]["torch_ms"] = median_ms(lambda: generic(Wm), args.regions, max(1, args.iters // 2))
                if name == "degenerate":
                    old(Wm)
                    torch.cuda.synchronize()
                    row["degenerate_bits_equal"] = bool(torch.equal(ev.sums, old.sums))
            rows.append(row)
            print(json.dumps(row), flush=True)
    cell = lambda ms, parent_ms: " / ".join(f"{v:.4f}" for v in [ms] + parent_ms)
    lines = ["| B x N | mode | chamfer ms | degenerate ms | mixed ms | outliers ms | outlier share | x chamfer: degenerate / mixed / "
             "outliers | torch ops ms: degenerate / mixed / outliers |", "|---" * 9 + "|"]
    if args.parent_lib:
        lines.insert(0, f"(every ms cell: this build / {' / '.join(args.parent_lib)})\n")
    for r in rows:
        d, m, o = r["degenerate"], r["mixed"], r["outliers"]
        base = r["chamfer_ms"]
        lines.append(f"| {r['B']:,} x {r['N']:,} | {r['mode']} | {cell(base, r['chamfer_parent_ms'])} | "
                     + " | ".join(cell(v["ms"], v["parent_ms"]) for v in (d, m, o))
                     + f" | {o['outlier_share_of_active']:.3f} | {d['ms'] / base:.2f} / {m['ms'] / base:.2f} / {o['ms'] / base:.2f} | "
                     + " / ".join(f"{v.get('torch_ms', math.nan):.3f}" for v in (d, m, o)) + " |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
