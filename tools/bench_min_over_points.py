"""min_over_points (csrc/min_over_points.hip) against what a caller writes without it: HIP-event timings after a warm-up, median of
--regions regions, the variants alternated in one process on the same inputs.  Cases: C4 (RobotSDF, 8 links of 100 KB, A = 200,
P = 262,144) and C3 (8 placed drills, one configuration, 4M points), nearest and trilinear leaves; per case
  (a) __call__ then .min(-1)                 (b) min_over_points()             (c) min_over_points(per_leaf=True)
  (d) S one-leaf compositions, each __call__ then .min(-1)
and, on C4, forward + backward to q of (a) against (b).  Prints one JSON line per case and writes the markdown table to --out.

  python tools/bench_min_over_points.py [--regions 15] [--iters 10] [--out profiles/min_over_points.md]
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402


def region_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(fns, regions, iters):
    for fn in fns.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(regions):
        for k, fn in fns.items():
            times[k].append(region_ms(fn, iters))
    return {k: statistics.median(v) for k, v in times.items()}


def parent_library(path, names=None):
    """Another build of libpvamd.so, a parent commit's say, through a handle of its own (so with code objects of its own in
    memory), its entry points `names` (default: all of include/pvamd.h) given the binding's signatures."""
    lib = ctypes.CDLL(path)
    for name in _lib.SIGNATURES if names is None else names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@contextlib.contextmanager
def through(lib):
    """Inside the block the package's own calls (_lib.load().pvamd_...) go to `lib`, a parent_library with all entry points."""
    saved, _lib._lib = _lib.load(), lib
    try:
        yield
    finally:
        _lib._lib = saved


def same_bits(a, b):
    ints = {4: torch.int32, 8: torch.int64}
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(ints[a.element_size()]), b.view(ints[b.element_size()])))


def against_parents(fn, parents, regions, iters):
    """fn() -> a tuple of tensors, computed through the package.  Timed as it is and with the package's library calls going to
    each of `parents` (parent_library handles), the regions of all of them alternating: the row's
    {"ms", "parent_ms": [...], "parent_bits_equal": [...]}, the last comparing every output of fn bit for bit.  Two builds of one
    parent give the spread a difference has to exceed."""
    def under(lib):
        def run():
            with through(lib):
                return fn()
        return run
    fns = {"this": under(_lib.load()), **{i: under(lib) for i, lib in enumerate(parents)}}  # the same host path for all of them
    ms = alternate(fns, regions, iters)
    outs = fns["this"]()
    mine = [t.clone() for t in outs]
    equal = []
    for i in range(len(parents)):
        for t in outs:  # where fn writes into buffers of its own, a parent that wrote nothing must not pass on this build's bits
            t.fill_(float("nan"))
        outs = theirs = fns[i]()
        equal.append(len(theirs) == len(mine) and all(same_bits(a, b) for a, b in zip(mine, theirs)))
    torch.cuda.synchronize()
    return {"ms": ms["this"], "parent_ms": [ms[i] for i in range(len(parents))], "parent_bits_equal": equal}


def one_leaf_compositions(comp):
    out = []
    for s in range(len(comp.sdfs)):
        one = pv.ComposedSDF([comp.sdfs[s]], None)
        one.set_transforms(comp._tf_matrix.detach()[comp.ith_transform_slice(s)], batch_dim=comp.tsf_batch, known_rigid=True)
        out.append(one)
    return out


def variants(comp, pts):
    singles = one_leaf_compositions(comp)
    return {
        "a_call_min": lambda: comp(pts)[0].min(dim=-1),
        "b_fused": lambda: comp.min_over_points(pts),
        "c_fused_per_leaf": lambda: comp.min_over_points(pts, per_leaf=True),
        "d_single_leaf_min": lambda: [one(pts)[0].min(dim=-1) for one in singles],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_over_points.md"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []

    robots = {"nearest": W.build_c4()}
    with tempfile.TemporaryDirectory() as tmp:
        chain = W.synthetic_arm(tmp)
        robots["trilinear"] = pv.RobotSDF(chain, path_prefix=tmp, link_sdf_cls=pv.cache_link_sdf_factory(
            0.02, 0.1, device="cuda", cache_path=None, interpolation="trilinear"))
    A, P = 200, 262_144
    q = W.c4_joint_configs(A, seed=0).cuda()
    pts = W.c4_points(P, seed=1)
    for mode, r in robots.items():
        r.set_joint_configuration(q)
        t = alternate(variants(r.sdf, pts), args.regions, args.iters)

        def fb_a(r=r):
            qq = q.clone().requires_grad_()
            r.set_joint_configuration(qq)
            v, _ = r(pts)
            v.min(dim=-1).values.sum().backward()

        def fb_b(r=r):
            qq = q.clone().requires_grad_()
            r.set_joint_configuration(qq)
            r.min_over_points(pts).values.sum().backward()
        fb = alternate({"a_call_min": fb_a, "b_fused": fb_b}, args.regions, max(1, args.iters // 2))
        r.set_joint_configuration(q)
        rows.append({"case": "C4", "mode": mode, "configs": A, "points": P, "leaves": len(r.sdf.sdfs), "fwd_ms": t, "fwd_bwd_q_ms": fb})

    caches = {"nearest": W.build_c2_cache(), "trilinear": W.build_c2_cache()}
    caches["trilinear"].interpolation = "trilinear"
    P3 = 1 << 22
    pts3 = W.c3_points(P3, seed=0)
    for mode, c in caches.items():
        comp = W.build_c3(c)
        t = alternate(variants(comp, pts3), args.regions, args.iters)
        rows.append({"case": "C3", "mode": mode, "configs": 1, "points": P3, "leaves": 8, "fwd_ms": t, "fwd_bwd_q_ms": None})

    for row in rows:
        print(json.dumps(row))
    lines = ["| case | leaves | (a) call + min ms | (b) fused ms | (c) fused per leaf ms | (d) one-leaf calls + min ms | b / a | "
             "fwd+bwd (a) ms | fwd+bwd (b) ms |", "|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        f, fb = row["fwd_ms"], row["fwd_bwd_q_ms"]
        lines.append(f"| {row['case']} {row['mode']} ({row['configs']} x {row['points']:,}) | {row['leaves']} | {f['a_call_min']:.4f} | "
                     f"{f['b_fused']:.4f} | {f['c_fused_per_leaf']:.4f} | {f['d_single_leaf_min']:.4f} | "
                     f"{f['b_fused'] / f['a_call_min']:.2f} | " +
                     (f"{fb['a_call_min']:.3f} | {fb['b_fused']:.3f} |" if fb else "- | - |"))
    table = "\n".join(lines)
    print(table)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(table + "\n")


if __name__ == "__main__":
    main()
