"""hinge_over_points (csrc/hinge_over_points.hip) against what a caller writes without it: HIP-event timings after a warm-up,
median of --regions regions, the variants alternated in one process on the same inputs.  Cases: C4 (RobotSDF, 8 links of
100 KB, A = 200, P = 262,144) with nearest and trilinear leaves, and C3 (8 placed drills, one configuration, 4M points); per case
  (a) __call__ then ((m - v).clamp(min=0) ** 2).sum(-1)     (b) hinge_over_points()     (c) hinge_over_points(per_leaf=True)
and forward + backward to q (C4) or to the transforms (C3) of (a) against (b).  Prints one JSON line per case and writes the
markdown table to --out.

With --parent-lib (the option repeats; another build of the library, a parent commit's say) it times instead the backward of (b)
alone -- torch.autograd.grad of the kept forward w.r.t. the transform stack -- through this build and through every parent's
entry points in alternating regions (bench_min_over_points.against_parents), one JSON line per case with parent_bits_equal.

  python tools/bench_hinge_over_points.py [--regions 15] [--iters 10] [--out table.md] [--parent-lib libpvamd.so]...
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402
from bench_min_over_points import against_parents, alternate, parent_library  # noqa: E402

MARGIN = 0.02


def variants(comp, pts):
    return {
        "a_call_expr": lambda: ((MARGIN - comp(pts)[0]).clamp(min=0) ** 2).sum(-1),
        "b_fused": lambda: comp.hinge_over_points(pts, MARGIN),
        "c_fused_per_leaf": lambda: comp.hinge_over_points(pts, MARGIN, per_leaf=True),
    }


def fwd_bwd(set_input, call, pts):
    """(a) and (b) of one optimiser step: set the differentiable input, the forward, .sum().backward()."""
    def fb_a():
        comp = set_input()
        ((MARGIN - call(comp)(pts)[0]).clamp(min=0) ** 2).sum().backward()

    def fb_b():
        comp = set_input()
        call(comp).hinge_over_points(pts, MARGIN).values.sum().backward()
    return {"a_call_expr": fb_a, "b_fused": fb_b}


def backward_against_parents(case, mode, comp, stack, pts, parents, regions, iters):
    """comp's stack requires grad: the backward of hinge_over_points to it alone, this build against `parents`."""
    out = comp.hinge_over_points(pts, MARGIN).values.sum()
    row = {"case": case, "mode": mode, "stack_rows": stack.shape[0], "points": pts.shape[0]}
    row.update(against_parents(lambda: torch.autograd.grad(out, stack, retain_graph=True), parents, regions, iters))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", action="append", default=[], help="another build of libpvamd.so to time the backward against (repeats)")
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the markdown table here (profiles/hinge_over_points.md quotes it)")
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
    parents = [parent_library(path) for path in args.parent_lib]
    for mode, r in robots.items():
        if parents:
            r.set_joint_configuration(q.clone().requires_grad_())
            backward_against_parents("C4", mode, r, r.sdf._tf_matrix, pts, parents, args.regions, args.iters)
            continue
        r.set_joint_configuration(q)
        t = alternate(variants(r, pts), args.regions, args.iters)

        def set_q(r=r):
            r.set_joint_configuration(q.clone().requires_grad_())
            return r
        fb = alternate(fwd_bwd(set_q, lambda comp: comp, pts), args.regions, max(1, args.iters // 2))
        r.set_joint_configuration(q)
        rows.append({"case": "C4", "mode": mode, "configs": A, "points": P, "leaves": len(r.sdf.sdfs), "fwd_ms": t, "fwd_bwd_ms": fb})

    caches = {"nearest": W.build_c2_cache(), "trilinear": W.build_c2_cache()}
    caches["trilinear"].interpolation = "trilinear"
    P3 = 1 << 22
    pts3 = W.c3_points(P3, seed=0)
    for mode, c in caches.items():
        comp = W.build_c3(c)
        if parents:
            stack = comp._tf_matrix.detach().clone().requires_grad_()
            comp.set_transforms(stack, batch_dim=comp.tsf_batch, known_rigid=True)
            backward_against_parents("C3", mode, comp, stack, pts3, parents, args.regions, args.iters)
            continue
        t = alternate(variants(comp, pts3), args.regions, args.iters)
        tfm = comp._tf_matrix.detach().clone()
        batch = comp.tsf_batch

        def set_tf(comp=comp, tfm=tfm, batch=batch):
            comp.set_transforms(tfm.clone().requires_grad_(), batch_dim=batch, known_rigid=True)
            return comp
        fb = alternate(fwd_bwd(set_tf, lambda cc: cc, pts3), args.regions, max(1, args.iters // 2))
        comp.set_transforms(tfm, batch_dim=batch, known_rigid=True)
        rows.append({"case": "C3", "mode": mode, "configs": 1, "points": P3, "leaves": 8, "fwd_ms": t, "fwd_bwd_ms": fb})

    if parents:
        return
    for row in rows:
        print(json.dumps(row))
    lines = ["| case | leaves | (a) call + expr ms | (b) fused ms | (c) fused per leaf ms | b / a | fwd+bwd (a) ms | "
             "fwd+bwd (b) ms | b / a |", "|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        f, fb = row["fwd_ms"], row["fwd_bwd_ms"]
        lines.append(f"| {row['case']} {row['mode']} ({row['configs']} x {row['points']:,}) | {row['leaves']} | "
                     f"{f['a_call_expr']:.4f} | {f['b_fused']:.4f} | {f['c_fused_per_leaf']:.4f} | "
                     f"{f['b_fused'] / f['a_call_expr']:.2f} | {fb['a_call_expr']:.3f} | {fb['b_fused']:.3f} | "
                     f"{fb['b_fused'] / fb['a_call_expr']:.2f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
