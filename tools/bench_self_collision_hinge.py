"""RobotSDF.self_collision_hinge (csrc/leaf_pair.hip) against what a caller writes without it: HIP-event timings after a warm-up,
median of --regions regions, the variants alternated in one process on the same inputs.  The cases of
tools/bench_self_collision.py (the synthetic 8-link arm, its 42 default ordered pairs; C4 and README link grids, nearest and
trilinear leaves, A in {1, 200, 1000}, 256 and 1024 surface points per link), margin 0.2, power 2:
  (a) self_collision_hinge(m)                                    the fused kernels
  (b) the generic per-pair path: one one-leaf hinge_over_points per pair under the kernel's pair transforms
  (c) the torch recipe of tools/bench_self_collision.py with the hinge sum in place of the minimum
and forward + backward to q of the same three.  "bwd" times the new backward alone: torch.autograd.grad of (a)'s values w.r.t.
a composition stack that requires grad (no chain), forward included, next to the forward alone on that composition.  Prints
one JSON line per case and writes the markdown table to --out.

With --parent-lib (the option repeats; another build of the library, a parent commit's say) it times instead that backward
alone -- torch.autograd.grad of the kept forward w.r.t. the stack -- through this build and through every parent's entry points
in alternating regions (bench_min_over_points.against_parents), one JSON line per case with parent_bits_equal.

  python tools/bench_self_collision_hinge.py [--regions 7] [--iters 3] [--out table.md] [--parent-lib libpvamd.so]...
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import transforms as tf  # noqa: E402
from bench_min_over_points import against_parents, alternate, parent_library  # noqa: E402
from bench_self_collision import build  # noqa: E402

MARGIN, POWER = 0.2, 2


def recipe(r, pairs, m=MARGIN, power=POWER):
    """(c): the hand-written torch version -- values (A, K), differentiable through the stack and the leaves' __call__."""
    comp = r.sdf
    S = len(comp.sdfs)
    stack = comp._tf_matrix.reshape(S, -1, 4, 4)
    out = []
    for s, t in pairs.tolist():
        p = r._sc_points[t]
        link_to_obj = tf.rigid_inverse(stack[t])
        x = p @ link_to_obj[:, :3, :3].transpose(1, 2) + link_to_obj[:, None, :3, 3]
        y = x @ stack[s][:, :3, :3].transpose(1, 2) + stack[s][:, None, :3, 3]
        out.append(((m - comp.sdfs[s](y)[0]).clamp(min=0) ** power).sum(dim=-1))
    return torch.stack(out, dim=-1)


def variants(r, pairs):
    plan = r.sdf._leaf_pair_plan(r._sc_points, pairs)
    return {
        "a_fused": lambda: r.self_collision_hinge(MARGIN, POWER, pairs),
        "b_generic": lambda: r.sdf._leaf_pair_hinge_generic(plan, MARGIN, POWER),
        "c_torch": lambda: recipe(r, pairs),
    }


def fwd_bwd(r, q, pairs):
    plan = r.sdf._leaf_pair_plan(r._sc_points, pairs)

    def step(f):
        def run():
            r.set_joint_configuration(q.clone().requires_grad_())
            f().sum().backward()
        return run
    return {
        "a_fused": step(lambda: r.self_collision_hinge(MARGIN, POWER, pairs).values),
        "b_generic": step(lambda: r.sdf._leaf_pair_hinge_generic(plan, MARGIN, POWER).values),
        "c_torch": step(lambda: recipe(r, pairs)),
    }


def stack_only(r, pairs):
    """The new kernels without the chain: forward alone, and forward + backward to a stack that requires grad."""
    A = r.sdf._tf_matrix.shape[0] // len(r.sdf.sdfs)
    tfm = r.sdf._tf_matrix.detach().clone().requires_grad_()
    comp = pv.ComposedSDF(list(r.sdf.sdfs), None)
    comp.set_transforms(tfm, batch_dim=(A,), known_rigid=True)
    pts = r._sc_points

    def fwd():
        with torch.no_grad():
            comp.leaf_pair_hinge(pts, pairs, MARGIN, POWER)

    def fb():
        torch.autograd.grad(comp.leaf_pair_hinge(pts, pairs, MARGIN, POWER).values.sum(), tfm)
    return {"stack_fwd": fwd, "stack_fwd_bwd": fb}


def backward_against_parents(r, pairs, parents, regions, iters):
    """stack_only's backward without its forward, this build against `parents`."""
    A = r.sdf._tf_matrix.shape[0] // len(r.sdf.sdfs)
    tfm = r.sdf._tf_matrix.detach().clone().requires_grad_()
    comp = pv.ComposedSDF(list(r.sdf.sdfs), None)
    comp.set_transforms(tfm, batch_dim=(A,), known_rigid=True)
    out = comp.leaf_pair_hinge(r._sc_points, pairs, MARGIN, POWER).values.sum()
    return against_parents(lambda: torch.autograd.grad(out, tfm, retain_graph=True), parents, regions, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", action="append", default=[], help="another build of libpvamd.so to time the backward against (repeats)")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the markdown table here (profiles/self_collision_hinge.md quotes it)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    parents = [parent_library(path) for path in args.parent_lib]
    rows = []
    for grid, padding in (("C4", 0.1), ("README", 1.0)):
        for mode in ("nearest", "trilinear"):
            r = build(padding, mode)
            pairs = r.self_collision_pairs()
            for npts in (256, 1024):
                r.set_self_collision_points(num_points=npts, seed=0)
                for A in (1, 200, 1000):
                    q = W.c4_joint_configs(A, seed=0).cuda()
                    r.set_joint_configuration(q)
                    if parents:
                        row = {"grid": grid, "mode": mode, "points": npts, "configs": A, "pairs": int(pairs.shape[0])}
                        row.update(backward_against_parents(r, pairs, parents, args.regions, args.iters))
                        print(json.dumps(row), flush=True)
                        continue
                    # the fused and generic paths agree bit for bit, the recipe within float32 rounding of the terms
                    a = r.self_collision_hinge(MARGIN, POWER, pairs).values
                    b = r.sdf._leaf_pair_hinge_generic(r.sdf._leaf_pair_plan(r._sc_points, pairs), MARGIN, POWER).values
                    assert torch.equal(a, b)
                    agree = float(((a - recipe(r, pairs)).abs() / (1e-6 + a.abs())).max())
                    t = alternate(variants(r, pairs), args.regions, args.iters)
                    fb = alternate(fwd_bwd(r, q, pairs), args.regions, max(1, args.iters // 2))
                    r.set_joint_configuration(q)
                    so = alternate(stack_only(r, pairs), args.regions, args.iters)
                    rows.append({"grid": grid, "mode": mode, "points": npts, "configs": A, "pairs": int(pairs.shape[0]),
                                 "fwd_ms": t, "fwd_bwd_ms": fb, "stack_ms": so, "max_rel_diff_torch": agree})
                    print(json.dumps(rows[-1]), flush=True)
            del r
            torch.cuda.empty_cache()
    if parents:
        return
    lines = ["| grid | leaves | pts/link | A | (a) fused ms | (b) per-pair ms | (c) torch ms | b / a | c / a | "
             "fwd+bwd to q (a) ms | (b) ms | (c) ms | stack fwd ms | stack fwd+bwd ms | bwd alone ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        f, fb, so = row["fwd_ms"], row["fwd_bwd_ms"], row["stack_ms"]
        lines.append(f"| {row['grid']} | {row['mode']} | {row['points']} | {row['configs']} | {f['a_fused']:.4f} | "
                     f"{f['b_generic']:.4f} | {f['c_torch']:.4f} | {f['b_generic'] / f['a_fused']:.1f} | "
                     f"{f['c_torch'] / f['a_fused']:.1f} | {fb['a_fused']:.3f} | {fb['b_generic']:.3f} | {fb['c_torch']:.3f} | "
                     f"{so['stack_fwd']:.4f} | {so['stack_fwd_bwd']:.4f} | {so['stack_fwd_bwd'] - so['stack_fwd']:.4f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
