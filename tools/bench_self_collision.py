"""RobotSDF.self_collision_distance (csrc/leaf_pair.hip) against what a caller writes without it: HIP-event timings after a
warm-up, median of --regions regions, the variants alternated in one process on the same inputs.  The synthetic 8-link arm
(workloads.synthetic_arm, its 42 default ordered pairs) with C4 link grids (cache_link_sdf_factory(0.02, 0.1)) and README grids
(padding=1.0), nearest and trilinear leaves, A in {1, 200, 1000} configurations, 256 and 1024 surface points per link:
  (a) self_collision_distance()                                the fused kernels
  (b) the generic per-pair path: one one-leaf min_over_points per pair under the kernel's pair transforms
  (c) the torch recipe: per pair, leaf t's points moved into leaf s's frame under every configuration (rigid_inverse, matmul,
      an (A, P, 3) tensor), leaf s's __call__ on them, min over the points
and forward + backward to q of the same three.  Prints one JSON line per case and writes the markdown table to --out.

  python tools/bench_self_collision.py [--regions 9] [--iters 5] [--out table.md]
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
from pytorch_volumetric_amd import transforms as tf  # noqa: E402
from bench_min_over_points import alternate  # noqa: E402


def build(padding, interpolation):
    with tempfile.TemporaryDirectory() as tmp:
        chain = W.synthetic_arm(tmp)
        return pv.RobotSDF(chain, path_prefix=tmp, link_sdf_cls=pv.cache_link_sdf_factory(
            0.02, padding, device="cuda", cache_path=None, interpolation=interpolation))


def recipe(r, pairs):
    """(c): the hand-written torch version -- values (A, K), differentiable through the stack and the leaves' __call__."""
    comp = r.sdf
    S = len(comp.sdfs)
    stack = comp._tf_matrix.reshape(S, -1, 4, 4)
    out = []
    for s, t in pairs.tolist():
        p = r._sc_points[t]
        link_to_obj = tf.rigid_inverse(stack[t])                                    # (A, 4, 4) leaf t -> robot frame
        x = p @ link_to_obj[:, :3, :3].transpose(1, 2) + link_to_obj[:, None, :3, 3]  # (A, P, 3) in the robot frame
        y = x @ stack[s][:, :3, :3].transpose(1, 2) + stack[s][:, None, :3, 3]      # (A, P, 3) in leaf s's frame
        out.append(comp.sdfs[s](y)[0].min(dim=-1).values)
    return torch.stack(out, dim=-1)


def variants(r, pairs):
    plan = r.sdf._leaf_pair_plan(r._sc_points, pairs)
    return {
        "a_fused": lambda: r.self_collision_distance(pairs),
        "b_generic": lambda: r.sdf._leaf_pair_generic(plan),
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
        "a_fused": step(lambda: r.self_collision_distance(pairs).values),
        "b_generic": step(lambda: r.sdf._leaf_pair_generic(plan).values),
        "c_torch": step(lambda: recipe(r, pairs)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the markdown table here (profiles/self_collision.md quotes it)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
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
                    # the three agree (values): the fused and generic paths bit for bit, the recipe within float32 rounding
                    a, b = r.self_collision_distance(pairs).values, r.sdf._leaf_pair_generic(
                        r.sdf._leaf_pair_plan(r._sc_points, pairs)).values
                    assert torch.equal(a, b)
                    c = recipe(r, pairs)
                    agree = float((a - c).abs().max())
                    t = alternate(variants(r, pairs), args.regions, args.iters)
                    fb = alternate(fwd_bwd(r, q, pairs), args.regions, max(1, args.iters // 2))
                    r.set_joint_configuration(q)
                    rows.append({"grid": grid, "mode": mode, "points": npts, "configs": A, "pairs": int(pairs.shape[0]),
                                 "fwd_ms": t, "fwd_bwd_ms": fb, "max_abs_diff_torch": agree})
                    print(json.dumps(rows[-1]), flush=True)
            del r
            torch.cuda.empty_cache()
    lines = ["| grid | leaves | pts/link | A | (a) fused ms | (b) per-pair ms | (c) torch ms | a / b | a / c | "
             "fwd+bwd (a) ms | (b) ms | (c) ms | a / b | a / c |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        f, fb = row["fwd_ms"], row["fwd_bwd_ms"]
        lines.append(f"| {row['grid']} | {row['mode']} | {row['points']} | {row['configs']} | {f['a_fused']:.4f} | "
                     f"{f['b_generic']:.4f} | {f['c_torch']:.4f} | {f['a_fused'] / f['b_generic']:.2f} | "
                     f"{f['a_fused'] / f['c_torch']:.2f} | {fb['a_fused']:.3f} | {fb['b_generic']:.3f} | {fb['c_torch']:.3f} | "
                     f"{fb['a_fused'] / fb['b_generic']:.2f} | {fb['a_fused'] / fb['c_torch']:.2f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
