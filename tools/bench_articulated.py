"""pv.joint_normal_equations / pv.refine_joint_configuration (csrc/articulated.hip) on two robots -- tests/fk_ref.py's TREE (12
leaves, 8 joints, branches, prismatic joints; caches at 0.02 m) and the 8-link arm of workloads.build_c4 (8 leaves, 7 joints) --
for A in {1, 64} configurations and N in {15,251, 262,144} points sampled from the links' surfaces at the first configuration
(grouped by link, 5 mm of jitter: the coherent cloud of a depth image), with kinds, targets and Huber weights switched on:

  eval       one evaluation: configure, pvamd_joint_normal_eq, pvamd_chain_twists, pvamd_joint_assemble (a graph replay)
  refine10   refine_joint_configuration(iterations=10): eleven evaluations and steps (a graph replay)
  baseline   what a caller could write before: robot(points), one one-leaf query per leaf for the first-minimum winner mask,
             then one semantic_normal_equations call per (configuration, leaf) on the masked kinds and a float64 torch assembly
             with the twist Jacobians (taken from pvamd_chain_twists here, so their cost is not in the figure); timed eagerly

Every --parent-lib (the option repeats) names another build of the library, a parent commit's say: one evaluation through its
entry points, called by address through a handle of their own in the same process into buffers of their own, is timed in regions
that alternate with this build's (eval_parent_ms) and its sums compared bit for bit (parent_bits_equal).  Two builds of one source
give the spread a difference has to exceed.  --eval-only leaves refine10 and the baseline out.

HIP-event timings after a warm-up, median of --regions regions.  Prints one JSON line per row and writes the markdown table to
--out.

  python tools/bench_articulated.py [--regions 11] [--iters 3] [--parent-lib libpvamd.so]... [--eval-only] [--out table.md]
"""
import argparse
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pytorch_volumetric_amd as pv  # noqa: E402
import workloads as W  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402
from pytorch_volumetric_amd import articulated as art  # noqa: E402
from pytorch_volumetric_amd import registration as reg  # noqa: E402
from pytorch_volumetric_amd import transforms as tf  # noqa: E402
from bench_min_over_points import alternate, parent_library  # noqa: E402
from bench_registration import graphed, median_ms  # noqa: E402

CONFIGS = (1, 64)
COUNTS = (15251, 262144)
DELTA = 0.01


def tree_robot(tmp, interpolation):
    from tests import fk_ref, test_fk_tree
    chain = pv.build_chain_from_urdf(test_fk_tree.write_robot(fk_ref.TREE, tmp))
    return pv.RobotSDF(chain, path_prefix=tmp, link_sdf_cls=pv.cache_link_sdf_factory(
        resolution=test_fk_tree.RES, padding=test_fk_tree.PADDING, device="cuda", cache_path=None, interpolation=interpolation))


def arm_robot(interpolation):
    robot = W.build_c4()
    for leaf in robot.sdf.sdfs:
        leaf.interpolation = interpolation
    return robot


def stack_of(robot, q32):
    A, M, S = q32.shape[0], len(robot.joint_names), len(robot.sdf_to_link_name)
    return robot._configure(_lib.load(), q32.device, q32, A, M, S, robot._offset_inv_dev(q32.device))


def surface_cloud(robot, q_row, n, seed, jitter=0.005):
    """n points of the links' surfaces under q_row, link after link, in the object frame, float32 on the device."""
    S = len(robot.sdf_to_link_name)
    to_object = tf.rigid_inverse(stack_of(robot, q_row[None].contiguous()))
    per = -(-n // S)
    out = []
    for s, factory in enumerate(robot.link_factories):
        p = pv.sample_mesh_points(factory, num_points=per, seed=seed + s, dbpath=None, device="cuda")[0].to(torch.float32)
        out.append(p @ to_object[s, :3, :3].T + to_object[s, :3, 3])
    pts = torch.cat(out)[:n]
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (pts + (torch.rand(pts.shape, generator=g, device="cuda") * 2 - 1) * jitter).contiguous()


def baseline(robot, q32, pts, kinds, targets, delta, J, scale=1000.):
    """The joint-space normal equations from the entry points the package had before (the docstring above)."""
    A, S = q32.shape[0], len(robot.sdf_to_link_name)
    robot.set_joint_configuration(q32)
    v = robot(pts)[0].reshape(A, -1)
    stack = robot.sdf._tf_matrix.reshape(S, A, 4, 4)
    taken = torch.zeros_like(v, dtype=torch.bool)
    cost = torch.zeros((A,), dtype=torch.float64, device=pts.device)
    g = torch.zeros((A, J.shape[-1]), dtype=torch.float64, device=pts.device)
    H = torch.zeros((A, J.shape[-1], J.shape[-1]), dtype=torch.float64, device=pts.device)
    ignore = torch.full_like(kinds, pv.POINT_IGNORE)
    for s, leaf in enumerate(robot.sdf.sdfs):
        one = pv.ComposedSDF([leaf], None)
        one.set_transforms(stack[s], batch_dim=(A,))
        mine = (one(pts)[0].reshape(A, -1) == v) & ~taken  # the first leaf that attains the minimum
        taken |= mine
        for a in range(A):
            ne = pv.semantic_normal_equations(stack[s, a:a + 1], pts, leaf, scale=scale, semantics=torch.where(mine[a], kinds, ignore),
                                              targets=targets, huber_delta=delta)
            Js = J[a, s]
            cost[a] += ne.cost[0]
            g[a] += Js.T @ ne.gradient[0]
            H[a] += Js.T @ ne.hessian[0] @ Js
    return cost, g, H


PARENT_ENTRIES = ("pvamd_configure_chain", "pvamd_joint_normal_eq", "pvamd_chain_twists", "pvamd_joint_assemble")


def parent_evaluation(lib, ev, q32):
    """art._Evaluator.__call__ through another build's entry points, on ev's buffers."""
    def run():
        stream = _lib.stream_ptr()
        ev.robot._configure(lib, ev.dev, q32, ev.A, ev.M, ev.S, ev.offset_inv, stack=ev.stack)
        _lib.check(lib.pvamd_joint_normal_eq(_lib.ptr(ev.grids), ev.S, ev.mode, _lib.ptr(ev.stack), ev.A, _lib.ptr(ev.pts), ev.N,
                                             _lib.ptr(ev.kinds), _lib.ptr(ev.targets), ev.delta, _lib.ptr(ev.leaf_sums),
                                             _lib.ptr(ev.leaf_counts), _lib.ptr(ev.scratch), stream), "pvamd_joint_normal_eq (parent)")
        _lib.check(lib.pvamd_chain_twists(_lib.ptr(ev.joints), ev.F, _lib.ptr(q32), ev.A, ev.M, _lib.ptr(ev.offset_inv), ev.S,
                                          _lib.ptr(ev.J), stream), "pvamd_chain_twists (parent)")
        _lib.check(lib.pvamd_joint_assemble(_lib.ptr(ev.leaf_sums), _lib.ptr(ev.leaf_counts), _lib.ptr(ev.J), ev.A, ev.S, ev.M,
                                            _lib.ptr(ev.sums), _lib.ptr(ev.counts), stream), "pvamd_joint_assemble (parent)")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--parent-lib", action="append", default=[], help="another build of libpvamd.so to time side by side (repeats)")
    ap.add_argument("--eval-only", action="store_true", help="leave refine10 and the baseline out")
    ap.add_argument("--out", default=None, help="also write the markdown table here (profiles/articulated.md quotes it)")
    args = ap.parse_args()
    parent_libs = [parent_library(path, PARENT_ENTRIES) for path in args.parent_lib]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("nearest", "trilinear"):
            for name, robot in (("tree", tree_robot(tmp, mode)), ("arm", arm_robot(mode))):
                S, M, leaf_mode = art._check_robot(robot)
                g = torch.Generator().manual_seed(4)
                for A in CONFIGS:
                    q0 = torch.randn(M, generator=g) * 0.3
                    q32 = (q0 + torch.randn(A, M, generator=g) * 0.03).to(dev).contiguous()
                    q32[0] = q0.to(dev)
                    for N in COUNTS:
                        pts = surface_cloud(robot, q32[0], N, seed=7)
                        rng = np.random.default_rng(3)
                        kinds = torch.from_numpy(rng.integers(0, 4, size=N)).cuda()
                        targets = torch.from_numpy(rng.uniform(-0.005, 0.005, size=N).astype(np.float32)).cuda()
                        k8 = reg._prepare_semantics(kinds, None, dev)[0]
                        ev = art._Evaluator(robot, S, M, leaf_mode, dev, pts, A, k8, targets, DELTA)
                        kw = dict(semantics=kinds, targets=targets, huber_delta=DELTA)
                        parents = [art._Evaluator(robot, S, M, leaf_mode, dev, pts, A, k8, targets, DELTA) for _ in parent_libs]
                        ms = alternate({"this": graphed(lambda: ev(q32)),
                                        **{i: graphed(parent_evaluation(lib, p, q32)) for i, (lib, p) in enumerate(zip(parent_libs, parents))}},
                                       args.regions, args.iters)
                        torch.cuda.synchronize()
                        row = {"robot": name, "S": S, "M": M, "mode": mode, "A": A, "N": N,
                               "slab_bytes": _lib.joint_normal_eq_scratch_bytes(A, S, N), "eval_ms": ms["this"],
                               "eval_parent_ms": [ms[i] for i in range(len(parents))],
                               "parent_bits_equal": [bool(torch.equal(p.sums, ev.sums) and torch.equal(p.leaf_sums, ev.leaf_sums)
                                                          and torch.equal(p.counts, ev.counts)) for p in parents],
                               "leaves_observed": int((ev.counts[0, _lib.SEM_COUNTS:] > 0).sum())}
                        if not args.eval_only:
                            row["refine10_ms"] = median_ms(graphed(lambda: pv.refine_joint_configuration(robot, q32, pts, iterations=10,
                                                                                                          **kw)), args.regions, 1)
                        if mode == "nearest" and not args.eval_only:
                            ne = pv.joint_normal_equations(robot, q32, pts, **kw)
                            row["baseline_ms"] = median_ms(lambda: baseline(robot, q32, pts, kinds, targets, DELTA, ev.J), 3, 1)
                            cost, gq, Hq = baseline(robot, q32, pts, kinds, targets, DELTA, ev.J)
                            row["baseline_cost_rel_diff"] = float(((cost - ne.cost).abs() / ne.cost.abs().clamp_min(1e-300)).max())
                            row["baseline_hessian_rel_diff"] = float((Hq - ne.hessian).abs().max() / ne.hessian.abs().max())
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    lines = ["| robot | mode | A x N | eval ms" + "".join(f" / {path}" for path in args.parent_lib) + " | refine10 ms | "
             "baseline eval ms | baseline / eval | slab MB | leaves observed |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r.get("baseline_ms", math.nan)
        lines.append(f"| {r['robot']} (S {r['S']}, M {r['M']}) | {r['mode']} | {r['A']} x {r['N']:,} | "
                     + " / ".join(f"{v:.4f}" for v in [r["eval_ms"]] + r["eval_parent_ms"])
                     + f" | {r.get('refine10_ms', math.nan):.3f} | {b:.3f} | {b / r['eval_ms']:.0f} | {r['slab_bytes'] / 1e6:.2f} | "
                     f"{r['leaves_observed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
