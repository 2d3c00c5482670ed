"""ray_cast(..., differentiable=True), forward plus backward (csrc/ray_cast.hip + csrc/ray_cast_backward.hip), against the same
gradient computed by the torch restatement of include/pvamd.h "Ray casting: gradient of the hit distance" on the GPU: the same
fused forward without a graph, then the contract's formula as torch ops on its outputs (float64 terms, index_add sums, the
winning leaf found by querying every one-leaf composition at the hit points).  There is no other baseline: without this call the
gradient does not exist.  The loss is sum((t d_z - depth)^2) over the rays that hit; both variants form its derivative
w.r.t. t by the same torch expression and differ only in what takes that upstream to the rays and the stack.

HIP-event timings after a warm-up, median of --regions regions of --iters calls, the variants alternated in one process on the
same rays.  Cases (those of profiles/ray_cast.md): 640 x 480 pinhole rays at the drill cache (0.01 m), nearest and trilinear,
gradient w.r.t. the shared eye and the directions; 160 x 120 rays at the C4 robot (W.build_c4) under A = 20 configurations,
gradient w.r.t. the eye, the directions and the transform stack.  Prints one JSON line per case and the markdown table of
profiles/ray_cast_backward.md (--out FILE writes the table there too).

With --parent-lib (the option repeats; another build of the library, a parent commit's say) it times instead the fused backward
of the C4 robot alone at the table's size and at A = 200 under 640 x 480 rays, nearest and trilinear -- torch.autograd.grad of the kept forward w.r.t. the eye, the directions and
the stack, and w.r.t. the first two only -- through this build and through every parent's entry points in alternating regions
(bench_min_over_points.against_parents), one JSON line per row with parent_bits_equal.

  python tools/bench_ray_cast_backward.py [--regions 9] [--iters 3] [--out FILE] [--parent-lib libpvamd.so]...
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
from pytorch_volumetric_amd.sdf import first_argmin  # noqa: E402
from bench_ray_cast import alternate, pinhole  # noqa: E402
from bench_min_over_points import against_parents, parent_library  # noqa: E402

T_MAX, TOL, MAX_STEPS = 3.0, 1e-3, 128
KW = dict(t_max=T_MAX, hit_tolerance=TOL, max_steps=MAX_STEPS)


def loss_upstream(res, dz, depth):
    """d loss / d t of sum over hits of (t d_z - depth)^2, in t's dtype."""
    hit = res.status == pv.RAY_HIT
    return torch.where(hit, 2 * (res.t * dz - depth) * dz, torch.zeros_like(res.t))


def restated(sdf, singles, eye, dirs, dz, depth, want_tf):
    """The contract in torch on the fused forward's outputs: (d eye, d directions, d stack or None)."""
    with torch.no_grad():
        res = sdf.ray_cast(eye, dirs, **KW)
        lead = dirs.shape[:-1]
        R = dirs.numel() // 3
        A = res.t.numel() // R
        up = loss_upstream(res, dz, depth).reshape(A, R).double()
        t, n = res.t.reshape(A, R).double(), res.gradients.reshape(A, R, 3).double()
        d, o = dirs.reshape(R, 3).double(), eye.double()
        c = n[..., 0] * d[:, 0] + n[..., 1] * d[:, 1] + n[..., 2] * d[:, 2]
        on = (res.status.reshape(A, R) == pv.RAY_HIT) & (c < 0) & torch.isfinite(c)
        w = torch.where(on, -up / torch.where(on, c, torch.ones_like(c)), torch.zeros_like(c))
        go = (w.unsqueeze(-1) * n).sum(0)
        gd = ((w * t).unsqueeze(-1) * n).sum(0)
        gtf = None
        if want_tf:
            comp = sdf.sdf
            S = len(comp.sdfs)
            stack = comp._tf_matrix.detach().reshape(S, A, 4, 4)
            x32 = eye + res.t.reshape(A, R, 1) * dirs.reshape(1, R, 3)
            vals = torch.stack([torch.stack([singles[s][a](x32[a])[0].reshape(R) for a in range(A)]) for s in range(S)], dim=-1)
            win = first_argmin(vals)  # (A, R)
            M = stack.double()[win, torch.arange(A, device=win.device).unsqueeze(-1)]
            x = o + t.unsqueeze(-1) * d
            gamma = (M[..., :3, :3] * n.unsqueeze(-2)).sum(-1)
            wg = w.unsqueeze(-1) * gamma
            term = torch.zeros((A, R, 4, 4), dtype=torch.float64, device=win.device)
            term[..., :3, :3] = wg.unsqueeze(-1) * x.unsqueeze(-2)
            term[..., :3, 3] = wg
            row = (win * A + torch.arange(A, device=win.device).unsqueeze(-1)).reshape(-1)
            gtf = torch.zeros((S * A, 4, 4), dtype=torch.float64, device=win.device).index_add_(0, row, term.reshape(-1, 4, 4)).float()
        return go.sum(0).float(), gd.reshape(*lead, 3).float(), gtf


def fused(sdf, eye, dirs, dz, depth, stack):
    e, dd = eye.detach().requires_grad_(), dirs.detach().requires_grad_()
    res = sdf.ray_cast(e, dd, differentiable=True, **KW)
    with torch.no_grad():  # the loss's own derivative is formed the same way in both variants
        up = loss_upstream(res, dz, depth)
    return torch.autograd.grad(res.t, (e, dd) + ((stack,) if stack is not None else ()), grad_outputs=up)


def against_parent_builds(robot, args):
    """The fused backward of the C4 robot alone (the forward kept), this build against every --parent-lib: the case of the table
    (A = 20, 160 x 120 rays), where the call is launch-bound, and A = 200 under 640 x 480 rays, where the kernel is the time."""
    parents = [parent_library(path) for path in args.parent_lib]
    for A, (w, h) in ((20, (160, 120)), (200, (640, 480))):
        robot.set_joint_configuration(W.c4_joint_configs(A, seed=0).cuda().requires_grad_())
        stack = robot.sdf._tf_matrix
        eye, dirs = pinhole(w, h, [1.2, 0.5, 0.8], [0.0, 0.0, 0.6], 70.0)
        for mode in ("nearest", "trilinear"):
            for leaf in robot.sdf.sdfs:
                leaf.interpolation = mode
            e, dd = eye.detach().requires_grad_(), dirs.detach().requires_grad_()
            res = robot.ray_cast(e, dd, differentiable=True, **KW)
            up = loss_upstream(res, dirs[..., 2], (res.t * dirs[..., 2] + 0.01).detach()).detach()
            for wrt in ((e, dd, stack), (e, dd)):  # without the stack: the kernel without the slab, for the session's spread
                row = {"case": f"C4 robot, {mode}", "configs": A, "rays": dirs.numel() // 3, "stack": len(wrt) == 3,
                       "hit_fraction": float((res.status == pv.RAY_HIT).float().mean())}
                row.update(against_parents(lambda: torch.autograd.grad(res.t, wrt, grad_outputs=up, retain_graph=True), parents,
                                           args.regions, args.iters))
                print(json.dumps(row), flush=True)
            del res, up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file (profiles/ray_cast_backward.md holds it with its notes)")
    ap.add_argument("--parent-lib", action="append", default=[], help="another build of libpvamd.so to time the backward against (repeats)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []

    def case(name, sdf, singles, eye, dirs, stack):
        R = dirs.numel() // 3
        with torch.no_grad():
            plain = sdf.ray_cast(eye, dirs, **KW)
        A = plain.t.numel() // R
        dz = dirs[..., 2]
        depth = (plain.t * dz + 0.01).detach()  # an observed depth 1 cm off: a non-zero upstream on every hit
        got = fused(sdf, eye, dirs, dz, depth, stack)
        want = restated(sdf, singles, eye, dirs, dz, depth, stack is not None)
        worst = max(float((g - w).abs().max() / w.abs().max().clamp_min(1e-30)) for g, w in zip(got, want))
        t = alternate({"forward": lambda: sdf.ray_cast(eye, dirs, **KW),
                       "restated": lambda: restated(sdf, singles, eye, dirs, dz, depth, stack is not None),
                       "fused": lambda: fused(sdf, eye, dirs, dz, depth, stack)}, args.regions, args.iters)
        rows.append({"case": name, "configs": A, "rays": R, "forward_only_ms": t["forward"], "restated_ms": t["restated"],
                     "fused_ms": t["fused"], "fused_over_restated": t["fused"] / t["restated"],
                     "hit_fraction": float((plain.status == pv.RAY_HIT).float().mean()), "max_rel_difference": worst})

    for mode in () if args.parent_lib else ("nearest", "trilinear"):
        c = W.build_c2_cache()
        c.interpolation = mode
        centre = [(r[0] + r[1]) / 2 for r in c.ranges]
        eye, dirs = pinhole(640, 480, [centre[0] + 0.55, centre[1] + 0.2, centre[2] + 0.12], centre, 50.0)
        case(f"drill cache 0.01 m, {mode}", c, None, eye, dirs, None)

    robot = W.build_c4()
    if args.parent_lib:
        return against_parent_builds(robot, args)
    A = 20
    q = W.c4_joint_configs(A, seed=0).cuda().requires_grad_()
    robot.set_joint_configuration(q)
    comp = robot.sdf
    S = len(comp.sdfs)
    stack = comp._tf_matrix
    rows_of = stack.detach().reshape(S, A, 4, 4)
    singles = []
    for s in range(S):
        per_config = []
        for a in range(A):
            one = pv.ComposedSDF([comp.sdfs[s]], None)
            one.set_transforms(rows_of[s, a:a + 1].contiguous(), known_rigid=True)
            per_config.append(one)
        singles.append(per_config)
    eye, dirs = pinhole(160, 120, [1.2, 0.5, 0.8], [0.0, 0.0, 0.6], 70.0)
    case("C4 robot, nearest", robot, singles, eye, dirs, stack)

    for row in rows:
        print(json.dumps(row))
    lines = ["| case | configurations x rays | forward only ms | forward + torch restatement ms | forward + fused backward ms | "
             "fused / restated | rays that hit | largest relative difference |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['configs']} x {r['rays']:,} | {r['forward_only_ms']:.4f} | {r['restated_ms']:.3f} | "
                     f"{r['fused_ms']:.4f} | {r['fused_over_restated']:.4f} | {100 * r['hit_fraction']:.1f} % | "
                     f"{r['max_rel_difference']:.1e} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
