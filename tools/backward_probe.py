"""Times the autograd backward kernels (csrc/backward.hip) with HIP events at C3 and C4 size, next to the forward with and without
the saved leaf ids, and (C4) torch autograd through the reference's op sequence (oracle.torch_opforop.ComposedOpForOp) on the
same GPU.  Prints one JSON object; `--out FILE` also writes it.

With --parent-lib (the option repeats; another build of the library, a parent commit's say) it times instead
pvamd_composed_query_backward / pvamd_composed_query_interp_backward alone at the same two sizes, nearest and trilinear, for a
value-only and a full upstream, with and without dtf, this build and every parent's in alternating regions on the same buffers
(bench_min_over_points.against_parents), and prints one JSON line per row with parent_bits_equal.

  python tools/backward_probe.py [--reps 20] [--out profiles/backward_probe.json]
  python tools/backward_probe.py --parent-lib A/libpvamd.so --parent-lib B/libpvamd.so [--regions 11] [--iters 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workloads as Wk  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402
from pytorch_volumetric_amd import autograd as ag  # noqa: E402
from bench_min_over_points import against_parents, parent_library  # noqa: E402


def timed(fn, reps):
    """median ms per call over `reps` calls, each between its own pair of HIP events (after 3 warm-up calls)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def measure(comp, pts, reps):
    lib = _lib.load()
    S = len(comp.sdfs)
    A = 1 if comp.tsf_batch is None else comp.tsf_batch[0]
    P = pts.shape[0]
    dev = pts.device
    grids = comp._leaf_grids(dev)
    tfd = comp._tf_device(dev)
    val = torch.empty((A, P), device=dev)
    grad = torch.empty((A, P, 3), device=dev)
    leaf = torch.empty((A, P), dtype=torch.int32, device=dev)
    flags = comp._direct_flags()

    def fwd(with_leaf):
        return lambda: _lib.check(lib.pvamd_composed_query(_lib.ptr(grids), S, _lib.ptr(tfd), A, _lib.ptr(pts), P, _lib.ptr(val),
                                                           _lib.ptr(grad), _lib.ptr(leaf if with_leaf else None), flags,
                                                           _lib.stream_ptr()), "pvamd_composed_query")

    out = {"S": S, "A": A, "P": P, "pairs": A * P}
    out["forward_ms"] = timed(fwd(False), reps)
    out["forward_out_leaf_ms"] = timed(fwd(True), reps)
    fwd(True)()
    dval = torch.randn((A, P), device=dev)
    dgrad = torch.randn((A, P, 3), device=dev)
    dpoints = torch.empty((P, 3), device=dev)
    dtf = torch.empty((S * A, 4, 4), device=dev)
    scratch = torch.empty((int(lib.pvamd_composed_backward_scratch_bytes(S, A, P, 0)),), dtype=torch.uint8, device=dev)

    def bwd(dg, dp):
        return lambda: _lib.check(lib.pvamd_composed_query_backward(_lib.ptr(grids), S, _lib.ptr(tfd), A, _lib.ptr(pts), P,
                                                                    _lib.ptr(leaf), _lib.ptr(dval), _lib.ptr(dg), _lib.ptr(dp),
                                                                    _lib.ptr(dtf), _lib.ptr(scratch), _lib.stream_ptr()),
                                  "pvamd_composed_query_backward")

    out["backward_val_only_dtf_ms"] = timed(bwd(None, None), reps)
    out["backward_full_ms"] = timed(bwd(dgrad, dpoints), reps)
    out["scratch_bytes"] = scratch.numel()
    # arithmetic floors at 8 TB/s (not measured): val-only reads dval + leaf id (8 B/pair); full reads 20 B/pair; out_leaf writes 4 B/pair
    pairs = A * P
    out["floor_val_only_ms"] = pairs * 8 / 8e12 * 1e3
    out["floor_full_ms"] = pairs * 20 / 8e12 * 1e3
    out["floor_out_leaf_extra_ms"] = pairs * 4 / 8e12 * 1e3
    out["fraction_of_floor_val_only"] = out["floor_val_only_ms"] / out["backward_val_only_dtf_ms"]
    out["fraction_of_floor_full"] = out["floor_full_ms"] / out["backward_full_ms"]
    return out


def rows_against_parents(case, comp, pts, mode, parents, regions, iters):
    """The composed backward of `comp` at `pts` alone (C ABI, the forward's leaf ids kept), this build against `parents`."""
    dev = pts.device
    with torch.no_grad():
        _, _, leaf, flat, tfd = comp._fused_forward(pts, mode, want_leaf=True)
    S, A, P = len(comp.sdfs), leaf.shape[0], flat.shape[0]
    grids = comp._leaf_grids(dev)
    entry = ag._BACKWARD[mode].format("composed")
    dval = torch.randn((A, P), device=dev)
    dgrad = torch.randn((A, P, 3), device=dev)
    dpoints = torch.empty((P, 3), device=dev)
    dtf = torch.empty((S * A, 4, 4), device=dev)
    scratch = ag._scratch(S, A, P, False, dev)
    for upstream, dg in (("val-only", None), ("full", dgrad)):
        for want_dtf in (True, False):
            def run(dg=dg, want_dtf=want_dtf):
                _lib.check(getattr(_lib.load(), entry)(_lib.ptr(grids), S, _lib.ptr(tfd), A, _lib.ptr(flat), P, _lib.ptr(leaf),
                                                       _lib.ptr(dval), _lib.ptr(dg), _lib.ptr(dpoints),
                                                       _lib.ptr(dtf if want_dtf else None), _lib.ptr(scratch), _lib.stream_ptr()), entry)
                return (dpoints, dtf) if want_dtf else (dpoints,)
            row = {"case": case, "mode": mode, "S": S, "A": A, "P": P, "upstream": upstream, "dtf": want_dtf}
            row.update(against_parents(run, parents, regions, iters))
            print(json.dumps(row), flush=True)


def main_against_parents(args):
    parents = [parent_library(path) for path in args.parent_lib]
    for mode in ("nearest", "trilinear"):
        cached = Wk.build_c2_cache()
        cached.interpolation = mode
        rows_against_parents("C3", Wk.build_c3(cached), Wk.c3_points(1 << 22, seed=0), mode, parents, args.regions, args.iters)
        robot = Wk.build_c4()
        for leaf in robot.sdf.sdfs:
            leaf.interpolation = mode
        robot.set_joint_configuration(Wk.c4_joint_configs(200).cuda())
        rows_against_parents("C4", robot.sdf, Wk.c4_points(262144), mode, parents, args.regions, args.iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", action="append", default=[], help="another build of libpvamd.so to time side by side (repeats)")
    ap.add_argument("--regions", type=int, default=11, help="with --parent-lib: alternating regions per library")
    ap.add_argument("--iters", type=int, default=3, help="with --parent-lib: calls per region")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-autograd restatement at C4 size")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.parent_lib:
        return main_against_parents(args)
    res = {}
    cached = Wk.build_c2_cache()
    c3 = Wk.build_c3(cached)
    res["C3"] = measure(c3, Wk.c3_points(1 << 22, seed=0), args.reps)
    robot = Wk.build_c4()
    q = Wk.c4_joint_configs(200).cuda()
    robot.set_joint_configuration(q)
    pts = Wk.c4_points(262144)
    res["C4"] = measure(robot.sdf, pts, args.reps)
    # the HIP path end to end through autograd (set_joint_configuration + query + val-only loss backward to q)
    def hip_autograd():
        qg = q.clone().requires_grad_()
        robot.set_joint_configuration(qg)
        v, _ = robot(pts)
        ((0.05 - v).clamp(min=0) ** 2).sum().backward()
    res["C4"]["autograd_end_to_end_ms"] = timed(hip_autograd, max(3, args.reps // 4))
    robot.set_joint_configuration(q)
    if not args.no_torch:
        from oracle.torch_opforop import CachedOpForOp, ComposedOpForOp
        leaves = []
        for c in robot.sdf.sdfs:
            pk = c._packed
            leaves.append(CachedOpForOp(pk[:, 0].reshape(c._view.shape).contiguous(), pk[:, 1:4].contiguous(),
                                        c._view.min.cuda(), c._view.max.cuda(), c.bb))

        def torch_autograd():
            qg = q.clone().requires_grad_()
            stack = robot._stack_torch(qg)
            v, _ = ComposedOpForOp(leaves, stack, batch=200)(pts)
            ((0.05 - v).clamp(min=0) ** 2).sum().backward()
        res["C4"]["torch_opforop_autograd_ms"] = timed(torch_autograd, 3)
        res["C4"]["hip_speedup_vs_torch_autograd"] = res["C4"]["torch_opforop_autograd_ms"] / res["C4"]["autograd_end_to_end_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
