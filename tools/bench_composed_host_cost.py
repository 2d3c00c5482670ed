"""Host time per eager ComposedSDF.__call__ on the C4 robot at the C4 shape (A = 200, P = 262,144: the chunk-grouped pair of
launches) and at the README point count (A = 200, P = 15,251: one per-lane launch, through the host-call module unless
PVAMD_NO_FASTCALL=1).  Timed: the call alone, from entry to return; the stream is drained after every call, outside the timed
span, so that no call waits for a full queue.  argv[1]: the tree whose package to import (this repository, or a checkout of
another commit built the same way), argv[2]: output JSON.  Run alternately on two trees, in fresh processes."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tree = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
sys.path.insert(0, tree)
import torch  # noqa: E402
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(pv.__file__))) == tree, pv.__file__


def host_us(fn, calls):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter_ns()
        fn()
        t1 = time.perf_counter_ns()
        torch.cuda.synchronize()
        out.append((t1 - t0) * 1e-3)
    out.sort()
    return {"p50": statistics.median(out), "p10": out[len(out) // 10], "p90": out[len(out) * 9 // 10]}


torch.cuda.set_device(0)
r = W.build_c4()
r.set_joint_configuration(W.c4_joint_configs(200, seed=0).cuda())
fast = pv._lib.fastcall() is not None
res = {"fastcall": fast}
with torch.no_grad():
    for P, calls in ((262144, 300), (15251, 3000)):
        pts = W.c4_points(P, seed=1)
        res[f"A=200 P={P} grouped={bool(r.sdf._grouping_pays(200, P, r.sdf._query_flags))}"] = host_us(lambda: r.sdf(pts), calls)
json.dump(res, open(sys.argv[2], "w"), indent=1)
print(json.dumps(res))
