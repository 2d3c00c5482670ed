"""CPU: the C-ABI library loads and exports exactly what include/pvamd.h declares (no compute calls)."""
import ctypes
import os
import re
import subprocess

import pytest

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvamd.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pvamd_[a-z0-9_]+)\s*\(", text)))


def test_library_is_built_in_tree_and_loads():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = _lib.load()
    assert lib.pvamd_abi_version() == _lib.ABI_VERSION
    assert b"gfx950" in lib.pvamd_build_info()


def test_every_declared_symbol_is_exported_and_bound():
    names = declared_functions()
    assert len(names) >= 12
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/pvamd.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes binding and header disagree"


def test_no_library_kernels_inside_the_shared_object():
    """the spatial sort called rocprim::radix_sort_pairs from 1.5 M points on; the hot path is hand-written
    throughout now -- no rocPRIM / hipCUB / Thrust instantiation is linked into libpvamd.so."""
    out = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for lib_name in ("rocprim", "hipcub", "thrust", "rocblas", "hipblas"):
        assert lib_name not in out.lower(), f"{lib_name} symbols in libpvamd.so"
    src = open(os.path.join(ROOT, "pytorch_volumetric_amd", "csrc", "sort.hip")).read()
    assert "#include <rocprim" not in src


def test_struct_layouts_match_the_header(tmp_path):
    """Compile a tiny C program against the header and compare sizeof/offsetof with the ctypes mirrors."""
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "pvamd.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(pvamd_grid_t), offsetof(pvamd_grid_t, dres), offsetof(pvamd_grid_t, fmin),
             offsetof(pvamd_grid_t, bb_min), offsetof(pvamd_grid_t, shape), offsetof(pvamd_grid_t, index_f64),
             offsetof(pvamd_grid_t, oob_mode));
      printf("%zu %zu %zu\n", sizeof(pvamd_mesh_t), offsetof(pvamd_mesh_t, F), offsetof(pvamd_mesh_t, ray_dir));
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pvamd_mesh_plan_t), offsetof(pvamd_mesh_plan_t, path),
             offsetof(pvamd_mesh_plan_t, order), offsetof(pvamd_mesh_plan_t, groups), offsetof(pvamd_mesh_plan_t, slots),
             offsetof(pvamd_mesh_plan_t, scan_waves), offsetof(pvamd_mesh_plan_t, parts), offsetof(pvamd_mesh_plan_t, part_waves));
      printf("%d %d %d %d  %d %d %d  %d %d %d\n", PVAMD_MESH_PATH_NONE, PVAMD_MESH_PATH_LISTED, PVAMD_MESH_PATH_SCAN,
             PVAMD_MESH_PATH_SCAN_HEAVY, PVAMD_MESH_ORDER_GIVEN, PVAMD_MESH_ORDER_INSIDE, PVAMD_MESH_ORDER_SORT_CALL,
             PVAMD_ORDER_KERNEL_SMALL, PVAMD_ORDER_KERNEL_COUNTING, PVAMD_ORDER_KERNEL_RADIX);
      return 0; }'''
    exe = str(tmp_path / "pvamd_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    out = subprocess.run([exe], capture_output=True, check=True).stdout.decode().split()
    G, M = _lib.GridDesc, _lib.MeshDesc
    assert [int(x) for x in out[:7]] == [ctypes.sizeof(G), G.dres.offset, G.fmin.offset, G.bb_min.offset, G.shape.offset,
                                         G.index_f64.offset, G.oob_mode.offset]
    assert [int(x) for x in out[7:10]] == [ctypes.sizeof(M), M.F.offset, M.ray_dir.offset]
    Pl = _lib.MeshPlan
    assert [int(x) for x in out[10:18]] == [ctypes.sizeof(Pl)] + [getattr(Pl, name).offset for name, _ in Pl._fields_]
    assert [name for name, _ in Pl._fields_] == ["path", "order", "groups", "slots", "scan_waves", "parts", "part_waves"]
    assert [int(x) for x in out[18:]] == [_lib.MESH_PATH_NONE, _lib.MESH_PATH_LISTED, _lib.MESH_PATH_SCAN, _lib.MESH_PATH_SCAN_HEAVY,
                                          _lib.MESH_ORDER_GIVEN, _lib.MESH_ORDER_INSIDE, _lib.MESH_ORDER_SORT_CALL,
                                          _lib.ORDER_KERNEL_SMALL, _lib.ORDER_KERNEL_COUNTING, _lib.ORDER_KERNEL_RADIX]


def test_oracle_grid_layout_is_one_definition(tmp_path):
    """The checker's grid description lives in oracle/pvamd_oracle.h; the plain-C host test (tests/cabi/cabi_check.c) includes
    it and the ctypes mirror in oracle/oracle.py must agree with it (an outdated private copy in the C test once made the
    oracle read every grid after the first at the wrong stride)."""
    from oracle import oracle as orc
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "pvamd_oracle.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu\n", sizeof(oracle_grid_t), offsetof(oracle_grid_t, dres), offsetof(oracle_grid_t, fres),
             offsetof(oracle_grid_t, shape), offsetof(oracle_grid_t, rule), offsetof(oracle_grid_t, dbb_max));
      return 0; }'''
    exe = str(tmp_path / "pvamd_oracle_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "oracle"), "-o", exe], input=src.encode(), check=True)
    out = [int(x) for x in subprocess.run([exe], capture_output=True, check=True).stdout.decode().split()]
    G = orc.OracleGrid
    assert out == [ctypes.sizeof(G), G.dres.offset, G.fres.offset, G.shape.offset, G.rule.offset, G.dbb_max.offset]
    assert "pvamd_oracle.h" in open(os.path.join(ROOT, "tests", "cabi", "cabi_check.c")).read()


def test_buffer_size_macros_match_the_exported_functions(tmp_path):
    """The buffer-size macros the header keeps (records in whole tiles, tile / group spheres, the scratch of the mesh entry
    points, the scratch of the minimum's backward) are what the exported functions of the library return."""
    src = r'''
    #include <stdio.h>
    #include "pvamd.h"
    int main(void) {
      long long v[] = {0, 1, 255, 256, 257, 15728, 99500, 1 << 20, 1 << 21, (1 << 24) + 5, 67108877};
      for (int i = 0; i < 11; ++i)
        printf("%lld %lld %lld\n", (long long)PVAMD_REC_FLOATS(v[i]), (long long)PVAMD_TILES_FLOATS(v[i]),
               (long long)PVAMD_MESH_SCRATCH_BYTES(v[i]));
      printf("%d\n", PVAMD_MESH_SMALL_POINTS);
      printf("%lld %lld %lld %lld\n", (long long)PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(1, 1, 0),
             (long long)PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(1, 1, 1), (long long)PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(8, 200, 0),
             (long long)PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(8, 200, 1));
      return 0; }'''
    exe = str(tmp_path / "pvamd_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()]
    lib = _lib.load()
    assert len(out) == 13
    for n, row in zip((0, 1, 255, 256, 257, 15728, 99500, 1 << 20, 1 << 21, (1 << 24) + 5, 67108877), out):
        assert row == [lib.pvamd_mesh_rec_floats(n), lib.pvamd_mesh_tiles_floats(n), lib.pvamd_mesh_scratch_bytes(n)], (n, row)
    assert out[-2] == [lib.pvamd_mesh_small_points()] == [16384]
    assert out[-1] == [lib.pvamd_min_over_points_backward_scratch_bytes(S, A, per_leaf)
                       for S, A in ((1, 1), (8, 200)) for per_leaf in (0, 1)]
    assert out[-1] == [24, 24, 24 * 200, 24 * 200 * 8]


def test_morton_order_scratch_size_steps_up_and_stays_under_the_old_bound():
    """pvamd_morton_order_scratch_bytes is the larger of the two sorts' layouts: across each branch point (one launch / 2^15 /
    2^18 cells, counting / radix sort, 196 -> 197 tiles where the supergroups round, 2^21 cells) it does not shrink, and it
    never exceeds what the header's macro asked for before the function existed (<= 512 words per radix tile)."""
    lib = _lib.load()
    sizes = []
    for P in (1, 16384, 16385, 65535, 65536, 786431, 786432, 806912, 1048575, 1048576, (1 << 24) + 5):
        bits = 21 if P >= (1 << 20) else (18 if P >= (1 << 16) else 15)
        old = 4 * max(8 + 4 * P + 512 * ((P + 4095) // 4096), 8 + (1 << bits) + P + 2048)
        sizes.append(lib.pvamd_morton_order_scratch_bytes(P))
        assert 0 < sizes[-1] <= old, (P, sizes[-1], old)
    assert sizes == sorted(sizes), sizes


SIZE_FUNCTIONS = ("min_over_points_scratch_bytes", "hinge_over_points_scratch_bytes", "hinge_over_points_backward_scratch_bytes",
                  "leaf_pair_scratch_bytes", "leaf_pair_hinge_scratch_bytes", "chamfer_normal_eq_scratch_bytes",
                  "min_over_points_backward_scratch_bytes", "mesh_scratch_bytes", "morton_order_scratch_bytes")
MESH_SIZE_FUNCTIONS = ("rec_floats", "tiles_floats")  # _lib.NAME asks pvamd_mesh_NAME


def test_scratch_size_macros_match_the_exported_functions(tmp_path):
    """The exported pvamd_*_scratch_bytes functions are the definition of every scratch size; the header keeps a macro only for
    the one-expression sizes the library itself returns.  Each of those against its function, at the branch points of the
    formulas: one point, a full chunk, one point more, many chunks; both element sizes; per_leaf / backward on and off."""
    src = r'''
    #include <stdio.h>
    #include "pvamd.h"
    int main(void) {
      long long P[] = {1, 4096, 4097, 262145}, SA[][2] = {{1, 1}, {8, 200}}, KA[][2] = {{1, 1}, {42, 200}};
      long long N[] = {1, 2048, 2049}, B[] = {1, 1024};
      for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) for (int pl = 0; pl < 2; ++pl)
        printf("mop %lld %lld %lld %d %lld %lld\n", SA[j][0], SA[j][1], P[i], pl,
               (long long)PVAMD_MIN_OVER_POINTS_SCRATCH_BYTES(SA[j][0], SA[j][1], P[i], pl),
               (long long)PVAMD_HINGE_OVER_POINTS_SCRATCH_BYTES(SA[j][0], SA[j][1], P[i], pl));
      for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) for (int f64 = 0; f64 < 2; ++f64) for (int bwd = 0; bwd < 2; ++bwd)
        printf("lp %lld %lld %lld %d %d %lld\n", KA[j][0], KA[j][1], P[i], f64, bwd,
               (long long)PVAMD_LEAF_PAIR_SCRATCH_BYTES(KA[j][0], KA[j][1], P[i], f64 ? 8 : 4, bwd));
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 2; ++j)
        printf("reg %lld %lld %lld\n", B[j], N[i], (long long)PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES(B[j], N[i]));
      printf("const %d %d %d\n", PVAMD_MOP_CHUNK, PVAMD_REG_CHUNK, PVAMD_REG_SUMS);
      return 0; }'''
    exe = str(tmp_path / "pvamd_scratch_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    lines = [line.split() for line in subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()]
    lib = _lib.load()
    seen = {"mop": 0, "lp": 0, "reg": 0, "const": 0}
    for kind, *rest in lines:
        v = [int(x) for x in rest]
        seen[kind] += 1
        if kind == "mop":
            S, A, P, pl, mop, hop = v
            assert lib.pvamd_min_over_points_scratch_bytes(S, A, P, pl) == mop, v
            assert lib.pvamd_hinge_over_points_scratch_bytes(S, A, P, pl) == hop, v
        elif kind == "lp":
            K, A, P, f64, bwd, n = v
            assert lib.pvamd_leaf_pair_scratch_bytes(K, A, P, f64, bwd) == n, v
            if not bwd:  # the hinge's forward is the distance's; its backward has no macro (a launch plan decides it)
                assert lib.pvamd_leaf_pair_hinge_scratch_bytes(K, A, P, f64, 0) == n, v
        elif kind == "reg":
            B, N, n = v
            assert lib.pvamd_chamfer_normal_eq_scratch_bytes(B, N) == n, v
        else:
            assert v == [_lib.MOP_CHUNK, _lib.REG_CHUNK, _lib.REG_SUMS] == [4096, 2048, 28]
    assert seen == {"mop": 16, "lp": 32, "reg": 6, "const": 1}
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(re.findall(r"#define\s+(PVAMD_\w*SCRATCH_BYTES)\b", text)) == sorted(
        ["PVAMD_MIN_OVER_POINTS_SCRATCH_BYTES", "PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES",
         "PVAMD_HINGE_OVER_POINTS_SCRATCH_BYTES", "PVAMD_LEAF_PAIR_SCRATCH_BYTES", "PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES",
         "PVAMD_MESH_SCRATCH_BYTES"]), "a size macro without a check against its definition"


def test_binding_asks_the_library_for_scratch_sizes():
    """_lib's size functions are one call of the exported function of the same name (bool arguments converted), with no
    arithmetic of their own to drift from it."""
    import inspect
    lib = _lib.load()
    for S, A, P in ((8, 200, 262145), (1, 1, 1), (3, 64, 33792)):
        for pl in (False, True):
            assert _lib.min_over_points_scratch_bytes(S, A, P, pl) == lib.pvamd_min_over_points_scratch_bytes(S, A, P, int(pl))
            assert _lib.hinge_over_points_scratch_bytes(S, A, P, pl) == lib.pvamd_hinge_over_points_scratch_bytes(S, A, P, int(pl))
            for f64 in (False, True):
                assert _lib.hinge_over_points_backward_scratch_bytes(S, A, P, pl, f64) == \
                    lib.pvamd_hinge_over_points_backward_scratch_bytes(S, A, P, int(pl), int(f64))
                # (K, A, max_points, f64, backward)
                assert _lib.leaf_pair_scratch_bytes(S, A, P, f64, pl) == lib.pvamd_leaf_pair_scratch_bytes(S, A, P, int(f64), int(pl))
                assert _lib.leaf_pair_hinge_scratch_bytes(S, A, P, f64, pl) == \
                    lib.pvamd_leaf_pair_hinge_scratch_bytes(S, A, P, int(f64), int(pl))
            assert _lib.min_over_points_backward_scratch_bytes(S, A, pl) == lib.pvamd_min_over_points_backward_scratch_bytes(S, A, int(pl))
        assert _lib.chamfer_normal_eq_scratch_bytes(A, P) == lib.pvamd_chamfer_normal_eq_scratch_bytes(A, P)
        for n in (P, A * 64 * 8192, 0):
            assert _lib.mesh_scratch_bytes(n) == lib.pvamd_mesh_scratch_bytes(n) > 0
            assert _lib.morton_order_scratch_bytes(n) == lib.pvamd_morton_order_scratch_bytes(n) > 0
            assert _lib.rec_floats(n) == lib.pvamd_mesh_rec_floats(n)
            assert _lib.tiles_floats(n) == lib.pvamd_mesh_tiles_floats(n)
    assert _lib.mesh_small_points() == lib.pvamd_mesh_small_points()
    for name in SIZE_FUNCTIONS + MESH_SIZE_FUNCTIONS:
        source = inspect.getsource(getattr(_lib, name))
        assert f"load().pvamd_{'mesh_' if name in MESH_SIZE_FUNCTIONS else ''}{name}(" in source, name
        for operator in ("//", "*", "+"):
            assert operator not in source, (name, operator)


def test_no_gpu_means_a_loud_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.PvamdError):
        _lib.require_gpu()
    obj = pv.MeshObjectFactory(mesh=pv.mesh_io.box_mesh()) if hasattr(pv, "mesh_io") else None
    from pytorch_volumetric_amd import mesh_io
    obj = pv.MeshObjectFactory(mesh=mesh_io.box_mesh())
    with pytest.raises(_lib.PvamdError):
        pv.MeshSDF(obj)(torch.zeros(4, 3))


def test_product_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under pytorch_volumetric_amd/ may import, load or link it."""
    pkg = os.path.join(ROOT, "pytorch_volumetric_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "libpvamd_oracle" not in text, f
                if f.endswith((".hip", ".h")) and f != "xform.hip":
                    assert '#include "../../oracle' not in text and "oracle/" not in text.replace("oracle/pvamd_oracle.c", ""), f
    deps = subprocess.run(["ldd", _lib.LIB_PATH], capture_output=True).stdout.decode()
    assert "oracle" not in deps


def test_no_wrong_result_experiments_in_the_product_sources_and_variants_are_refused():
    """timing experiments that return WRONG results are patches under tools/patches now, not #ifdefs in
    csrc/; an A/B build (tools/build_variant.sh) names itself through `pvamd_variant` and _lib.load() refuses it unless
    PVAMD_ALLOW_VARIANT=1.  The product library exports no such symbol.
    Nor do the sources keep build knobs, alternate paths or instrumentation behind PVAMD_ macros ("prune the
    laboratory out of the product"): every kernel has one configuration, and the only preprocessor conditionals on a PVAMD_
    macro are the include-order guards and the variant's name."""
    import glob
    import re
    csrc = os.path.join(ROOT, "pytorch_volumetric_amd", "csrc")
    conditionals = set()
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        text = open(path).read()
        for word in ("ABLATE", "ONLY_SEED", "WRONG results"):
            assert word not in text, f"{word} in {os.path.basename(path)}"
        for line in text.splitlines():
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                conditionals |= {(os.path.basename(path), macro) for macro in re.findall(r"\bPVAMD_\w+", line)}
    assert conditionals == {("wave_ops.h", "PVAMD_DEV"), ("exact_math.h", "PVAMD_DEV"), ("mesh_math.h", "PVAMD_DEV"),
                            ("common.h", "PVAMD_VARIANT")}, sorted(conditionals)
    out = subprocess.run(["nm", "-D", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pvamd_variant" not in out and "pvamd_debug" not in out
    assert "pvamd_variant" in open(os.path.join(csrc, "common.h")).read()
    assert "PVAMD_ALLOW_VARIANT" in open(os.path.join(ROOT, "pytorch_volumetric_amd", "_lib.py")).read()
