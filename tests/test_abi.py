"""CPU: the C-ABI library loads and exports exactly what include/pvamd.h declares (no compute calls)."""
import ctypes
import os
import re
import subprocess

import pytest

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _header, _lib

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


STRUCT_MIRRORS = {"pvamd_grid_t": _lib.GridDesc, "pvamd_mesh_t": _lib.MeshDesc, "pvamd_mesh_plan_t": _lib.MeshPlan,
                  "pvamd_joint_t": _lib.JointDesc}


def test_struct_layouts_match_the_header(tmp_path):
    """Compile a tiny C program against the header and compare sizeof, and offsetof and size of every field, with the four
    ctypes mirrors.  The program is generated from the mirrors' _fields_: a field the header does not have fails to compile, one
    the mirror lacks moves a later offset or the size."""
    prints = []
    for ctype, mirror in STRUCT_MIRRORS.items():
        prints.append(f'printf("%zu", sizeof({ctype}));')
        prints += [f'printf(" %zu %zu", offsetof({ctype}, {name}), sizeof((({ctype}*)0)->{name}));' for name, _ in mirror._fields_]
        prints.append(r'printf("\n");')
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "pvamd.h"
    int main(void) {
      STRUCTS
      printf("%d %d %d %d  %d %d %d  %d %d %d\n", PVAMD_MESH_PATH_NONE, PVAMD_MESH_PATH_LISTED, PVAMD_MESH_PATH_SCAN,
             PVAMD_MESH_PATH_SCAN_HEAVY, PVAMD_MESH_ORDER_GIVEN, PVAMD_MESH_ORDER_INSIDE, PVAMD_MESH_ORDER_SORT_CALL,
             PVAMD_ORDER_KERNEL_SMALL, PVAMD_ORDER_KERNEL_COUNTING, PVAMD_ORDER_KERNEL_RADIX);
      return 0; }'''.replace("STRUCTS", "\n      ".join(prints))
    exe = str(tmp_path / "pvamd_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()]
    assert len(out) == len(STRUCT_MIRRORS) + 1
    for (ctype, mirror), row in zip(STRUCT_MIRRORS.items(), out):
        want = [ctypes.sizeof(mirror)]
        for name, _ in mirror._fields_:
            want += [getattr(mirror, name).offset, getattr(mirror, name).size]
        assert row == want, ctype
    assert [len(mirror._fields_) for mirror in STRUCT_MIRRORS.values()] == [22, 8, 7, 7]
    Pl = _lib.MeshPlan
    assert [name for name, _ in Pl._fields_] == ["path", "order", "groups", "slots", "scan_waves", "parts", "part_waves"]
    assert out[-1] == [_lib.MESH_PATH_NONE, _lib.MESH_PATH_LISTED, _lib.MESH_PATH_SCAN, _lib.MESH_PATH_SCAN_HEAVY,
                       _lib.MESH_ORDER_GIVEN, _lib.MESH_ORDER_INSIDE, _lib.MESH_ORDER_SORT_CALL,
                       _lib.ORDER_KERNEL_SMALL, _lib.ORDER_KERNEL_COUNTING, _lib.ORDER_KERNEL_RADIX]


HOST_MIRRORS = {"GridDesc": _lib.GridDesc, "MeshDesc": _lib.MeshDesc, "MeshPlan": _lib.MeshPlan}
SYNTHETIC_HEADER = r"""
/* a comment that mentions pvamd_not_declared( and
 * #define PVAMD_IN_COMMENT 5 */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PVAMD_PLAIN 16
#define PVAMD_ZERO 0   /* a trailing comment */
#define PVAMD_PAREN (7)
#define PVAMD_NEG_PAREN (-3)  /* a comment that
                                 runs over two lines */
#define PVAMD_NEG_BARE -4
  #  define PVAMD_INDENTED 9
#define PVAMD_FUNCTION_LIKE(F) ((F) + 1)
#define PVAMD_EXPRESSION (3 << 18)
#define PVAMD_REAL 1.5
#define PVAMD_HEX 0x10
#define PVAMD_TEXT "16"
#define PVAMD_HALF_OPEN (8
#define PVAMD_EMPTY
#define PVAMD_CONTINUED(a, b) \
    ((a) + \
     pvamd_in_a_macro(b))
typedef struct pvamd_grid { const float* vox; int32_t shape[3]; } pvamd_grid_t;
int pvamd_no_arguments(void);
const char* pvamd_text(void);
int64_t pvamd_scalars(int a, int32_t b, int64_t c, uint64_t d, uint8_t e, float f, double g);
int pvamd_over_lines(const float* points, void *stream,
                     int64_t * out_index,   /* a comment between parameters */
                     uint8_t*out_flags);
int pvamd_host_structs(const pvamd_grid_t* grid, pvamd_mesh_t* mesh, pvamd_mesh_plan_t* plan_out);
int pvamd_device_arrays(const pvamd_grid_t* grids, const pvamd_mesh_t* meshes, pvamd_mesh_plan_t* plan, const pvamd_joint_t* joints,
                        const float* grid);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_reader_maps_each_rule_on_a_synthetic_header():
    """_header.parse on a header written for it: one declaration per rule, and the #defines it keeps and ignores."""
    c = ctypes
    declarations, defines = _header.parse(SYNTHETIC_HEADER, HOST_MIRRORS)
    assert list(declarations.items()) == [
        ("pvamd_no_arguments", (c.c_int, [])),
        ("pvamd_text", (c.c_char_p, [])),
        ("pvamd_scalars", (c.c_int64, [c.c_int, c.c_int32, c.c_int64, c.c_uint64, c.c_uint8, c.c_float, c.c_double])),
        ("pvamd_over_lines", (c.c_int, [c.c_void_p] * 4)),
        ("pvamd_host_structs", (c.c_int, [c.POINTER(_lib.GridDesc), c.POINTER(_lib.MeshDesc), c.POINTER(_lib.MeshPlan)])),
        # the same types under other names, and another type under a host struct's name: raw addresses
        ("pvamd_device_arrays", (c.c_int, [c.c_void_p] * 5)),
    ]
    assert defines == {"PVAMD_PLAIN": 16, "PVAMD_ZERO": 0, "PVAMD_PAREN": 7, "PVAMD_NEG_PAREN": -3, "PVAMD_NEG_BARE": -4,
                       "PVAMD_INDENTED": 9}
    assert sorted(_header.HOST_STRUCTS) == [("pvamd_grid_t", "grid"), ("pvamd_mesh_plan_t", "plan_out"), ("pvamd_mesh_t", "mesh")]


@pytest.mark.parametrize("line", [
    "int pvamd_refused(foo_t a);",                          # an unknown scalar type
    "int pvamd_refused(unsigned int a);",
    "void pvamd_refused(int a);",                           # an unknown return type
    "const float* pvamd_refused(int a);",
    "int pvamd_refused(const float*, int64_t P);",          # a parameter without a name
    "int pvamd_refused(const float* points, int64_t);",
    "int pvamd_refused();",
    "int pvamd_refused(float** rows);",
    "int pvamd_refused(float rows[3]);",
    "int pvamd_refused(int (*callback)(int), void* stream);",  # a function-pointer parameter
    "int pvamd_refused(int a)",                             # no semicolon: runs into the next declaration
    "static inline int pvamd_refused(int a) { return a; }",
    "int (*pvamd_refused)(int a);",
    "typedef int pvamd_refused(int a);",
    "int pvamd_no_arguments(int a);",                       # a second declaration of a name
    "typedef struct { int (*member)(int); int pvamd_refused(int); } odd_t;",
])
def test_header_reader_refuses_what_it_cannot_map(line):
    """No declaration is ever skipped: whatever is not `type pvamd_name(parameters);` under the rules raises, naming it."""
    name = "pvamd_no_arguments" if "pvamd_no_arguments" in line else "pvamd_refused"
    text = SYNTHETIC_HEADER.replace("int pvamd_no_arguments(void);", line + "\nint pvamd_no_arguments(void);")
    assert text != SYNTHETIC_HEADER
    with pytest.raises(ValueError, match=name):
        _header.parse(text, HOST_MIRRORS)


def test_missing_header_is_a_loud_error_without_a_fallback_table(tmp_path, monkeypatch):
    """The binding executed with no header to read raises PvamdError naming the path it expected."""
    import importlib.util
    assert os.path.samefile(_header.HEADER_PATH, HEADER)
    missing = str(tmp_path / "include" / "pvamd.h")
    monkeypatch.setattr(_header, "HEADER_PATH", missing)
    with pytest.raises(OSError):
        _header.read(HOST_MIRRORS)
    spec = importlib.util.spec_from_file_location("pvamd_lib_without_header", _lib.__file__)  # a second copy: _lib itself stays
    with pytest.raises(RuntimeError, match=re.escape(missing)) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "PvamdError"


def test_binding_is_the_header_read_with_pins_on_what_must_not_move():
    """_lib.SIGNATURES is what the reader makes of include/pvamd.h; the entries whose types a caller's arguments depend on are
    pinned literally, so that a change of the rules cannot move them unnoticed."""
    c = ctypes
    declarations, defines = _header.read(HOST_MIRRORS)
    assert _lib.SIGNATURES == declarations and _lib.H == defines and len(declarations) >= 102
    S = _lib.SIGNATURES
    assert S["pvamd_cached_query"] == (c.c_int, [c.POINTER(_lib.GridDesc), c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
                                                 c.c_void_p])
    assert S["pvamd_composed_query"][1][0] is c.c_void_p and len(S["pvamd_composed_query"][1]) == 11
    assert S["pvamd_grid_finalize"] == (c.c_int, [c.POINTER(_lib.GridDesc)])
    assert S["pvamd_mesh_query"][1][0] == c.POINTER(_lib.MeshDesc)
    assert S["pvamd_mesh_query_plan"][1] == [c.c_int64, c.c_int32, c.c_int32, c.c_int32, c.POINTER(_lib.MeshPlan)]
    assert S["pvamd_chamfer_mesh_plan"][1][-1] == c.POINTER(_lib.MeshPlan)
    assert S["pvamd_chain_fk"][1][0] is c.c_void_p and S["pvamd_configure_chain"][1][0] is c.c_void_p  # joints: a device array
    at = S["pvamd_leaf_pair_hinge"][1].index(c.c_float)
    assert at == 10 and S["pvamd_leaf_pair_hinge_f64"][1][at] is c.c_double
    assert c.c_double not in S["pvamd_leaf_pair_hinge"][1] and c.c_float not in S["pvamd_leaf_pair_hinge_f64"][1]
    for name in ("pvamd_leaf_pair_hinge_backward", "pvamd_composed_hinge_over_points", "pvamd_composed_hinge_over_points_backward"):
        margin = [i for i, t in enumerate(S[name][1]) if t is c.c_float]
        assert len(margin) == 1 and [i for i, t in enumerate(S[name + "_f64"][1]) if t is c.c_double] == margin, name
    assert S["pvamd_build_info"] == (c.c_char_p, [])
    sizes = [name for name in S if name.endswith("_scratch_bytes")]
    assert len(sizes) >= 12 and all(S[name][0] is c.c_int64 for name in sizes), sizes
    assert all(restype in (c.c_int, c.c_int64, c.c_char_p) for restype, _ in S.values())


def test_binding_copies_no_value_the_header_defines():
    """The source of _lib.py assigns no integer literal to a name the header defines as PVAMD_<name> (nor inside LEAF_MODES and
    the keys of _ERRORS): each is looked up in the header that was read, so the value cannot drift from it."""
    import ast
    import inspect
    mirrored = {}
    for node in ast.parse(inspect.getsource(_lib)).body:
        if not isinstance(node, ast.Assign):
            continue
        names = [n.id for target in node.targets for n in ast.walk(target) if isinstance(n, ast.Name)]
        literals = [k.value for k in ast.walk(node.value) if isinstance(k, ast.Constant) and type(k.value) is int]
        for name in names:
            if "PVAMD_" + name in _lib.H or name in ("LEAF_MODES", "_ERRORS"):
                assert not literals, (name, literals)
                mirrored[name] = getattr(_lib, name)
    assert len(mirrored) >= 37, sorted(mirrored)
    for name, value in mirrored.items():
        if name not in ("LEAF_MODES", "_ERRORS"):
            assert value == _lib.H["PVAMD_" + name], name
    assert mirrored["LEAF_MODES"] == {"nearest": _lib.H["PVAMD_LEAF_NEAREST"], "trilinear": _lib.H["PVAMD_LEAF_TRILINEAR"]}
    assert sorted(mirrored["_ERRORS"]) == sorted(v for k, v in _lib.H.items() if k.startswith("PVAMD_E_"))
    assert _lib.ABI_VERSION == _lib.H["PVAMD_ABI_VERSION"] == 16 and _lib.E_SHAPE == -2 and _lib.RAY_HIT == 1


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
