"""CPU: the checked call path of the binding (_lib.call) -- what the reader keeps of every parameter, every call site in the
package against the header without a GPU, the sites that still call an entry point directly, and the refusals."""
import ast
import ctypes
import os

import pytest
import torch

from pytorch_volumetric_amd import _header, _lib

PACKAGE = os.path.dirname(os.path.abspath(_lib.__file__))
MIRRORS = {"GridDesc": _lib.GridDesc, "MeshDesc": _lib.MeshDesc, "MeshPlan": _lib.MeshPlan}


# ---------------------------------------------------------------- 1. the reader
def test_reader_keeps_name_type_pointer_and_const_of_every_parameter():
    P = _lib.PARAMETERS
    assert list(P) == list(_lib.SIGNATURES) and all(len(P[n]) == len(_lib.SIGNATURES[n][1]) for n in P)
    assert P["pvamd_cached_query"] == [
        ("grid", "pvamd_grid_t", True, True), ("points", "float", True, True), ("P", "int64_t", False, False),
        ("out_val", "float", True, False), ("out_grad", "float", True, False), ("out_oob", "uint8_t", True, False),
        ("stream", "void", True, False)]
    mop = {name: rest for name, *rest in P["pvamd_composed_min_over_points_f64"]}
    assert mop["out_index"] == ["int64_t", True, False] and mop["out_leaf"] == ["int32_t", True, False]
    assert mop["points"] == ["double", True, True] and mop["out_val"] == ["double", True, False]
    # what _plan's kinds rest on: a pointer parameter is a typed data pointer, void* or a struct, and a stream comes last
    pointers = [(n, p) for n in P for p in P[n] if p[2]]
    assert all(P[n][-1] == p for n, p in pointers if p[0] == "stream") and any(p[0] == "stream" for _, p in pointers)
    assert {p[1] for _, p in pointers} - set(_lib._ELEMENTS) == {"void", "pvamd_grid_t", "pvamd_mesh_t", "pvamd_mesh_plan_t",
                                                               "pvamd_joint_t"}


def test_reader_keeps_const_and_element_type_under_every_spacing():
    text = """
    int pvamd_spacing(const float* a, const   double  *b, int64_t * c, uint8_t*d, const int32_t*e,
                      const pvamd_grid_t* grid, pvamd_mesh_plan_t *plan_out, const  pvamd_joint_t * joints,
                      void *scratch, const int n, double x, void* stream);
    int64_t pvamd_size(int32_t n);
    """
    (declarations, defines), parameters = _header.parse(text, MIRRORS), _header.parameters(text)
    assert _header.read_parameters() == _lib.PARAMETERS
    assert defines == {} and list(parameters) == list(declarations) == ["pvamd_spacing", "pvamd_size"]
    assert parameters["pvamd_spacing"] == [
        ("a", "float", True, True), ("b", "double", True, True), ("c", "int64_t", True, False), ("d", "uint8_t", True, False),
        ("e", "int32_t", True, True), ("grid", "pvamd_grid_t", True, True), ("plan_out", "pvamd_mesh_plan_t", True, False),
        ("joints", "pvamd_joint_t", True, True), ("scratch", "void", True, False), ("n", "int", False, True),
        ("x", "double", False, False), ("stream", "void", True, False)]
    assert parameters["pvamd_size"] == [("n", "int32_t", False, False)]
    c = ctypes
    assert declarations["pvamd_spacing"][1] == [c.c_void_p] * 5 + [c.POINTER(_lib.GridDesc), c.POINTER(_lib.MeshPlan)] + \
        [c.c_void_p] * 2 + [c.c_int, c.c_double, c.c_void_p]


# ---------------------------------------------------------------- 2 and 3. the call sites, walked with ast
def status_entries():
    """Entry points that return a status: `int` with at least one pointer parameter (the others report a constant or a choice)."""
    return {name for name, (restype, _) in _lib.SIGNATURES.items()
            if restype is ctypes.c_int and any(p[2] for p in _lib.PARAMETERS[name])}


def walk_package():
    """(calls, direct): every `_lib.call(...)` / `call(...)` as (file, function, node), and every other use of a status-returning
    entry point -- `<anything>.pvamd_x`, `getattr(<lib>, ...)`, `entry_address("pvamd_x")` -- as (file, function, entry)."""
    status = status_entries()
    calls, direct = [], []

    def visit(node, file, function):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            function = f"{function}.{node.name}" if function else node.name
        if isinstance(node, ast.Call):
            f = node.func
            if (isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name) and f.value.id == "_lib") or \
                    (file == "_lib.py" and isinstance(f, ast.Name) and f.id == "call"):
                calls.append((file, function, node))
            elif isinstance(f, ast.Name) and f.id == "getattr" and ast.unparse(node.args[0]) in ("lib", "load()", "_lib.load()"):
                direct.append((file, function, "getattr(" + ast.unparse(node.args[0]) + ", ...)"))
            elif isinstance(f, ast.Attribute) and f.attr == "entry_address" and node.args and \
                    isinstance(node.args[0], ast.Constant) and node.args[0].value in status:
                direct.append((file, function, "entry_address " + node.args[0].value))
        if isinstance(node, ast.Attribute) and node.attr in status:
            direct.append((file, function, node.attr))
        for child in ast.iter_child_nodes(node):
            visit(child, file, function)

    for file in sorted(os.listdir(PACKAGE)):
        if file.endswith(".py"):
            with open(os.path.join(PACKAGE, file)) as f:
                visit(ast.parse(f.read()), file, "")
    return calls, direct


def literal_names(node):
    """The entry names a call site's first argument can take: a string literal, or a conditional between literals."""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return [node.value]
    if isinstance(node, ast.IfExp):
        a, b = literal_names(node.body), literal_names(node.orelse)
        return a + b if a and b else []
    return []


# the two sites whose name is not a literal: the backward of a query names the entry of the mode its forward ran in
COMPUTED_NAMES = {("autograd.py", "CachedQuery.backward"): "cached", ("autograd.py", "ComposedQuery.backward"): "composed"}


def test_every_call_site_names_a_declared_entry_with_the_declared_argument_count():
    from pytorch_volumetric_amd import autograd
    P = _lib.PARAMETERS
    calls, _ = walk_package()
    assert len(calls) >= 80, len(calls)  # the walk finds the sites: 82 of them
    computed = {}
    for file, function, node in calls:
        where = f"{file}:{node.lineno} ({function})"
        assert node.args and not isinstance(node.args[0], ast.Starred), where
        names = literal_names(node.args[0])
        if not names:
            computed[file, function] = ast.unparse(node.args[0])
            names = [pattern.format(COMPUTED_NAMES[file, function]) for pattern in autograd._BACKWARD.values()]
        f64 = [k for k in node.keywords if k.arg == "f64"]
        assert len(node.keywords) == len(f64) <= 1, where
        for name in names:
            assert name in P, f"{where}: {name} is not declared"
            variants = [name] + ([name + "_f64"] if f64 else [])
            for variant in variants:
                assert variant in P, f"{where}: {variant} is not declared"
                expected = len(P[variant]) - (1 if P[variant] and P[variant][-1][0] == "stream" else 0)
                if not any(isinstance(a, ast.Starred) for a in node.args):
                    assert len(node.args) - 1 == expected, f"{where}: {variant} takes {expected} arguments before the stream"
    assert computed == {site: "ctx.backward_entry" for site in COMPUTED_NAMES}, computed


# Outside _lib.py, a status-returning entry point is called directly only here: the hand-tuned host paths the benchmark times,
# which keep a function object in a remembered plan or pass raw data_ptr() integers.
DIRECT_SITES = {
    ("sdf.py", "CachedSDF._fast_plan", "pvamd_cached_query"): "the function object the planned branches of __call__ / query_into call",
    ("sdf.py", "CachedSDF._fast_plan", "entry_address pvamd_cached_query"): "its address, for the host-call module (csrc/fastcall.cpp)",
    ("sdf.py", "ComposedSDF._call_plan", "pvamd_composed_query"): "the function object the planned branch of __call__ calls",
    ("sdf.py", "ComposedSDF._call_plan", "entry_address pvamd_composed_query"): "its address, for the host-call module",
    ("sdf.py", "ComposedSDF.__call__", "pvamd_composed_query_grouped"): "the planned branch's chunk-grouped launch, on raw addresses",
    ("model_to_sdf.py", "RobotSDF._configure", "pvamd_configure_chain"): "set_joint_configuration's one launch, on raw addresses",
    ("model_to_sdf.py", "RobotSDF._configure", "pvamd_chain_fk"): "its three-launch form for many links, on raw addresses",
    ("model_to_sdf.py", "RobotSDF._configure", "pvamd_transform_stack"): "its three-launch form for many links, on raw addresses",
}


def test_only_the_listed_sites_call_an_entry_point_directly():
    _, direct = walk_package()
    outside = {site for site in direct if site[0] != "_lib.py"}
    assert outside == set(DIRECT_SITES), sorted(outside ^ set(DIRECT_SITES))
    # inside _lib.py: load binds every declaration, and entry_address (what feeds the host-call module) and call itself look an
    # entry up by name
    inside = {(function, what) for file, function, what in direct if file == "_lib.py"}
    assert inside == {("load", "getattr(lib, ...)"), ("entry_address", "getattr(load(), ...)"), ("call", "getattr(load(), ...)")}, inside
    wrapped = set()

    def visit(node, file, function):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            function = f"{function}.{node.name}" if function else node.name
        if isinstance(node, ast.Attribute) and node.attr == "ptr" and ast.unparse(node.value) == "_lib":
            wrapped.add((file, function))
        for child in ast.iter_child_nodes(node):
            visit(child, file, function)

    for file in os.listdir(PACKAGE):
        if file.endswith(".py") and file != "_lib.py":
            with open(os.path.join(PACKAGE, file)) as f:
                visit(ast.parse(f.read()), file, "")
    assert not wrapped, sorted(wrapped)  # no site outside _lib.py wraps a tensor by hand


# ---------------------------------------------------------------- 4. refusals that need no GPU
def test_refusals_come_before_the_library_is_asked(monkeypatch):
    def no_load():
        raise AssertionError("load() was called for a refused call")
    monkeypatch.setattr(_lib, "load", no_load)
    desc = _lib.GridDesc()
    with pytest.raises(_lib.PvamdError, match="pvamd_no_such_entry is not declared"):
        _lib.call("pvamd_no_such_entry", 1, 2)
    with pytest.raises(_lib.PvamdError, match="pvamd_cached_query_interp_backward_f64_f64 is not declared"):
        _lib.call("pvamd_cached_query_interp_backward_f64", f64=True)
    with pytest.raises(_lib.PvamdError, match=r"pvamd_cached_query takes 6 arguments before the stream \(grid, points, P, .*given 5"):
        _lib.call("pvamd_cached_query", desc, None, 0, None, None)
    with pytest.raises(_lib.PvamdError, match="pvamd_cached_query_f64 takes 6 arguments before the stream.*given 7"):
        _lib.call("pvamd_cached_query", desc, None, 0, None, None, None, 0, f64=True)
    with pytest.raises(_lib.PvamdError, match=r"pvamd_mesh_query_plan takes 5 arguments \(P, F, .*given 4"):
        _lib.call("pvamd_mesh_query_plan", 1, 1, 0, 0)
    with pytest.raises(_lib.PvamdError, match="pvamd_cached_query: `points` takes a contiguous GPU tensor of torch.float32 or None, "
                                              "given a contiguous torch.float32 tensor on cpu"):
        _lib.call("pvamd_cached_query", desc, torch.zeros(5, 3), 5, None, None, None)
    with pytest.raises(_lib.PvamdError, match="pvamd_group_points: `scratch` takes a contiguous GPU tensor or None, given .* on cpu"):
        _lib.call("pvamd_group_points", None, 5, torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(_lib.PvamdError, match="pvamd_cached_query: `points` takes .*given list"):
        _lib.call("pvamd_cached_query", desc, [0.0, 0.0, 0.0], 1, None, None, None)
    with pytest.raises(_lib.PvamdError, match="pvamd_cached_query: `grid` takes a GridDesc, given MeshDesc"):
        _lib.call("pvamd_cached_query", _lib.MeshDesc(), None, 0, None, None, None)


def test_host_structs_and_scalars_pass_and_a_bad_scalar_is_named():
    """The plan entry points take no tensor and no stream: they run without a GPU, through the same path."""
    plan = _lib.MeshPlan()
    _lib.call("pvamd_mesh_query_plan", 10_000, 5000, True, False, plan)  # bool goes as int
    assert plan.path != _lib.MESH_PATH_NONE and plan.groups > 0
    again = _lib.mesh_query_plan(10_000, 5000, True, False)
    assert bytes(again) == bytes(plan)
    with pytest.raises(_lib.PvamdError, match="pvamd_mesh_query_plan: `F` takes a int32_t, given str"):
        _lib.call("pvamd_mesh_query_plan", 10_000, "many", True, False, plan)
    with pytest.raises(_lib.PvamdError, match=r"pvamd_mesh_query_plan: invalid argument \(a size/shape argument is out of range\)"):
        _lib.call("pvamd_mesh_query_plan", -1, 5000, True, False, plan)  # the status goes through check under the entry's name


def test_the_loop_of_call_and_the_stated_rule_agree(monkeypatch):
    """call()'s loop is _takes() written out per kind: over every kind of parameter and a set of arguments, call() passes exactly
    what _takes() accepts, and names the parameter of what it refuses.  CPU tensors stand in for tensors on the current GPU: they
    report device -1, which is made the current one here."""
    monkeypatch.setattr(_lib, "current_device_index", lambda: -1)
    kinds = (_lib._TYPED, _lib._TYPED, _lib._UNTYPED, _lib._SCALAR, _lib._STRUCT)
    wants = (torch.float32, torch.int64, None, None, _lib.GridDesc)
    names = ("values", "index", "scratch", "count", "grid")
    passed = []
    monkeypatch.setitem(_lib._plans, "pvamd_stand_in", [kinds, wants, names, False, lambda *a: passed.append(a) and 0])
    good = [torch.zeros(4), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.uint8), 3, _lib.GridDesc()]
    candidates = [None, torch.zeros(4), torch.zeros(4).double(), torch.zeros(2, 3).t(), torch.zeros(4, dtype=torch.int64),
                  torch.zeros(2, 3, dtype=torch.int64).t(), [1.0], 3, _lib.GridDesc(), _lib.MeshDesc()]
    verdicts = {kind_at: set() for kind_at in range(5)}
    for at in range(5):
        for candidate in candidates:
            args = list(good)
            args[at] = candidate
            takes = _lib._takes(candidate, kinds[at], wants[at], -1)
            verdicts[at].add(takes)
            before = len(passed)
            if takes:
                _lib.call("pvamd_stand_in", *args)
                assert len(passed) == before + 1, (names[at], candidate)
            else:
                with pytest.raises(_lib.PvamdError, match=f"pvamd_stand_in: `{names[at]}` takes"):
                    _lib.call("pvamd_stand_in", *args)
                assert len(passed) == before, (names[at], candidate)
    assert verdicts == {0: {True, False}, 1: {True, False}, 2: {True, False}, 3: {True}, 4: {True, False}}
    assert _lib._takes(torch.zeros(4), _lib._TYPED, torch.float32, 0) is False  # elsewhere than on the current device
    with pytest.raises(_lib.PvamdError, match="`values` takes a contiguous GPU tensor of torch.float32 or None, given .* on cpu"):
        monkeypatch.setattr(_lib, "current_device_index", lambda: 0)
        _lib.call("pvamd_stand_in", *good)
