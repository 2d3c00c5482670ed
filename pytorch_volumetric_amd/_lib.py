"""ctypes binding of libpvamd.so (C ABI in include/pvamd.h).

The HIP library is the only compute path of this package: there is no CPU or eager-PyTorch fallback.  Loading
fails loudly if the shared object is missing, and every query raises if no MI355X is visible.
"""
import ctypes
import functools
import os
import re

import torch

from pytorch_volumetric_amd import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVAMD_LIB") or os.path.join(_HERE, "csrc", "libpvamd.so")  # PVAMD_LIB: A/B builds (tools/)


# Buffer sizes: the library's exported size functions are the definition (include/pvamd.h) -- what they report is what the
# launch code carves.  Nothing here restates their arithmetic.  A size depends on the arguments only, and an optimiser loop
# asks for the same few: remembered, it costs less than the ctypes call.
_remembered = functools.lru_cache(maxsize=64)


@_remembered
def rec_floats(F):
    """pvamd_mesh_rec_floats: records are stored in whole tiles."""
    return load().pvamd_mesh_rec_floats(F)


@_remembered
def tiles_floats(F):
    """pvamd_mesh_tiles_floats: tile spheres followed by group spheres."""
    return load().pvamd_mesh_tiles_floats(F)


@_remembered
def mesh_scratch_bytes(P):
    """pvamd_mesh_scratch_bytes: the slots of the point groups a mesh query hands over, then the by-point part of an unordered one."""
    return load().pvamd_mesh_scratch_bytes(P)


@_remembered
def morton_order_scratch_bytes(P):
    """pvamd_morton_order_scratch_bytes: enough for either sort, whichever the library was built to pick at P."""
    return load().pvamd_morton_order_scratch_bytes(P)


@_remembered
def min_over_points_scratch_bytes(S, A, P, per_leaf):
    """pvamd_min_over_points_scratch_bytes: one 16-byte key per pair and point chunk."""
    return load().pvamd_min_over_points_scratch_bytes(S, A, P, int(per_leaf))


@_remembered
def min_over_points_backward_scratch_bytes(S, A, per_leaf):
    """pvamd_min_over_points_backward_scratch_bytes: three values per pair, sized for float64."""
    return load().pvamd_min_over_points_backward_scratch_bytes(S, A, int(per_leaf))


@_remembered
def hinge_over_points_scratch_bytes(S, A, P, per_leaf):
    """pvamd_hinge_over_points_scratch_bytes: one 16-byte (sum, count) per pair and point chunk."""
    return load().pvamd_hinge_over_points_scratch_bytes(S, A, P, int(per_leaf))


@_remembered
def hinge_over_points_backward_scratch_bytes(S, A, P, per_leaf, f64):
    """pvamd_hinge_over_points_backward_scratch_bytes: the composed backward's plan; per_leaf runs one-leaf passes, whose
    dpoints term needs one more [P][3] buffer when there is more than one leaf."""
    return load().pvamd_hinge_over_points_backward_scratch_bytes(S, A, P, int(per_leaf), int(f64))


@_remembered
def leaf_pair_scratch_bytes(K, A, max_points, f64, backward):
    """pvamd_leaf_pair_scratch_bytes: the forward's one 16-byte key per pair, configuration and 4096-point chunk when a set
    holds more than one chunk (else none); the backward's dMs and dMt per pair and configuration."""
    return load().pvamd_leaf_pair_scratch_bytes(K, A, max_points, int(f64), int(backward))


@_remembered
def leaf_pair_hinge_scratch_bytes(K, A, max_points, f64, backward):
    """pvamd_leaf_pair_hinge_scratch_bytes: the forward's one 16-byte (sum, count) per pair, configuration and 4096-point chunk
    when a set holds more than one chunk (else none); the backward's dC slab of 12 values per pair, configuration and
    1024-point chunk, then dMs and dMt per pair and configuration."""
    return load().pvamd_leaf_pair_hinge_scratch_bytes(K, A, max_points, int(f64), int(backward))


@_remembered
def ray_cast_backward_scratch_bytes(S, A, R, f64):
    """pvamd_ray_cast_backward_scratch_bytes: 12 float64 per ray chunk, leaf and configuration, then 6 float64 per configuration
    split and ray when the plan splits the configurations."""
    return load().pvamd_ray_cast_backward_scratch_bytes(S, A, R, int(f64))


@_remembered
def chamfer_normal_eq_scratch_bytes(B, N):
    """pvamd_chamfer_normal_eq_scratch_bytes: 28 float64 sums and one int64 count per pose and point chunk."""
    return load().pvamd_chamfer_normal_eq_scratch_bytes(B, N)


@_remembered
def semantic_normal_eq_scratch_bytes(B, N):
    """pvamd_semantic_normal_eq_scratch_bytes: 28 float64 sums and five int64 counts per pose and point chunk."""
    return load().pvamd_semantic_normal_eq_scratch_bytes(B, N)


@_remembered
def joint_normal_eq_scratch_bytes(A, S, N):
    """pvamd_joint_normal_eq_scratch_bytes: 28 float64 sums and five int64 counts per configuration, leaf and point chunk."""
    return load().pvamd_joint_normal_eq_scratch_bytes(A, S, N)


@_remembered
def distance_transform_scratch_bytes(nx, ny, nz, signed):
    """pvamd_distance_transform_scratch_bytes: one int32 per voxel, site class and line pass that hands on a state."""
    return load().pvamd_distance_transform_scratch_bytes(nx, ny, nz, int(signed))


@_remembered
def redistance_scratch_bytes(nx, ny, nz):
    """pvamd_redistance_scratch_bytes: the sample column, then one 8-byte state per voxel for pass 1 and for pass 2 of each family."""
    return load().pvamd_redistance_scratch_bytes(nx, ny, nz)


@_remembered
def surface_scratch_bytes(nx, ny, nz):
    """pvamd_surface_scratch_bytes: the cell -> vertex id map, the scanned chunk sums, then three bytes of classes per voxel."""
    return load().pvamd_surface_scratch_bytes(nx, ny, nz)


@_remembered
def composed_query_kernel(A, P, flags):
    """pvamd_composed_query_kernel: the kernel (CO_KERNEL_*) pvamd_composed_query launches for A configurations of P points."""
    return load().pvamd_composed_query_kernel(A, P, flags)


def scratch_buffer(nbytes, dev):
    """The one place a byte-sized scratch buffer of an entry point is allocated (uint8, uninitialised)."""
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


_c_float_p = ctypes.POINTER(ctypes.c_float)


class GridDesc(ctypes.Structure):
    """pvamd_grid_t"""
    _fields_ = [
        ("vox", ctypes.c_void_p),
        ("dmin", ctypes.c_double * 3),
        ("dmax", ctypes.c_double * 3),
        ("dres", ctypes.c_double * 3),
        ("fmin", ctypes.c_float * 3),
        ("fmax", ctypes.c_float * 3),
        ("fres", ctypes.c_float * 3),
        ("bb_min", ctypes.c_float * 3),
        ("bb_max", ctypes.c_float * 3),
        ("shape", ctypes.c_int32 * 3),
        ("index_f64", ctypes.c_int32),
        ("oob_mode", ctypes.c_int32),
        ("finalized", ctypes.c_int32),
        ("vlo", ctypes.c_float * 3),
        ("vhi", ctypes.c_float * 3),
        ("inv32", ctypes.c_float * 3),
        ("err32", ctypes.c_float * 3),
        ("rule", ctypes.c_int32),
        ("dbb_min", ctypes.c_double * 3),
        ("dbb_max", ctypes.c_double * 3),
        ("range_n2", ctypes.c_float),
        ("reserved0", ctypes.c_float),
    ]


class MeshDesc(ctypes.Structure):
    """pvamd_mesh_t"""
    _fields_ = [
        ("normal", ctypes.c_void_p),
        ("rec", ctypes.c_void_p),
        ("tiles", ctypes.c_void_p),
        ("rec_of_face", ctypes.c_void_p),
        ("F", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("ray_dir", ctypes.c_double * 3),
        ("pair_counters", ctypes.c_void_p),
    ]


class MeshPlan(ctypes.Structure):
    """pvamd_mesh_plan_t: the launches of a mesh query / mesh chamfer call (pvamd_mesh_query_plan, pvamd_chamfer_mesh_plan)."""
    _fields_ = [("path", ctypes.c_int32), ("order", ctypes.c_int32), ("groups", ctypes.c_int32), ("slots", ctypes.c_int32),
                ("scan_waves", ctypes.c_int32), ("parts", ctypes.c_int32), ("part_waves", ctypes.c_int32)]


def mesh_query_plan(P, F, has_scratch, unordered=False):
    """pvamd_mesh_query_plan as a MeshPlan."""
    plan = MeshPlan()
    call("pvamd_mesh_query_plan", P, F, has_scratch, unordered, plan)
    return plan


def chamfer_mesh_plan(N, rows, F, has_scratch):
    """pvamd_chamfer_mesh_plan as a MeshPlan."""
    plan = MeshPlan()
    call("pvamd_chamfer_mesh_plan", N, rows, F, has_scratch, plan)
    return plan


class JointDesc(ctypes.Structure):
    """pvamd_joint_t"""
    _fields_ = [("parent", ctypes.c_int32), ("jtype", ctypes.c_int32), ("jcol", ctypes.c_int32),
                ("leaf_slot", ctypes.c_int32), ("axis", ctypes.c_float * 3), ("reserved", ctypes.c_float),
                ("origin", ctypes.c_float * 12)]


class PvamdError(RuntimeError):
    pass


# The binding is read from include/pvamd.h, the one definition of the C ABI (_header.py states the rules).  SIGNATURES: name ->
# (restype, argtypes) of every declaration; scalars map to their ctypes scalar and pointers to c_void_p, except the host structs
# passed with byref -- `pvamd_grid_t* grid`, `pvamd_mesh_t* mesh`, `pvamd_mesh_plan_t* plan_out` -- which map to POINTER of the
# mirror above.  H: the header's integer #defines.  PARAMETERS: name -> [(parameter name, base type, is a pointer, is const)],
# the element types that argtypes drops and call() checks tensors against.  The test-suite checks that every entry is exported
# by the .so and that the mirrors have the header's layout.
_MIRRORS = {"GridDesc": GridDesc, "MeshDesc": MeshDesc, "MeshPlan": MeshPlan}
try:
    SIGNATURES, H = _header.read(_MIRRORS)
    PARAMETERS = _header.read_parameters()
except OSError as e:
    raise PvamdError(f"{_header.HEADER_PATH} cannot be read ({e}): the binding of libpvamd.so is read from the header that "
                     f"the library was built from, and there is no second copy of it") from e

ABI_VERSION = H["PVAMD_ABI_VERSION"]  # of the header in this tree: load() compares it with the .so's
OOB_LOOKUP_GT_SDF = H["PVAMD_OOB_LOOKUP_GT_SDF"]
OOB_BOUNDING_BOX = H["PVAMD_OOB_BOUNDING_BOX"]
COMPOSED_INLINE_EXACT = H["PVAMD_COMPOSED_INLINE_EXACT"]
COMPOSED_FORCE_PER_LANE = H["PVAMD_COMPOSED_FORCE_PER_LANE"]
COMPOSED_FORCE_WAVE_TILE = H["PVAMD_COMPOSED_FORCE_WAVE_TILE"]
COMPOSED_OUT_PACKED = H["PVAMD_COMPOSED_OUT_PACKED"]
COMPOSED_NO_GROUPING = H["PVAMD_COMPOSED_NO_GROUPING"]
COMPOSED_FORCE_FUSED = H["PVAMD_COMPOSED_FORCE_FUSED"]
TILE_POINTS = H["PVAMD_COMPOSED_TILE_POINTS"]  # the bucketed and packed composed queries take whole tiles of points
CO_KERNEL_PER_LANE = H["PVAMD_CO_KERNEL_PER_LANE"]
CO_KERNEL_WAVE_TILE = H["PVAMD_CO_KERNEL_WAVE_TILE"]
CO_KERNEL_FUSED = H["PVAMD_CO_KERNEL_FUSED"]
ORDER_KERNEL_SMALL = H["PVAMD_ORDER_KERNEL_SMALL"]
ORDER_KERNEL_COUNTING = H["PVAMD_ORDER_KERNEL_COUNTING"]
ORDER_KERNEL_RADIX = H["PVAMD_ORDER_KERNEL_RADIX"]
MESH_PATH_NONE = H["PVAMD_MESH_PATH_NONE"]
MESH_PATH_LISTED = H["PVAMD_MESH_PATH_LISTED"]
MESH_PATH_SCAN = H["PVAMD_MESH_PATH_SCAN"]
MESH_PATH_SCAN_HEAVY = H["PVAMD_MESH_PATH_SCAN_HEAVY"]
MESH_ORDER_GIVEN = H["PVAMD_MESH_ORDER_GIVEN"]
MESH_ORDER_INSIDE = H["PVAMD_MESH_ORDER_INSIDE"]
MESH_ORDER_SORT_CALL = H["PVAMD_MESH_ORDER_SORT_CALL"]
RULE_VALID_ON_INDEX = H["PVAMD_RULE_VALID_ON_INDEX"]
RULE_ROUND_HALF_AWAY = H["PVAMD_RULE_ROUND_HALF_AWAY"]
RULE_ROUND_FLOOR_HALF = H["PVAMD_RULE_ROUND_FLOOR_HALF"]
RULE_RES_F64 = H["PVAMD_RULE_RES_F64"]
LEAF_MODES = {"nearest": H["PVAMD_LEAF_NEAREST"], "trilinear": H["PVAMD_LEAF_TRILINEAR"]}
MOP_CHUNK = H["PVAMD_MOP_CHUNK"]
REG_CHUNK = H["PVAMD_REG_CHUNK"]
REG_SUMS = H["PVAMD_REG_SUMS"]  # the row length of pvamd_chamfer_normal_eq's out_sums
POINT_SURFACE = H["PVAMD_POINT_SURFACE"]  # POINT_*: the kind of a point of pvamd_semantic_normal_eq
POINT_FREE = H["PVAMD_POINT_FREE"]
POINT_OCCUPIED = H["PVAMD_POINT_OCCUPIED"]
POINT_IGNORE = H["PVAMD_POINT_IGNORE"]  # and every larger value
SEM_COUNTS = H["PVAMD_SEM_COUNTS"]  # the row length of pvamd_semantic_normal_eq's out_counts
JOINT_MAX = H["PVAMD_JOINT_MAX"]  # the most joint values of pvamd_chain_twists, pvamd_joint_assemble and pvamd_joint_lm_step
JOINT_MAX_LEAVES = H["PVAMD_JOINT_MAX_LEAVES"]  # the most leaves of pvamd_joint_normal_eq
RAY_MISS = H["PVAMD_RAY_MISS"]  # RAY_*: the status codes of the ray-cast entry points
RAY_HIT = H["PVAMD_RAY_HIT"]
RAY_MAX_STEPS = H["PVAMD_RAY_MAX_STEPS"]
RAY_INVALID = H["PVAMD_RAY_INVALID"]
RAY_BACKWARD_CHUNK = H["PVAMD_RAY_BACKWARD_CHUNK"]
EDT_NO_SITE = H["PVAMD_EDT_NO_SITE"]  # DistanceTransform.squared where the site class is empty
REDIST_KEPT = H["PVAMD_REDIST_KEPT"]  # Redistance.sites of a voxel inside the band
MARK_FREE = H["PVAMD_MARK_FREE"]  # MARK_*: a scan's classification of a voxel (pvamd_ray_mark); 0: no ray touched it
MARK_HIT = H["PVAMD_MARK_HIT"]
LATTICE_MAX_AXIS = H["PVAMD_LATTICE_MAX_AXIS"]  # the longest axis of a volume lattice; *_MIN_AXIS, *_MAX_VOXELS: per feature
EDT_MIN_AXIS = H["PVAMD_EDT_MIN_AXIS"]
EDT_MAX_VOXELS = H["PVAMD_EDT_MAX_VOXELS"]
RAY_MARK_MIN_AXIS = H["PVAMD_RAY_MARK_MIN_AXIS"]
TSDF_MIN_AXIS = H["PVAMD_TSDF_MIN_AXIS"]
TSDF_MAX_VOXELS = H["PVAMD_TSDF_MAX_VOXELS"]
TSDF_MAX_PIXELS = H["PVAMD_TSDF_MAX_PIXELS"]  # K * H * W of one pvamd_tsdf_integrate call
REDIST_MIN_AXIS = H["PVAMD_REDIST_MIN_AXIS"]
REDIST_MAX_VOXELS = H["PVAMD_REDIST_MAX_VOXELS"]
SURFACE_MIN_AXIS = H["PVAMD_SURFACE_MIN_AXIS"]
SURFACE_MAX_VOXELS = H["PVAMD_SURFACE_MAX_VOXELS"]
E_SHAPE = H["PVAMD_E_SHAPE"]
_ERRORS = {H["PVAMD_E_NULL"]: "a required pointer is NULL", H["PVAMD_E_SHAPE"]: "a size/shape argument is out of range",
           H["PVAMD_E_ALIGN"]: "a pointer is misaligned", H["PVAMD_E_MODE"]: "unknown enum value"}

_lib = None


def load():
    """Load libpvamd.so once; raise if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PvamdError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C pytorch_volumetric_amd/csrc`) from the repository root. There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.pvamd_abi_version() != ABI_VERSION:
        raise PvamdError(f"libpvamd ABI {lib.pvamd_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    # an A/B build (tools/build_variant.sh: one translation unit compiled with tuning / counter knobs) names itself; the product
    # path and the tests never load one by accident
    if hasattr(lib, "pvamd_variant"):
        lib.pvamd_variant.restype = ctypes.c_char_p
        what = lib.pvamd_variant().decode()
        if os.environ.get("PVAMD_ALLOW_VARIANT") != "1":
            raise PvamdError(f"{LIB_PATH} is an A/B build ({what}); set PVAMD_ALLOW_VARIANT=1 to time it, or unset PVAMD_LIB")
        import sys
        print(f"[pvamd] A/B build loaded: {what} ({LIB_PATH})", file=sys.stderr)
    _lib = lib
    return lib


def check(code, what):
    if code == 0:
        return
    if code < 0:
        raise PvamdError(f"{what}: invalid argument ({_ERRORS.get(code, code)})")
    raise PvamdError(f"{what}: hipError_t {code}")


_gpu_checked = False
_devices = {}


def require_gpu():
    """The compute device of this package.  No GPU -> loud failure (never a silent CPU path)."""
    global _gpu_checked
    if not _gpu_checked:  # availability cannot change within a process; the check costs several us per call otherwise
        if not torch.cuda.is_available():
            raise PvamdError("pytorch_volumetric_amd needs an AMD MI355X (gfx950) visible to PyTorch-ROCm; "
                             "torch.cuda.is_available() is False and there is no CPU fallback")
        torch.cuda.current_device()  # torch's lazy CUDA/HIP initialisation, once
        _gpu_checked = True
    index = torch._C._cuda_getDevice()
    dev = _devices.get(index)
    if dev is None:
        dev = _devices[index] = torch.device("cuda", index)
    return dev


def stream_ptr():
    """hipStream_t of torch's current stream on the current device (the raw-handle call: torch.cuda.current_stream()
    builds a Stream object and re-validates the device, ~8 us)."""
    if not _gpu_checked:
        require_gpu()
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


class on_device:
    """`with on_device(dev):` = torch.cuda.device(dev) without its per-entry validation when dev is already current."""
    __slots__ = ("index", "prev")

    def __init__(self, dev):
        self.index = dev.index if dev.index is not None else torch._C._cuda_getDevice()
        self.prev = -1

    def __enter__(self):
        cur = torch._C._cuda_getDevice()
        if cur != self.index:
            self.prev = cur
            torch.cuda.set_device(self.index)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


_fast = False  # False: not looked for yet; None: absent / disabled


def fastcall():
    """The optional host-call module (csrc/fastcall.cpp -> pytorch_volumetric_amd/_pvamd_fast.so; `make -C csrc fast`,
    built by __graft_entry__.build()): the two allocations + the C-ABI call of the drop-in fast paths without the interpreter
    in between (cached(points) 7.4 -> 5.9 us of host time).  Plumbing only -- the same entry points of the same libpvamd.so,
    by address; None when it has not been built or PVAMD_NO_FASTCALL=1, and the ctypes path runs instead."""
    global _fast
    if _fast is False:
        _fast = None
        if os.environ.get("PVAMD_NO_FASTCALL") != "1":
            try:
                from pytorch_volumetric_amd import _pvamd_fast
                _pvamd_fast.set_error_class(PvamdError)
                _fast = _pvamd_fast
            except ImportError:
                pass
    return _fast


def entry_address(name):
    """Address of a libpvamd.so entry point (what _pvamd_fast calls through)."""
    return ctypes.cast(getattr(load(), name), ctypes.c_void_p).value


# Bumped whenever an attribute that the cached call plans of CachedSDF / ComposedSDF depend on is assigned
# (CachedSDF.__setattr__): a plan remembers the epoch it was built in and is rebuilt when it has moved on.
EPOCH = [0]
current_device_index = torch._C._cuda_getDevice
current_raw_stream = torch._C._cuda_getCurrentRawStream


def same_gpu(out_device, dev):
    """Whether results wanted on `out_device` (a str / torch.device as the reference's `device=` arguments take them)
    can stay where the kernel wrote them, on `dev`."""
    d = torch.device(out_device)
    return d.type == "cuda" and (d.index is None or d.index == dev.index)


def ptr(t):
    """Device address of a tensor (None -> NULL)."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


_ELEMENTS = {"float": torch.float32, "double": torch.float64, "int32_t": torch.int32, "int64_t": torch.int64,
             "uint8_t": torch.uint8}
_TYPED, _UNTYPED, _SCALAR, _STRUCT = range(4)
_plans = {}


def _plan(name):
    """[kinds, wants, names, whether the stream is appended, the bound function once it has been called] of a declared entry
    point, made once per name.  Per parameter the caller passes: its kind, the dtype of a typed data pointer / the mirror of a
    host struct / None, and its name in the header."""
    params = PARAMETERS.get(name)
    if params is None:
        raise PvamdError(f"{name} is not declared in include/pvamd.h")
    stream = bool(params) and params[-1] == ("stream", "void", True, False)
    kinds, wants = [], []
    for pname, ctype, pointer, _ in params[:-1] if stream else params:
        if not pointer:
            kind, want = _SCALAR, None
        elif (ctype, pname) in _header.HOST_STRUCTS:
            kind, want = _STRUCT, _MIRRORS[_header.HOST_STRUCTS[ctype, pname]]
        elif ctype in _ELEMENTS:
            kind, want = _TYPED, _ELEMENTS[ctype]
        else:  # void* and the device arrays of structs take any dtype
            kind, want = _UNTYPED, None
        kinds.append(kind)
        wants.append(want)
    plan = _plans[name] = [tuple(kinds), tuple(wants), tuple(p[0] for p in params), stream, None]
    return plan


def _takes(arg, kind, want, dev):
    """Whether call() takes `arg` for a parameter of `kind`: THE statement of the rule.  call()'s loop is this function written
    out per kind (a call per argument would cost what the checks cost); tests/test_binding_call.py holds the two together."""
    if kind == _SCALAR:
        return True
    if kind == _STRUCT:
        return isinstance(arg, want)
    return arg is None or (torch.is_tensor(arg) and (kind == _UNTYPED or arg.dtype is want) and arg.is_contiguous()
                           and arg.get_device() == dev)


def _refusal(name, plan, args, dev):
    """The PvamdError for the first argument _takes() refuses, worked out off call()'s loop."""
    for arg, kind, want, pname in zip(args, *plan[:3]):
        if _takes(arg, kind, want, dev):
            continue
        if kind == _STRUCT:
            return PvamdError(f"{name}: `{pname}` takes a {want.__name__}, given {type(arg).__name__}")
        expected = f"a contiguous GPU tensor{'' if want is None else ' of ' + str(want)} or None"
        if not torch.is_tensor(arg):
            return PvamdError(f"{name}: `{pname}` takes {expected}, given {type(arg).__name__}")
        if arg.is_cuda and arg.is_contiguous() and (want is None or arg.dtype is want):
            return PvamdError(f"{name}: `{pname}` is on GPU {arg.get_device()} and the current device is GPU {dev}, whose stream "
                              f"the call would take (wrap it in `with _lib.on_device(dev):`)")
        return PvamdError(f"{name}: `{pname}` takes {expected}, given a "
                          f"{'contiguous' if arg.is_contiguous() else 'non-contiguous'} {arg.dtype} tensor on {arg.device}")
    raise AssertionError(f"{name}: call() refused arguments that _takes() accepts: the two have drifted apart")


def call(name, *args, f64=False):
    """The one way the package calls a status-returning entry point: `name` (+ "_f64" with f64=True) with every argument
    checked against its parameter in include/pvamd.h, the current stream appended where the declaration ends in `void* stream`,
    and the status through check().  A typed data pointer takes None (NULL) or a contiguous GPU tensor of the element type's
    dtype -- a tensor of another dtype on purpose says so with .view(dtype); void* and the device arrays of structs a contiguous
    GPU tensor of any dtype; a host struct pointer the ctypes mirror itself; scalars pass through.  Every tensor is on the
    current device, whose stream it is (get_device() is its index there and -1 off a GPU).  A refused argument raises PvamdError
    naming the parameter, and nothing is launched.  Per tensor: four reads and no object built -- the address goes as an int,
    which c_void_p takes."""
    if f64:
        name += "_f64"
    plan = _plans.get(name) or _plan(name)
    kinds, wants, names, stream, fn = plan
    if len(args) != len(kinds):
        raise PvamdError(f"{name} takes {len(kinds)} arguments{' before the stream' if stream else ''} "
                         f"({', '.join(names[:len(kinds)])}), given {len(args)}")
    try:
        dev = current_device_index()
    except RuntimeError:  # no GPU: no tensor is on it, and each is refused by name
        dev = -2
    out = []
    append = out.append
    try:
        for arg, kind, want in zip(args, kinds, wants):
            if kind == _TYPED:
                if arg is None:
                    append(None)
                elif arg.dtype is want and arg.is_contiguous() and arg.get_device() == dev:
                    append(arg.data_ptr())
                else:
                    raise AttributeError
            elif kind == _SCALAR:
                append(arg)
            elif kind == _UNTYPED:
                if arg is None:
                    append(None)
                elif arg.is_contiguous() and arg.get_device() == dev:
                    append(arg.data_ptr())
                else:
                    raise AttributeError
            elif isinstance(arg, want):
                append(ctypes.byref(arg))
            else:
                raise AttributeError
    except AttributeError:  # raised above, or by something that is no tensor
        raise _refusal(name, plan, args, dev) from None
    if stream:
        if dev < 0 or not _gpu_checked:
            dev = require_gpu().index
        append(current_raw_stream(dev))
    if fn is None:
        fn = plan[4] = getattr(load(), name)
    try:
        code = fn(*out)
    except ctypes.ArgumentError as e:  # a scalar that ctypes could not convert; its text is "argument N: ..."
        number = re.match(r"argument (\d+):", str(e))
        at = int(number.group(1)) - 1 if number else len(args)
        if at < len(args):
            raise PvamdError(f"{name}: `{names[at]}` takes a {PARAMETERS[name][at][1]}, given {type(args[at]).__name__}") from None
        raise PvamdError(f"{name}: {e}") from None
    if code:
        check(code, name)


def as_query_points(points, device=None, keep_f64=False):
    """[..., 3] any float dtype / device  ->  (contiguous fp32 [P,3] on the GPU, leading shape, dtype, device).

    `device`: the GPU that owns the grid / mesh the points will be looked up in (the kernel dereferences raw pointers
    of that device, so the points and the launch must be there too); None = the current device.
    `keep_f64`: float64 points stay float64 (the grid lookups have float64 entry points; the mesh query computes in
    float32 like the reference, sdf.py:132)."""
    if not torch.is_tensor(points):
        points = torch.as_tensor(points)
    if points.shape[-1] != 3:
        raise ValueError(f"query points must have last dimension 3, got {tuple(points.shape)}")
    dev = require_gpu() if device is None else device
    lead = points.shape[:-1]
    flat = points.detach().reshape(-1, 3).to(device=dev, dtype=torch.float64 if keep_f64 and points.dtype == torch.float64
                                              else torch.float32).contiguous()
    return flat, lead, points.dtype if points.dtype.is_floating_point else torch.float32, points.device


_group_chunk = None
_mesh_small = None


def group_chunk_points():
    """Points per chunk of the chunk-grouped composed query (a build constant of the library)."""
    global _group_chunk
    if _group_chunk is None:
        _group_chunk = int(load().pvamd_group_chunk_points())
    return _group_chunk


def mesh_small_points():
    """The most points pvamd_mesh_query_unordered takes (a build constant of the library)."""
    global _mesh_small
    if _mesh_small is None:
        _mesh_small = int(load().pvamd_mesh_small_points())
    return _mesh_small


def whole_tiles(P):
    """P rounded up to whole tiles of TILE_POINTS: the Pp of pvamd_composed_query_bucketed and pvamd_composed_query_packed."""
    return -(-P // TILE_POINTS) * TILE_POINTS


def group_points(flat):
    """pvamd_group_points over contiguous fp32 (P, 3) GPU points: the scratch (uint8 tensor) pvamd_composed_query_grouped reads."""
    P = flat.shape[0]
    scratch = scratch_buffer(int(load().pvamd_group_scratch_bytes(P)), flat.device)
    call("pvamd_group_points", flat, P, scratch)
    return scratch


def morton_order(points, min_points=2048, want_inverse=False, want_sorted=False):
    """int32 permutation that walks fp32 [P,3] device points along a Hilbert curve (None below `min_points`, where
    ordering costs more than it saves).  Spatially coherent waves are what lets the mesh kernels skip far tiles and the
    bucketed composed kernel skip far leaves.  One C-ABI call (pvamd_morton_order -- the name is older than the curve: a
    seven-launch counting sort on the cells of the curve); nothing comes back to the host.  With want_inverse / want_sorted: (order, inverse, sorted points)."""
    P = points.shape[0]
    if P < min_points or P == 0:
        return (None, None, None) if (want_inverse or want_sorted) else None
    dev = points.device
    order = torch.empty((P,), dtype=torch.int32, device=dev)
    inv = torch.empty((P,), dtype=torch.int32, device=dev) if want_inverse else None
    spts = torch.empty((P, 3), dtype=torch.float32, device=dev) if want_sorted else None
    scratch = scratch_buffer(morton_order_scratch_bytes(P), dev)
    call("pvamd_morton_order", points, P, order, inv, spts, scratch)
    return (order, inv, spts) if (want_inverse or want_sorted) else order
