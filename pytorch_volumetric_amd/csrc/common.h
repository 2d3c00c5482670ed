// Host-side helpers shared by the C-ABI translation units.  gfx950 (MI355X) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pvamd.h"

// A/B builds (tools/build_variant.sh compiles ONE edited or patched translation unit with -DPVAMD_VARIANT="name: flags") carry
// their name in the library: _lib.load() refuses a library that exports pvamd_variant unless PVAMD_ALLOW_VARIANT=1 is set, so a
// tuning build cannot be picked up by the product path or the tests by accident.  The product build never defines it.
#ifdef PVAMD_VARIANT
extern "C" __attribute__((visibility("default"), weak)) const char* pvamd_variant(void) { return PVAMD_VARIANT; }
#endif

namespace pvamd {

// native clang vectors: the non-temporal builtins and 16-B global_load/store_dwordx4 want these, not HIP's structs
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// same 16-byte vector, but allowed to alias plain float storage (LDS slices accessed both as floats and as float4s)
typedef f32x4 __attribute__((may_alias)) f32x4_alias;
// the same 16 bytes at an address that is only 4-byte aligned: gfx950 global_load/store_dwordx4 take any dword address
// (amdhsa runs with unaligned access mode on), so an (A, P) output row that starts at a * P floats with P odd still
// leaves as 16-byte stores -- the compiler emits the same instruction as for f32x4
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));

// Wave-synchronous LDS exchange: lanes of ONE wave hand data to each other through LDS without a block barrier.  The
// hardware executes a wave's DS instructions in order, but the compiler reasons per thread and will move a lane's
// LDS store past loads that (for that lane) cannot alias -- seen in the ISA of the first version of cached_query_wave.
// A wavefront-scope release/acquire fence pair around a wave_barrier pins the order; it emits no s_barrier.
#define PVAMD_WAVE_SYNC()                                         \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

constexpr int kNumCU = 256;         // MI355X: 8 XCDs x 32 CUs
constexpr int kMaxBlocksPerCU = 8;  // memory-bound kernels: cap the grid at 256 CU x 8 and grid-stride the rest
constexpr int kMaxGridRows = 65535; // gridDim.y and gridDim.z of a HIP launch hold no more

static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// gridDim.y (or .z) of a kernel that wraps its row (a += gridDim.y): n, at least 1 and at most kMaxGridRows
static inline unsigned grid_rows(int64_t n) { return (unsigned)(n < 1 ? 1 : (n < kMaxGridRows ? n : kMaxGridRows)); }

// fn(first, count) for consecutive slabs of at most kMaxGridRows rows that cover [0, rows): the launches of a kernel that takes
// its row from blockIdx.y and does not wrap.  Counted in 64 bits: rows near INT32_MAX do not overflow.
template <typename F>
static inline void for_row_slabs(int32_t rows, F fn) {
    for (int64_t first = 0; first < rows; first += kMaxGridRows)
        fn((int32_t)first, (int32_t)(rows - first < kMaxGridRows ? rows - first : kMaxGridRows));
}

// grid size for a streaming kernel over n items with `block` threads
static inline unsigned stream_grid(int64_t n, int block) {
    const int64_t need = (n + block - 1) / block;
    const int64_t cap = (int64_t)kNumCU * kMaxBlocksPerCU;
    return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}

// gridDim.y of a kernel that takes the configuration as blockIdx.x (any count: one launch for any A) and grid-strides over
// `need` rows of work per configuration in y: up to ~65536 blocks in total, split over the A configurations (about one
// 256-point tile per wave in the composed query), at least 1 and at most kMaxGridRows.  (Sweep on C4, 200 x 262,144:
// 1024 blocks 1.40 ms, 4096 1.17, 8192 1.13, 32768 1.09, 65536 1.08 -- the hardware dispatcher balances better than a
// grid-stride loop over unequal tiles.)
static inline unsigned config_rows(int32_t A, int64_t need) {
    const int64_t cap = ((int64_t)65536 + A - 1) / A;
    return grid_rows(need < cap ? need : cap);
}

static inline int check_grid(const pvamd_grid_t& g, bool need_vox = true) {
    if (need_vox && !g.vox) return PVAMD_E_NULL;
    if (need_vox && !aligned_to(g.vox, 16)) return PVAMD_E_ALIGN;
    for (int d = 0; d < 3; ++d) {
        if (g.shape[d] < 2) return PVAMD_E_SHAPE;
    }
    if ((int64_t)g.shape[0] * g.shape[1] * g.shape[2] > (int64_t)INT32_MAX) return PVAMD_E_SHAPE;
    if (g.oob_mode != PVAMD_OOB_LOOKUP_GT_SDF && g.oob_mode != PVAMD_OOB_BOUNDING_BOX) return PVAMD_E_MODE;
    if (!g.finalized) return PVAMD_E_MODE;  // pvamd_grid_finalize() was not called
    return 0;
}

// ---- The lattice of the volume entry points (include/pvamd.h "Volume lattices"): distance transform, ray integration, TSDF,
// redistancing.
#define PVAMD_DEV __device__ __forceinline__

// a coordinate in the packed states the line passes hand on: (high << kAxisBits) | low, low = packed & kAxisMask
constexpr int kAxisBits = 11;
constexpr int kAxisMask = (1 << kAxisBits) - 1;
static_assert(PVAMD_LATTICE_MAX_AXIS <= (1 << kAxisBits), "a lattice coordinate must fit kAxisBits");

// every axis in [min_axis, PVAMD_LATTICE_MAX_AXIS] and at most `cap` voxels
static inline bool lattice_shape_ok(int32_t nx, int32_t ny, int32_t nz, int min_axis, int64_t cap) {
    if (nx < min_axis || ny < min_axis || nz < min_axis) return false;
    if (nx > PVAMD_LATTICE_MAX_AXIS || ny > PVAMD_LATTICE_MAX_AXIS || nz > PVAMD_LATTICE_MAX_AXIS) return false;
    return (int64_t)nx * ny * nz <= cap;
}

// what a kernel reads of a descriptor's lattice: the float32 fields, whatever index_f64 says
struct Lattice {
    float fmin[3], fres[3];
    int n[3];
};

static inline Lattice lattice_of(const pvamd_grid_t& g) {
    Lattice L;
    for (int k = 0; k < 3; ++k) {
        L.fmin[k] = g.fmin[k];
        L.fres[k] = g.fres[k];
        L.n[k] = g.shape[k];
    }
    return L;
}

// voxel (x, y, z) of a flat C-order index; rest = y * nz + z, the index inside the x plane (plane = ny * nz)
struct Voxel {
    unsigned x, y, z, rest;
};

PVAMD_DEV Voxel voxel_of(unsigned flat, unsigned plane, unsigned nz) {
    const unsigned x = flat / plane, rest = flat - x * plane;
    const unsigned y = rest / nz, z = rest - y * nz;
    return {x, y, z, rest};
}

}  // namespace pvamd
