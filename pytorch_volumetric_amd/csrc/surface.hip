// Surface extraction (include/pvamd.h "Surface extraction"): an indexed triangle mesh of the level set of a sampled signed field by
// naive surface nets -- one vertex per cell the surface passes through, one quad per lattice edge with a crossing, no case table.
// Replaces nothing in the reference: its voxel.py stops at the containers.
//
// One lane per voxel in every pass, lanes along z: a voxel stands for itself (its sample), for the cell whose lowest corner it is,
// and for the three edges that leave it upward.  The neighbours a lane reads sit at the same offsets for neighbouring lanes, so
// every global access is a run of consecutive addresses.
//
// pvamd_surface_count, five launches:
//   classify   records, valid -> cls        one byte per voxel: usable | negative << 1
//   cells      cls -> act                   whether the voxel's cell is active (eight bytes of cls each, from L1/L2)
//   flags      cls, act -> flags            active | quad of family x, y, z << 1..3, and the sums of both per chunk of 256 voxels
//   scan       the chunk sums -> their exclusive prefix, in place; counts.  ONE workgroup of 1024, 1024 chunks a turn
//   ids        flags -> cell_id             the vertex id of the voxel's cell, -1 without one: chunk prefix + the waves before
//                                           + popcount of the lower lanes of a ballot
// pvamd_surface_emit, two launches, scratch read only:
//   vertices   cell_id, records -> vertices, normals     eight records per active cell, f recomputed per edge
//   faces      flags, cell_id, cls -> faces               the quad's first row by the same ballots; four ids gathered per quad
// Flat order everywhere, so ids and rows are those of the contract without an atomic: two calls give the same bits.
//
// Scratch, in this order (pvamd_surface_scratch_bytes = 7 n + 8 ceil(n / 256) bytes):
//   cell_id [n] int32, chunk_cells [chunks] int32, chunk_quads [chunks] int32, cls [n], act [n], flags [n] uint8
//
// hipcc -O3, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs / scratch bytes / LDS bytes per kernel
//   classify 8 / 0 / 0, cells 19 / 0 / 0, flags 20 / 0 / 32, scan 60 / 0 / 128, ids 16 / 0 / 16,
//   vertices 40 / 0 / 0 (with normals 62 / 0 / 0), faces 34 / 0 / 16
#include "common.h"
#include "exact_math.h"

namespace pvamd {

constexpr int kChunk = PVAMD_SURFACE_CHUNK;          // voxels per chunk: one workgroup
constexpr int kScanWidth = PVAMD_SURFACE_SCAN_WIDTH;  // chunk sums the scan takes per turn
constexpr int kChunkWaves = kChunk / 64, kScanWaves = kScanWidth / 64;
constexpr unsigned kUsable = 1, kNegative = 2;        // cls
constexpr unsigned kActive = 1;                       // flags; the quad of family k is bit 1 + k
static_assert(kChunk == 256, "the chunked kernels are launched with stream_grid(n, 256)");

struct SurfScratch {
    int *cell_id, *chunk_cells, *chunk_quads;
    uint8_t *cls, *act, *flags;
};

static inline int64_t surf_chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }

static inline SurfScratch surf_carve(void* scratch, int64_t n) {
    SurfScratch s;
    const int64_t chunks = surf_chunks(n);
    s.cell_id = (int*)scratch;
    s.chunk_cells = s.cell_id + n;
    s.chunk_quads = s.chunk_cells + chunks;
    s.cls = (uint8_t*)(s.chunk_quads + chunks);
    s.act = s.cls + n;
    s.flags = s.act + n;
    return s;
}

PVAMD_DEV uint64_t surf_lower_lanes() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// `mine`, a wave's total, summed over the waves before it in a workgroup of `waves` waves (sums: LDS, one int a wave); `total`: over
// all of them.  Every lane of the workgroup calls it.
PVAMD_DEV int surf_waves_before(int* sums, int waves, int mine, int& total) {
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // the readers of the previous turn are done with sums
    if ((threadIdx.x & 63) == 0) sums[wave] = mine;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < waves; ++w) {
        const int s = sums[w];
        if (w < wave) before += s;
        total += s;
    }
    return before;
}

// 1.
__global__ __launch_bounds__(256) void surf_classify_kernel(const f32x4* __restrict__ records, const uint8_t* __restrict__ valid,
                                                            float level, int64_t n, uint8_t* __restrict__ cls) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float w = sub_rn(records[i].x, level);
        const bool usable = sub_rn(w, w) == 0.0f && (!valid || valid[i] != 0);
        cls[i] = (uint8_t)(usable ? (kUsable | (w < 0.0f ? kNegative : 0u)) : 0u);
    }
}

// 3.
__global__ __launch_bounds__(256) void surf_cells_kernel(const uint8_t* __restrict__ cls, int64_t n, int nx, int ny, int nz,
                                                         uint8_t* __restrict__ act) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)ny * (unsigned)nz;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Voxel c = voxel_of((unsigned)i, plane, (unsigned)nz);
        unsigned active = 0;
        if ((int)c.x < nx - 1 && (int)c.y < ny - 1 && (int)c.z < nz - 1) {  // the cell exists: its far corner is i + plane + nz + 1 < n
            unsigned all = kUsable | kNegative, any = 0;
            for (int corner = 0; corner < 8; ++corner) {
                const unsigned v = cls[i + (corner & 4 ? plane : 0u) + (corner & 2 ? (unsigned)nz : 0u) + (corner & 1)];
                all &= v;
                any |= v;
            }
            active = (all & kUsable) && (any & kNegative) && !(all & kNegative);
        }
        act[i] = (uint8_t)active;
    }
}

// 7.: which of the three edges that leave voxel i upward emit a quad.  act[i] says that i's own cell (C2) is active, which puts
// every a_j at most n_j - 2 and makes the far ends of the three edges usable: such an edge carries a crossing iff the signs differ.
PVAMD_DEV unsigned surf_quads(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ act, int64_t i, const Voxel a, int64_t plane,
                              int64_t nz) {
    const unsigned ca = cls[i];
    const bool x = a.x >= 1, y = a.y >= 1, z = a.z >= 1;  // tested before any index is lowered
    unsigned f = 0;
    if (((ca ^ cls[i + plane]) & kNegative) && y && z && act[i - nz] && act[i - 1] && act[i - nz - 1]) f |= 2u;
    if (((ca ^ cls[i + nz]) & kNegative) && z && x && act[i - 1] && act[i - plane] && act[i - 1 - plane]) f |= 4u;
    if (((ca ^ cls[i + 1]) & kNegative) && x && y && act[i - plane] && act[i - nz] && act[i - plane - nz]) f |= 8u;
    return f;
}

__global__ __launch_bounds__(kChunk) void surf_flags_kernel(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ act, int64_t n,
                                                            int ny, int nz, uint8_t* __restrict__ flags,
                                                            int* __restrict__ chunk_cells, int* __restrict__ chunk_quads) {
    __shared__ int cells_of[kChunkWaves], quads_of[kChunkWaves];
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    const unsigned plane = (unsigned)ny * (unsigned)nz;
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int64_t i = chunk * kChunk + threadIdx.x;
        unsigned f = 0;
        if (i < n && act[i]) f = kActive | surf_quads(cls, act, i, voxel_of((unsigned)i, plane, (unsigned)nz), (int64_t)plane, (int64_t)nz);
        if (i < n) flags[i] = (uint8_t)f;
        const int cells = __popcll(__ballot(f & kActive));
        const int quads = __popcll(__ballot(f & 2u)) + __popcll(__ballot(f & 4u)) + __popcll(__ballot(f & 8u));
        int all_cells, all_quads;
        surf_waves_before(cells_of, kChunkWaves, cells, all_cells);
        surf_waves_before(quads_of, kChunkWaves, quads, all_quads);
        if (threadIdx.x == 0) {
            chunk_cells[chunk] = all_cells;
            chunk_quads[chunk] = all_quads;
        }
    }
}

// the chunk sums to their exclusive prefix, in place, and the totals: one workgroup, kScanWidth chunks a turn with a running carry
__global__ __launch_bounds__(kScanWidth) void surf_scan_kernel(int* __restrict__ chunk_cells, int* __restrict__ chunk_quads,
                                                               int64_t chunks, int64_t* __restrict__ counts) {
    __shared__ int cells_of[kScanWaves], quads_of[kScanWaves];
    const int lane = threadIdx.x & 63;
    int carry_cells = 0, carry_quads = 0;  // the same in every lane
    for (int64_t first = 0; first < chunks; first += kScanWidth) {
        const int64_t j = first + threadIdx.x;
        const int c = j < chunks ? chunk_cells[j] : 0, q = j < chunks ? chunk_quads[j] : 0;
        int upto_c = c, upto_q = q;  // inclusive within the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int uc = __shfl_up(upto_c, d), uq = __shfl_up(upto_q, d);
            if (lane >= d) {
                upto_c += uc;
                upto_q += uq;
            }
        }
        const int wave_c = __shfl(upto_c, 63), wave_q = __shfl(upto_q, 63);
        int all_c, all_q;
        const int before_c = surf_waves_before(cells_of, kScanWaves, wave_c, all_c);
        const int before_q = surf_waves_before(quads_of, kScanWaves, wave_q, all_q);
        if (j < chunks) {
            chunk_cells[j] = carry_cells + before_c + (upto_c - c);
            chunk_quads[j] = carry_quads + before_q + (upto_q - q);
        }
        carry_cells += all_c;
        carry_quads += all_q;
    }
    if (threadIdx.x == 0) {
        counts[0] = carry_cells;
        counts[1] = 2 * (int64_t)carry_quads;
    }
}

// 6.
__global__ __launch_bounds__(kChunk) void surf_ids_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ chunk_cells,
                                                          int64_t n, int* __restrict__ cell_id) {
    __shared__ int cells_of[kChunkWaves];
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int64_t i = chunk * kChunk + threadIdx.x;
        const bool active = i < n && (flags[i] & kActive);
        const uint64_t actives = __ballot(active);
        int all;
        const int before = surf_waves_before(cells_of, kChunkWaves, __popcll(actives), all);
        if (i < n) cell_id[i] = active ? chunk_cells[chunk] + before + __popcll(actives & surf_lower_lanes()) : -1;
    }
}

// 4. and 5.  Corner (dx, dy, dz) of the cell is number dx * 4 + dy * 2 + dz; every index below is a constant once unrolled.
template <bool kNormals>
__global__ __launch_bounds__(256) void surf_vertices_kernel(const Lattice L, const f32x4* __restrict__ records, float level,
                                                            const int* __restrict__ cell_id, int64_t n, int64_t max_vertices,
                                                            float* __restrict__ vertices, float* __restrict__ normals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)L.n[1] * (unsigned)L.n[2], nz = (unsigned)L.n[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int id = cell_id[i];
        if (id < 0 || id >= max_vertices) continue;
        const Voxel cell = voxel_of((unsigned)i, plane, nz);
        float W[8], G[8][3];
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {  // an active cell: the far corner is i + plane + nz + 1 < n
            const int64_t j = i + (corner & 4 ? plane : 0u) + (corner & 2 ? nz : 0u) + (corner & 1);
            if (kNormals) {
                const f32x4 r = records[j];
                W[corner] = sub_rn(r.x, level);
                G[corner][0] = r.y;
                G[corner][1] = r.z;
                G[corner][2] = r.w;
            } else {
                W[corner] = sub_rn(records[j].x, level);
            }
        }
        float S[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f};
        int m = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int o0 = k == 0 ? 1 : 0, o1 = k == 2 ? 1 : 2;  // the other two axes, ascending
#pragma unroll
            for (int d0 = 0; d0 < 2; ++d0) {
#pragma unroll
                for (int d1 = 0; d1 < 2; ++d1) {
                    const int ia = d0 * (4 >> o0) + d1 * (4 >> o1), ib = ia + (4 >> k);
                    const float wa = W[ia], wb = W[ib];
                    if ((wa < 0.0f) == (wb < 0.0f)) continue;  // all eight corners are usable
                    const float f = div_rn(wa, sub_rn(wa, wb));
                    float offset[3];
                    offset[k] = f;
                    offset[o0] = (float)d0;
                    offset[o1] = (float)d1;
#pragma unroll
                    for (int j = 0; j < 3; ++j) S[j] = add_rn(S[j], offset[j]);
                    ++m;
                    if (kNormals) {
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            N[j] = add_rn(N[j], add_rn(G[ia][j], mul_rn(f, sub_rn(G[ib][j], G[ia][j]))));
                    }
                }
            }
        }
        const float at[3] = {(float)cell.x, (float)cell.y, (float)cell.z};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float p = add_rn(at[j], div_rn(S[j], (float)m));
            vertices[(int64_t)id * 3 + j] = add_rn(L.fmin[j], mul_rn(p, L.fres[j]));
        }
        if (kNormals) {
            const float len = sqrt_rn(add_rn(add_rn(mul_rn(N[0], N[0]), mul_rn(N[1], N[1])), mul_rn(N[2], N[2])));
            const bool ok = len > 0.0f && len < __builtin_inff();
#pragma unroll
            for (int j = 0; j < 3; ++j) normals[(int64_t)id * 3 + j] = ok ? div_rn(N[j], len) : 0.0f;
        }
    }
}

// 7.
__global__ __launch_bounds__(kChunk) void surf_faces_kernel(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ flags,
                                                            const int* __restrict__ cell_id, const int* __restrict__ chunk_quads,
                                                            int64_t n, int ny, int nz, int64_t max_faces, int* __restrict__ faces) {
    __shared__ int quads_of[kChunkWaves];
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    const int64_t step[3] = {(int64_t)ny * nz, (int64_t)nz, 1};
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int64_t i = chunk * kChunk + threadIdx.x;
        const unsigned f = i < n ? flags[i] : 0u;
        const uint64_t bx = __ballot(f & 2u), by = __ballot(f & 4u), bz = __ballot(f & 8u), lower = surf_lower_lanes();
        int all;
        const int before = surf_waves_before(quads_of, kChunkWaves, __popcll(bx) + __popcll(by) + __popcll(bz), all);
        if (!(f & 14u)) continue;  // after the workgroup's barriers; the loop's trip count is the workgroup's
        int64_t row = 2 * (int64_t)(chunk_quads[chunk] + before + __popcll(bx & lower) + __popcll(by & lower) + __popcll(bz & lower));
        const bool negative = cls[i] & kNegative;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(f & (2u << k))) continue;
            const int64_t sp = step[(k + 1) % 3], sq = step[(k + 2) % 3];  // the quad exists: i - sp - sq >= 0
            const int v0 = cell_id[i - sp - sq], v2 = cell_id[i];
            const int c1 = cell_id[i - sq], c3 = cell_id[i - sp];
            const int v1 = negative ? c1 : c3, v3 = negative ? c3 : c1;
            if (row < max_faces) {
                faces[row * 3 + 0] = v0;
                faces[row * 3 + 1] = v1;
                faces[row * 3 + 2] = v2;
            }
            if (row + 1 < max_faces) {
                faces[row * 3 + 3] = v0;
                faces[row * 3 + 4] = v2;
                faces[row * 3 + 5] = v3;
            }
            row += 2;
        }
    }
}

// the checks the two entry points share, in the header's order up to the level
static int surf_check(const pvamd_grid_t* grid, float level) {
    if (!grid) return PVAMD_E_NULL;
    if (!lattice_shape_ok(grid->shape[0], grid->shape[1], grid->shape[2], PVAMD_SURFACE_MIN_AXIS, PVAMD_SURFACE_MAX_VOXELS))
        return PVAMD_E_SHAPE;
    if (int e = check_grid(*grid, /*need_vox=*/false)) return e;
    if (!(level - level == 0.0f)) return PVAMD_E_MODE;  // NaN, +/-inf
    return 0;
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_surface_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!lattice_shape_ok(nx, ny, nz, PVAMD_SURFACE_MIN_AXIS, PVAMD_SURFACE_MAX_VOXELS)) return 0;
    const int64_t n = (int64_t)nx * ny * nz;
    return 7 * n + 8 * surf_chunks(n);
}

extern "C" int pvamd_surface_count(const pvamd_grid_t* grid, const float* records, const uint8_t* valid, float level, void* scratch,
                                   int64_t* counts, void* stream) {
    if (int e = surf_check(grid, level)) return e;
    if (!records || !scratch || !counts) return PVAMD_E_NULL;
    if (!aligned_to(records, 16) || !aligned_to(counts, 8) || !aligned_to(scratch, 4)) return PVAMD_E_ALIGN;
    const Lattice L = lattice_of(*grid);
    const int64_t n = (int64_t)L.n[0] * L.n[1] * L.n[2];
    const SurfScratch s = surf_carve(scratch, n);
    hipStream_t q = (hipStream_t)stream;
    const dim3 grid_dim(stream_grid(n, 256)), block(256);
    hipLaunchKernelGGL(surf_classify_kernel, grid_dim, block, 0, q, reinterpret_cast<const f32x4*>(records), valid, level, n, s.cls);
    hipLaunchKernelGGL(surf_cells_kernel, grid_dim, block, 0, q, s.cls, n, L.n[0], L.n[1], L.n[2], s.act);
    hipLaunchKernelGGL(surf_flags_kernel, grid_dim, block, 0, q, s.cls, s.act, n, L.n[1], L.n[2], s.flags, s.chunk_cells, s.chunk_quads);
    hipLaunchKernelGGL(surf_scan_kernel, dim3(1), dim3(kScanWidth), 0, q, s.chunk_cells, s.chunk_quads, surf_chunks(n), counts);
    hipLaunchKernelGGL(surf_ids_kernel, grid_dim, block, 0, q, s.flags, s.chunk_cells, n, s.cell_id);
    return (int)hipGetLastError();
}

extern "C" int pvamd_surface_emit(const pvamd_grid_t* grid, const float* records, const uint8_t* valid, float level,
                                  const void* scratch, int64_t max_vertices, int64_t max_faces, float* vertices, float* normals,
                                  int32_t* faces, void* stream) {
    (void)valid;  // the classes count left in scratch already hold it
    if (!grid) return PVAMD_E_NULL;
    if (max_vertices < 0 || max_faces < 0) return PVAMD_E_SHAPE;
    if (int e = surf_check(grid, level)) return e;
    if (!records || !scratch || (max_vertices > 0 && !vertices) || (max_faces > 0 && !faces)) return PVAMD_E_NULL;
    if (!aligned_to(records, 16) || !aligned_to(scratch, 4) || !aligned_to(vertices, 4) || !aligned_to(normals, 4) ||
        !aligned_to(faces, 4))
        return PVAMD_E_ALIGN;
    const Lattice L = lattice_of(*grid);
    const int64_t n = (int64_t)L.n[0] * L.n[1] * L.n[2];
    const SurfScratch s = surf_carve(const_cast<void*>(scratch), n);
    hipStream_t q = (hipStream_t)stream;
    const dim3 grid_dim(stream_grid(n, 256)), block(256);
    const f32x4* rec = reinterpret_cast<const f32x4*>(records);
    if (max_vertices > 0) {
        if (normals)
            hipLaunchKernelGGL(surf_vertices_kernel<true>, grid_dim, block, 0, q, L, rec, level, s.cell_id, n, max_vertices, vertices,
                               normals);
        else
            hipLaunchKernelGGL(surf_vertices_kernel<false>, grid_dim, block, 0, q, L, rec, level, s.cell_id, n, max_vertices, vertices,
                               normals);
    }
    if (max_faces > 0)
        hipLaunchKernelGGL(surf_faces_kernel, grid_dim, block, 0, q, s.cls, s.flags, s.cell_id, s.chunk_quads, n, L.n[1], L.n[2],
                           max_faces, faces);
    return (int)hipGetLastError();
}
