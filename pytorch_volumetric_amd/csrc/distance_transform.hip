// Exact Euclidean distance transform of a voxel occupancy grid, fused with the SDF statements that turn it into the packed
// (val, gx, gy, gz) records a CachedSDF keeps (include/pvamd.h "Distance transform").  Replaces nothing in the reference: its
// VoxelGrid holds observed occupancy (voxel.py:42-103) and nothing turns that into a distance field.
//
// Three separable line passes, z then y then x, one lane per voxel in every pass, lanes along z so that every global access
// is a run of consecutive addresses.  A site class (the occupied voxels; in signed mode also the free ones) keeps ONE int32 per
// voxel between the passes -- the coordinates of the best site so far along the axes already done, or -1 when there is none:
//   after z: z' of the nearest site on the voxel's own z line                      (cost (z - z')^2)
//   after y: (y' << kAxisBits) | z' of the nearest site in the voxel's own x plane (cost (y - y')^2 + (z - z')^2)
// and the x pass writes the flat site, the squared distance and the record.  The cost is recomputed from the coordinates where
// it is compared: a candidate visit is one 4-byte load.  No sum ever includes the no-site sentinel: a candidate without a site
// is skipped.
//
// Tie rule (part of the contract): the site with the smallest flat C-order index wins an equal cost.  Flat order is
// lexicographic in (x', y', z'), so it is enough that every line minimum prefers the smaller coordinate along its own axis.
//   z pass: the line's occupancy is staged in LDS as a bit set, one 64-bit word per 64 voxels (a wave ballot); the nearest site
//           at or below z and at or above z are each one masked clz / ctz, walking whole words only across runs of 64 voxels
//           without a site.  The lower one wins an equal distance.
//   y, x passes: an outward scan from the voxel's own coordinate c: at offset d first c - d (smaller than every coordinate seen
//           so far: wins with cost <= best), then c + d (larger than all: wins with cost < best only).  A candidate at offset d
//           costs at least d^2, so the scan ends once d^2 > best -- not at d^2 == best, where a site at c - d with no cost of
//           its own still ties and, being the smaller coordinate, wins.  A line without any site is scanned to both ends.
// All of it is int32: the largest squared distance is 3 * 2047^2 < 2^24.  No atomics, no host synchronisation, no allocation.
#include "common.h"
#include "exact_math.h"

namespace pvamd {

constexpr int kEdtWords = PVAMD_LATTICE_MAX_AXIS / 64;  // bit-set words of one z line
constexpr int kEdtWaves = 4;                            // z pass: waves (= lines in flight) per workgroup

// nearest set bit of the line's bit set to position z (word w = z / 64, bit b = z % 64), the lower one on equal distance; -1: none
__device__ __forceinline__ int edt_nearest_bit(const unsigned long long* words, int nw, int w, int b, bool invert,
                                               unsigned long long last_valid) {
    auto word = [&](int k) {
        const unsigned long long v = words[k];
        return invert ? (~v & (k == nw - 1 ? last_valid : ~0ull)) : v;
    };
    int lo = -1, hi = -1;
    unsigned long long m = word(w) & ((2ull << b) - 1ull);  // bits 0..b (b = 63: 2 << 63 wraps to 0, minus one is all ones)
    for (int k = w; ; m = word(--k)) {
        if (m) { lo = k * 64 + 63 - __builtin_clzll(m); break; }
        if (k == 0) break;
    }
    m = word(w) & (~0ull << b);  // bits b..63
    for (int k = w; ; m = word(++k)) {
        if (m) { hi = k * 64 + __builtin_ctzll(m); break; }
        if (k == nw - 1) break;
    }
    const int z = w * 64 + b;
    if (lo < 0) return hi;
    if (hi < 0) return lo;
    return (z - lo) <= (hi - z) ? lo : hi;
}

// Pass 1.  One wave per z line, grid-stride over the nx * ny lines.  state0: nearest occupied z' per voxel; state1 (signed):
// nearest free z'.
template <bool SIGNED>
__global__ __launch_bounds__(kEdtWaves * 64) void edt_z_kernel(const uint8_t* __restrict__ occ, int64_t lines, int nz,
                                                               int* __restrict__ state0, int* __restrict__ state1) {
    __shared__ unsigned long long bits[kEdtWaves][kEdtWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* words = bits[wave];
    const int nw = (nz + 63) >> 6;
    const int tail = nz & 63;
    const unsigned long long last_valid = tail ? ((1ull << tail) - 1ull) : ~0ull;
    for (int64_t line = (int64_t)blockIdx.x * kEdtWaves + wave; line < lines; line += (int64_t)gridDim.x * kEdtWaves) {
        const int64_t base = line * nz;
        for (int w = 0; w < nw; ++w) {
            const int z = w * 64 + lane;
            const bool set = z < nz && occ[base + z] != 0;
            const unsigned long long b = __ballot(set);
            if (lane == 0) words[w] = b;
        }
        PVAMD_WAVE_SYNC();
        for (int w = 0; w < nw; ++w) {
            const int z = w * 64 + lane;
            if (z < nz) {
                state0[base + z] = edt_nearest_bit(words, nw, w, lane, false, last_valid);
                if (SIGNED) state1[base + z] = edt_nearest_bit(words, nw, w, lane, true, last_valid);
            }
        }
        PVAMD_WAVE_SYNC();  // the next line's words are written only after every lane has read this line's
    }
}

// One outward scan along a line of `len` candidates around position c.  cost_of(k, cost) reads candidate k and returns whether it
// has a site, with its cost so far (without the term of this axis).  Returns the winning position, -1 when the line has no site.
template <typename CostOf>
__device__ __forceinline__ int edt_scan(int c, int len, int& best, CostOf cost_of) {
    int at = -1;
    best = PVAMD_EDT_NO_SITE;
    for (int d = 0; d < len; ++d) {
        const int dd = d * d;
        if (dd > best) break;
        const int lo = c - d, hi = c + d;
        if (lo < 0 && hi >= len) break;
        int cost;
        if (lo >= 0 && cost_of(lo, cost) && cost + dd <= best) { best = cost + dd; at = lo; }
        if (d > 0 && hi < len && cost_of(hi, cost) && cost + dd < best) { best = cost + dd; at = hi; }
    }
    return at;
}

// Pass 2.  in: z' per voxel; out: (y' << kAxisBits) | z' per voxel.  Both classes of a signed call in one launch.
template <bool SIGNED>
__global__ __launch_bounds__(256) void edt_y_kernel(int64_t n, int ny, int nz, const int* __restrict__ in0, const int* __restrict__ in1,
                                                    int* __restrict__ out0, int* __restrict__ out1) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)ny * (unsigned)nz;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Voxel v = voxel_of((unsigned)i, plane, (unsigned)nz);
        const int y = (int)v.y, z = (int)v.z;
        const int64_t column = (int64_t)v.x * plane + z;  // + y' * nz: the candidates of this voxel
        for (int cls = 0; cls < (SIGNED ? 2 : 1); ++cls) {
            const int* __restrict__ in = cls ? in1 : in0;
            int best, zs = -1;
            const int at = edt_scan(y, ny, best, [&](int k, int& cost) {
                const int s = in[column + (int64_t)k * nz];
                if (s < 0) return false;
                cost = (z - s) * (z - s);
                return true;
            });
            if (at >= 0) zs = in[column + (int64_t)at * nz];
            (cls ? out1 : out0)[i] = at < 0 ? -1 : ((at << kAxisBits) | zs);
        }
    }
}

// Pass 3, fused with the value and gradient statements of the contract.  A voxel scans the one class it is measured against:
// the occupied sites, or for an occupied voxel of a signed call the free ones.
template <bool SIGNED>
__global__ __launch_bounds__(256) void edt_x_kernel(const uint8_t* __restrict__ occ, int64_t n, int nx, int ny, int nz,
                                                    const int* __restrict__ in0, const int* __restrict__ in1, float r,
                                                    f32x4* __restrict__ records, int* __restrict__ sites, int* __restrict__ squared) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)ny * (unsigned)nz;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Voxel v = voxel_of((unsigned)i, plane, (unsigned)nz);
        const unsigned rem = v.rest;
        const int x = (int)v.x, y = (int)v.y, z = (int)v.z;
        const bool occupied = occ[i] != 0;
        const int* __restrict__ in = (SIGNED && occupied) ? in1 : in0;
        int best;
        const int at = edt_scan(x, nx, best, [&](int k, int& cost) {
            const int s = in[(int64_t)k * plane + rem];
            if (s < 0) return false;
            const int dy = y - (s >> kAxisBits), dz = z - (s & kAxisMask);
            cost = dy * dy + dz * dz;
            return true;
        });
        const float inf = __builtin_inff();
        f32x4 rec = {occupied ? -inf : inf, 0.0f, 0.0f, 0.0f};
        int site = -1;
        if (at >= 0) {
            const int s = in[(int64_t)at * plane + rem];
            const int sy = s >> kAxisBits, sz = s & kAxisMask;
            site = (int)(((unsigned)at * (unsigned)ny + (unsigned)sy) * (unsigned)nz + (unsigned)sz);
            const float root = sqrt_rn((float)best);
            // toward increasing value: away from the site for a free voxel, toward it for an occupied one
            const int ex = occupied ? at - x : x - at, ey = occupied ? sy - y : y - sy, ez = occupied ? sz - z : z - sz;
            if (SIGNED) {
                const float v = mul_rn(r, sub_rn(root, 0.5f));
                rec.x = occupied ? -v : v;
            } else {
                rec.x = mul_rn(r, root);  // an occupied voxel is its own site: +0.0
            }
            if (best > 0) {
                rec.y = div_rn((float)ex, root);
                rec.z = div_rn((float)ey, root);
                rec.w = div_rn((float)ez, root);
            }
        }
        records[i] = rec;
        if (sites) sites[i] = site;
        if (squared) squared[i] = best;
    }
}

template <bool SIGNED>
static int edt_launch(const uint8_t* occ, int nx, int ny, int nz, float r, float* records, int32_t* sites, int32_t* squared,
                      int* scratch, hipStream_t s) {
    const int64_t n = (int64_t)nx * ny * nz, lines = (int64_t)nx * ny;
    // per class: the z pass's state, then the y pass's
    int* z0 = scratch;
    int* y0 = scratch + n;
    int* z1 = SIGNED ? scratch + 2 * n : nullptr;
    int* y1 = SIGNED ? scratch + 3 * n : nullptr;
    const int64_t zblocks = (lines + kEdtWaves - 1) / kEdtWaves;
    const int64_t cap = (int64_t)kNumCU * kMaxBlocksPerCU;
    hipLaunchKernelGGL((edt_z_kernel<SIGNED>), dim3((unsigned)(zblocks < cap ? zblocks : cap)), dim3(kEdtWaves * 64), 0, s, occ, lines,
                       nz, z0, z1);
    const dim3 gd(stream_grid(n, 256)), block(256);
    hipLaunchKernelGGL((edt_y_kernel<SIGNED>), gd, block, 0, s, n, ny, nz, z0, z1, y0, y1);
    hipLaunchKernelGGL((edt_x_kernel<SIGNED>), gd, block, 0, s, occ, n, nx, ny, nz, y0, y1, r, reinterpret_cast<f32x4*>(records), sites,
                       squared);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_distance_transform_scratch_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t is_signed) {
    if (!lattice_shape_ok(nx, ny, nz, PVAMD_EDT_MIN_AXIS, PVAMD_EDT_MAX_VOXELS) || (is_signed != 0 && is_signed != 1)) return 0;
    return (int64_t)nx * ny * nz * (is_signed ? 4 : 2) * (int64_t)sizeof(int32_t);
}

extern "C" int pvamd_distance_transform(const uint8_t* occupied, int32_t nx, int32_t ny, int32_t nz, float resolution,
                                        int32_t is_signed, float* records, int32_t* sites, int32_t* squared, void* scratch,
                                        void* stream) {
    if (!lattice_shape_ok(nx, ny, nz, PVAMD_EDT_MIN_AXIS, PVAMD_EDT_MAX_VOXELS)) return PVAMD_E_SHAPE;
    if (is_signed != 0 && is_signed != 1) return PVAMD_E_MODE;
    if (!occupied || !records || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(records, 16) || !aligned_to(scratch, 4) || !aligned_to(sites, 4) || !aligned_to(squared, 4)) return PVAMD_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    return is_signed ? edt_launch<true>(occupied, nx, ny, nz, resolution, records, sites, squared, (int*)scratch, s)
                     : edt_launch<false>(occupied, nx, ny, nz, resolution, records, sites, squared, (int*)scratch, s);
}
