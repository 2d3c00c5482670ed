// Redistancing (include/pvamd.h "Redistancing"): the exact Euclidean distance from every voxel to the zero set of a sampled signed
// field, the zero set taken at sub-voxel precision as the sign changes along the lattice edges ("ESDF from TSDF").  Replaces
// nothing in the reference: its voxel.py stops at the containers.
//
// A crossing of family k sits on an edge along axis k; its cost to a voxel is ((t^2 + d_p2^2) + d_p3^2) with p2 > p3 the other
// axes, so a family is three separable line passes -- along k over the edges, then along p2 and p3 over the voxels' states --
// in the manner of distance_transform.hip, with float costs:
//   family x: passes x, z, y     family y: passes y, z, x     family z: passes z, y, x
// One lane per voxel in every pass, lanes along z.  A scan along x or y reads, per step, the same offset of neighbouring z
// columns; a scan along z reads its own z + d, again neighbouring addresses for neighbouring lanes: every global access of every
// pass is a run of consecutive addresses, 4 or 8 bytes a lane.
//
// State between the passes: 8 bytes per voxel, (float cost, int32 packed).  packed is -1 without a site (cost +inf), else
//   after pass 1: a_k                       the edge's lower voxel along k        cost c1
//   after pass 2: a_k | (a_p2 << kAxisBits)                                       cost c2
// and the last pass of all three families is one kernel, which takes the best family (lowest k on a tie) and writes the records,
// sites and squared.  f, and with it t and the gradient, is recomputed there from the two samples of the winning edge.
//
// Scratch, in this order (pvamd_redistance_scratch_bytes = 36 n bytes, n = nx ny nz):
//   V  [n] float32      the val column of records_in, so that the edge pass reads 4 contiguous bytes a lane, not 4 of every 16
//   A  [n][2]           pass 1 of the family in hand, overwritten by the next family
//   Bx, By, Bz [n][2]   pass 2 of each family, read by the last kernel
// Eight launches: values; (edges, lines) for z, y, x; last.
//
// Scans are outward from the voxel's own coordinate, as edt_scan: a candidate at step d costs at least (float)(d * d), so the
// scan ends once that exceeds min(best, R2); at equal cost the candidate below wins (tested first, with <=), the one above only
// with <.  In space without crossings a scan runs to both ends of its line: max_distance is what bounds it.
// No LDS, no atomics, no allocation, no host synchronisation.
#include "common.h"
#include "exact_math.h"

namespace pvamd {

// the 8-byte state at an address that is only 4-byte aligned (the scratch's contract; gfx950 takes any dword address)
typedef float state2 __attribute__((ext_vector_type(2), aligned(4)));

PVAMD_DEV bool redist_finite(float a) { return sub_rn(a, a) == 0.0f; }

// whether the edge with samples (va, vb) carries a crossing, and where along it
PVAMD_DEV bool redist_crossing(float va, float vb, float& f) {
    if (!redist_finite(va) || !redist_finite(vb) || (va < 0.0f) == (vb < 0.0f)) return false;
    f = div_rn(va, sub_rn(va, vb));
    return true;
}

PVAMD_DEV state2 redist_state(float cost, int packed) {
    state2 s;
    s.x = cost;
    s.y = __int_as_float(packed);
    return s;
}

__global__ __launch_bounds__(256) void redist_values_kernel(const f32x4* __restrict__ records_in, int64_t n, float* __restrict__ V) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) V[i] = records_in[i].x;
}

// the coordinate of flat voxel i along `axis`.  voxel_of's statements written out: from locals the compiler divides by nz only
// where axis != 0, from voxel_of's result it divides everywhere (profiles/volume_lattice.md)
PVAMD_DEV int redist_coordinate(unsigned flat, unsigned ny, unsigned nz, int axis) {
    const unsigned plane = ny * nz;
    const unsigned x = flat / plane, rest = flat - x * plane;
    const unsigned y = rest / nz, z = rest - y * nz;
    return (int)(axis == 0 ? x : (axis == 1 ? y : z));
}

// Pass 1 of a family: per voxel the crossing of its own line along `axis` (len voxels, `step` flat indices apart) with the
// smallest c1.  Step d visits the edges c - 1 - d (t in [d, d + 1]) and c + d (t in [-d - 1, -d]); a sample is loaded once and
// handed from one edge to the next.
__global__ __launch_bounds__(256) void redist_edge_kernel(const float* __restrict__ V, int64_t n, int ny, int nz, int axis, int len,
                                                          int64_t step, float R2, state2* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c = redist_coordinate((unsigned)i, (unsigned)ny, (unsigned)nz, axis);
        const float* __restrict__ line = V + (i - (int64_t)c * step);  // + a * step: the line's samples, a in [0, len)
        float best = __builtin_inff();
        int at = -1;
        float below = line[(int64_t)c * step], above = below;  // the samples at lo + 1 and at hi
        for (int d = 0; d < len; ++d) {
            if ((float)(d * d) > fminf(best, R2)) break;
            const int lo = c - 1 - d, hi = c + d;
            if (lo < 0 && hi > len - 2) break;
            float f;
            if (lo >= 0) {
                const float va = line[(int64_t)lo * step];
                if (redist_crossing(va, below, f)) {
                    const float t = sub_rn((float)(c - lo), f);
                    const float cost = mul_rn(t, t);
                    if (cost <= best) { best = cost; at = lo; }
                }
                below = va;
            }
            if (hi <= len - 2) {
                const float vb = line[(int64_t)(hi + 1) * step];
                if (redist_crossing(above, vb, f)) {
                    const float t = sub_rn((float)(c - hi), f);
                    const float cost = mul_rn(t, t);
                    if (cost < best) { best = cost; at = hi; }
                }
                above = vb;
            }
        }
        if (best > R2) at = -1;
        out[i] = redist_state(at < 0 ? __builtin_inff() : best, at);
    }
}

// One outward scan over the states of a line (len voxels, `step` flat indices apart, `line` its first state) around position c.
// Returns the winning position, -1 when no candidate has a site or the best costs more than R2; `packed` is the winner's.
PVAMD_DEV int redist_scan(const state2* __restrict__ line, int64_t step, int c, int len, float R2, float& best, int& packed) {
    int at = -1;
    best = __builtin_inff();
    packed = -1;
    for (int d = 0; d < len; ++d) {
        const float dd = (float)(d * d);
        if (dd > fminf(best, R2)) break;
        const int lo = c - d, hi = c + d;
        if (lo < 0 && hi >= len) break;
        if (lo >= 0) {
            const state2 s = line[(int64_t)lo * step];
            const int p = __float_as_int(s.y);
            const float cost = add_rn(s.x, dd);
            if (p >= 0 && cost <= best) { best = cost; at = lo; packed = p; }
        }
        if (d > 0 && hi < len) {
            const state2 s = line[(int64_t)hi * step];
            const int p = __float_as_int(s.y);
            const float cost = add_rn(s.x, dd);
            if (p >= 0 && cost < best) { best = cost; at = hi; packed = p; }
        }
    }
    if (best > R2) at = -1;
    return at;
}

// Pass 2 of a family: along `axis` over the states of pass 1.
__global__ __launch_bounds__(256) void redist_line_kernel(const state2* __restrict__ in, int64_t n, int ny, int nz, int axis, int len,
                                                          int64_t step, float R2, state2* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c = redist_coordinate((unsigned)i, (unsigned)ny, (unsigned)nz, axis);
        float best;
        int packed;
        const int at = redist_scan(in + (i - (int64_t)c * step), step, c, len, R2, best, packed);
        out[i] = at < 0 ? redist_state(__builtin_inff(), -1) : redist_state(best, packed | (at << kAxisBits));
    }
}

// Pass 3 of all three families, and the records.  A kept voxel scans nothing.
__global__ __launch_bounds__(256) void redist_last_kernel(const f32x4* __restrict__ records_in, const float* __restrict__ V,
                                                          const state2* __restrict__ Bx, const state2* __restrict__ By,
                                                          const state2* __restrict__ Bz, int64_t n, int nx, int ny, int nz,
                                                          float resolution, float band, float max_distance, float R2,
                                                          f32x4* __restrict__ records_out, int* __restrict__ sites,
                                                          float* __restrict__ squared) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)ny * (unsigned)nz;
    const float inf = __builtin_inff();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Voxel here = voxel_of((unsigned)i, plane, (unsigned)nz);
        const int x = (int)here.x, y = (int)here.y, z = (int)here.z;
        const float v = V[i];
        if (fabsf(v) < band) {  // NaN: not kept
            records_out[i] = records_in[i];
            if (sites) sites[i] = PVAMD_REDIST_KEPT;
            if (squared) squared[i] = inf;
            continue;
        }
        const bool negative = v < 0.0f;
        // family x ends along y; families y and z end along x
        float best, cost;
        int packed, pk, k = 0;
        int at = redist_scan(Bx + (i - (int64_t)y * nz), nz, y, ny, R2, best, packed);
        int a = redist_scan(By + (i - (int64_t)x * plane), plane, x, nx, R2, cost, pk);
        if (a >= 0 && (at < 0 || cost < best)) { best = cost; at = a; packed = pk; k = 1; }
        a = redist_scan(Bz + (i - (int64_t)x * plane), plane, x, nx, R2, cost, pk);
        if (a >= 0 && (at < 0 || cost < best)) { best = cost; at = a; packed = pk; k = 2; }
        f32x4 rec = {negative ? -max_distance : max_distance, 0.0f, 0.0f, 0.0f};
        int site = -1;
        float c3 = inf;
        if (at >= 0) {
            const int first = packed & kAxisMask, second = packed >> kAxisBits;
            const int ax = k == 0 ? first : at;
            const int ay = k == 0 ? at : (k == 1 ? first : second);
            const int az = k == 2 ? first : second;
            const unsigned aflat = ((unsigned)ax * (unsigned)ny + (unsigned)ay) * (unsigned)nz + (unsigned)az;
            site = (int)(aflat * 4u + (unsigned)k);
            c3 = best;
            const float va = V[aflat], vb = V[aflat + (k == 0 ? plane : (k == 1 ? (unsigned)nz : 1u))];
            const float f = div_rn(va, sub_rn(va, vb));
            const float len = sqrt_rn(c3);
            const float val = mul_rn(resolution, len);
            rec.x = negative ? -val : val;
            if (c3 != 0.0f) {
                const float ex = k == 0 ? sub_rn((float)(x - ax), f) : (float)(x - ax);
                const float ey = k == 1 ? sub_rn((float)(y - ay), f) : (float)(y - ay);
                const float ez = k == 2 ? sub_rn((float)(z - az), f) : (float)(z - az);
                const float gx = div_rn(ex, len), gy = div_rn(ey, len), gz = div_rn(ez, len);
                rec.y = negative ? -gx : gx;
                rec.z = negative ? -gy : gy;
                rec.w = negative ? -gz : gz;
            }
        }
        records_out[i] = rec;
        if (sites) sites[i] = site;
        if (squared) squared[i] = c3;
    }
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_redistance_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!lattice_shape_ok(nx, ny, nz, PVAMD_REDIST_MIN_AXIS, PVAMD_REDIST_MAX_VOXELS)) return 0;
    return (int64_t)nx * ny * nz * 36;
}

extern "C" int pvamd_redistance(const float* records_in, int32_t nx, int32_t ny, int32_t nz, float resolution, float band,
                                float max_distance, float* records_out, int32_t* sites, float* squared, void* scratch,
                                void* stream) {
    if (!lattice_shape_ok(nx, ny, nz, PVAMD_REDIST_MIN_AXIS, PVAMD_REDIST_MAX_VOXELS)) return PVAMD_E_SHAPE;
    if (!(resolution > 0.0f && resolution < __builtin_inff()) || !(band >= 0.0f) || !(max_distance > 0.0f)) return PVAMD_E_MODE;
    if (!records_in || !records_out || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(records_in, 16) || !aligned_to(records_out, 16) || !aligned_to(scratch, 4) || !aligned_to(sites, 4) ||
        !aligned_to(squared, 4))
        return PVAMD_E_ALIGN;
    const int64_t n = (int64_t)nx * ny * nz, plane = (int64_t)ny * nz;
    const float Rv = max_distance / resolution;  // -ffp-contract=off: rounded on their own, as the contract's div_rn and mul_rn
    const float R2 = Rv * Rv;
    float* V = (float*)scratch;
    state2* A = (state2*)(V + n);
    state2* B[3] = {A + n, A + 2 * n, A + 3 * n};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(stream_grid(n, 256)), block(256);
    hipLaunchKernelGGL(redist_values_kernel, grid, block, 0, s, reinterpret_cast<const f32x4*>(records_in), n, V);
    const int len[3] = {nx, ny, nz};
    const int64_t step[3] = {plane, (int64_t)nz, 1};
    for (int k = 2; k >= 0; --k) {
        const int p2 = k == 2 ? 1 : 2;  // the higher of the two remaining axes
        hipLaunchKernelGGL(redist_edge_kernel, grid, block, 0, s, V, n, ny, nz, k, len[k], step[k], R2, A);
        hipLaunchKernelGGL(redist_line_kernel, grid, block, 0, s, A, n, ny, nz, p2, len[p2], step[p2], R2, B[k]);
    }
    hipLaunchKernelGGL(redist_last_kernel, grid, block, 0, s, reinterpret_cast<const f32x4*>(records_in), V, B[0], B[1], B[2], n, nx,
                       ny, nz, resolution, band, max_distance, R2, reinterpret_cast<f32x4*>(records_out), sites, squared);
    return (int)hipGetLastError();
}
