// Occupancy from sensor rays (include/pvamd.h "Ray integration"): one scan of R rays classifies the voxels of a lattice -- the
// voxels the rays crossed as FREE, the voxels their endpoints fall into as HIT -- and one pass over the voxels moves a log-odds
// map by that classification.  Replaces nothing in the reference: its voxel.py stops at the containers, which can only add.
//
// Three launches on one stream, and nothing is handed between workgroups inside any of them:
//   ray_walk_kernel   one lane per ray, grid-stride: the contract's cell walk (an Amanatides-Woo traversal whose exit parameters
//                     are recomputed from the cell, never accumulated).  A visit is one byte load and, where it read 0, one byte
//                     store of FREE; every writer stores the same value, so a stale 0 only repeats an identical store.
//   ray_hit_kernel    one lane per ray: HIT at the voxel voxel_flat gives the endpoint (what grid[e] = 1 writes).  Its own launch,
//                     so that HIT over FREE rests on stream order and on no ordering between workgroups.
//   occupancy_update_kernel  four voxels per lane: the clamped log-odds step, observed |= touched, marks back to 0.  A word of
//                     four untouched marks -- most of a map in any one scan -- costs its 4-byte load and nothing else.
// No atomics, no allocation, no host synchronisation.  Rays of one wave stop at different step counts; nothing sorts or compacts
// them (profiles/ray_integrate.md has the measured cost).
#include "common.h"
#include "grid_lookup.h"

namespace pvamd {

PVAMD_DEV bool ray_finite(const float o[3], const float e[3]) {
    const float inf = __builtin_inff();
    return fabsf(o[0]) < inf && fabsf(o[1]) < inf && fabsf(o[2]) < inf && fabsf(e[0]) < inf && fabsf(e[1]) < inf && fabsf(e[2]) < inf;
}

// statement 5: the ray's length in world units
PVAMD_DEV float ray_length(const float o[3], const float e[3]) {
    const float vx = sub_rn(e[0], o[0]), vy = sub_rn(e[1], o[1]), vz = sub_rn(e[2], o[2]);
    return sqrt_rn(add_rn(add_rn(mul_rn(vx, vx), mul_rn(vy, vy)), mul_rn(vz, vz)));
}

// statement 6c: where the ray leaves cell c along one axis
PVAMD_DEV float ray_exit(int c, int step, float a, float d) {
    return step == 0 ? __builtin_inff() : div_rn(sub_rn(add_rn((float)c, mul_rn(0.5f, (float)step)), a), d);
}

template <bool SHARED>
__global__ __launch_bounds__(256) void ray_walk_kernel(Lattice L, const float* __restrict__ origins,
                                                       const float* __restrict__ endpoints, int64_t R, float max_range,
                                                       uint8_t* __restrict__ marks) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int budget = L.n[0] + L.n[1] + L.n[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += stride) {
        const float* op = SHARED ? origins : origins + 3 * i;
        const float o[3] = {op[0], op[1], op[2]};
        const float e[3] = {endpoints[3 * i], endpoints[3 * i + 1], endpoints[3 * i + 2]};
        if (!ray_finite(o, e)) continue;
        const float len = ray_length(o, e);
        float t0 = 0.0f, t1 = len > max_range ? div_rn(max_range, len) : 1.0f;
        float a[3], d[3];
        bool walk = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = div_rn(sub_rn(o[k], L.fmin[k]), L.fres[k]);
            d[k] = sub_rn(div_rn(sub_rn(e[k], L.fmin[k]), L.fres[k]), a[k]);
            const float top = sub_rn((float)L.n[k], 0.5f);
            if (!(fabsf(d[k]) < __builtin_inff())) {
                walk = false;
            } else if (d[k] == 0.0f) {
                walk &= (-0.5f <= a[k]) && (a[k] < top);
            } else {
                const float u = div_rn(sub_rn(-0.5f, a[k]), d[k]), w = div_rn(sub_rn(top, a[k]), d[k]);
                t0 = fmaxf(t0, fminf(u, w));
                t1 = fminf(t1, fmaxf(u, w));
            }
        }
        if (!walk || !(t0 <= t1)) continue;
        int c[3], step[3];
        float tmax[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float at = add_rn(a[k], mul_rn(t0, d[k]));
            c[k] = (int)fminf(fmaxf(floorf(add_rn(at, 0.5f)), 0.0f), (float)(L.n[k] - 1));
            step[k] = d[k] > 0.0f ? 1 : (d[k] < 0.0f ? -1 : 0);
            tmax[k] = ray_exit(c[k], step[k], a[k], d[k]);
        }
        for (int visit = 0; visit < budget; ++visit) {
            uint8_t* cell = marks + ((int64_t)c[0] * L.n[1] + c[1]) * L.n[2] + c[2];  // c stays inside the grid: the step below checks
            const uint8_t seen = *cell;
            int k = tmax[1] < tmax[0] ? 1 : 0;
            const float near = k ? tmax[1] : tmax[0];
            k = tmax[2] < near ? 2 : k;
            const float exit_t = tmax[2] < near ? tmax[2] : near;
            if (seen == 0) *cell = PVAMD_MARK_FREE;
            if (!(exit_t < t1)) break;
            // one axis moves; written without a runtime-indexed array, which would live in scratch
            const int ck = (k == 0 ? c[0] : (k == 1 ? c[1] : c[2])) + (k == 0 ? step[0] : (k == 1 ? step[1] : step[2]));
            if (ck < 0 || ck >= (k == 0 ? L.n[0] : (k == 1 ? L.n[1] : L.n[2]))) break;
            const float tk = ray_exit(ck, k == 0 ? step[0] : (k == 1 ? step[1] : step[2]), k == 0 ? a[0] : (k == 1 ? a[1] : a[2]),
                                      k == 0 ? d[0] : (k == 1 ? d[1] : d[2]));
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                c[j] = j == k ? ck : c[j];
                tmax[j] = j == k ? tk : tmax[j];
            }
        }
    }
}

template <bool SHARED, bool F64>
__global__ __launch_bounds__(256) void ray_hit_kernel(pvamd_grid_t g, const float* __restrict__ origins,
                                                      const float* __restrict__ endpoints, int64_t R, float max_range,
                                                      uint8_t* __restrict__ marks) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += stride) {
        const float* op = SHARED ? origins : origins + 3 * i;
        const float o[3] = {op[0], op[1], op[2]};
        const float e[3] = {endpoints[3 * i], endpoints[3 * i + 1], endpoints[3 * i + 2]};
        if (!ray_finite(o, e) || ray_length(o, e) > max_range) continue;
        int flat;
        if (voxel_flat<F64>(g, e[0], e[1], e[2], flat)) marks[flat] = PVAMD_MARK_HIT;  // flat is clamped into the grid
    }
}

PVAMD_DEV float log_odds_step(float L, unsigned mark, float l_hit, float l_miss, float l_min, float l_max) {
    if (mark == 0) return L;
    return fminf(fmaxf(add_rn(L, mark == PVAMD_MARK_HIT ? l_hit : l_miss), l_min), l_max);
}

// words = n / 4 whole groups of four voxels, one per lane and turn; the lane after the last group takes the n % 4 voxels left
__global__ __launch_bounds__(256) void occupancy_update_kernel(uint8_t* __restrict__ marks, int64_t n, float l_hit, float l_miss,
                                                               float l_min, float l_max, float* __restrict__ log_odds,
                                                               uint8_t* __restrict__ observed) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t words = n >> 2;
    uint32_t* marks4 = reinterpret_cast<uint32_t*>(marks);
    uint32_t* observed4 = reinterpret_cast<uint32_t*>(observed);
    f32x4* log_odds4 = reinterpret_cast<f32x4*>(log_odds);
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= words; w += stride) {
        if (w == words) {
            for (int64_t i = words << 2; i < n; ++i) {
                const unsigned m = marks[i];
                if (m == 0) continue;
                log_odds[i] = log_odds_step(log_odds[i], m, l_hit, l_miss, l_min, l_max);
                if (observed) observed[i] = 1;
                marks[i] = 0;
            }
            continue;
        }
        const uint32_t m = marks4[w];
        if (m == 0) continue;
        f32x4 L = log_odds4[w];
        L.x = log_odds_step(L.x, m & 0xffu, l_hit, l_miss, l_min, l_max);
        L.y = log_odds_step(L.y, (m >> 8) & 0xffu, l_hit, l_miss, l_min, l_max);
        L.z = log_odds_step(L.z, (m >> 16) & 0xffu, l_hit, l_miss, l_min, l_max);
        L.w = log_odds_step(L.w, m >> 24, l_hit, l_miss, l_min, l_max);
        log_odds4[w] = L;
        if (observed) {
            const uint32_t touched = ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 0x100u : 0u) | ((m & 0xff0000u) ? 0x10000u : 0u) |
                                     ((m >> 24) ? 0x1000000u : 0u);
            observed4[w] |= touched;
        }
        marks4[w] = 0;
    }
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int pvamd_ray_mark(const pvamd_grid_t* grid, const float* origins, int32_t shared_origin, const float* endpoints,
                              int64_t R, float max_range, uint8_t* marks, void* stream) {
    if (R < 0) return PVAMD_E_SHAPE;
    if (!grid) return PVAMD_E_NULL;
    // the cap on the voxels is the descriptor's own, check_grid's
    const int32_t* shape = grid->shape;
    if (!lattice_shape_ok(shape[0], shape[1], shape[2], PVAMD_RAY_MARK_MIN_AXIS, INT64_MAX)) return PVAMD_E_SHAPE;
    if (int e = check_grid(*grid, /*need_vox=*/false)) return e;
    if (!(max_range > 0.0f)) return PVAMD_E_MODE;  // NaN included
    if (shared_origin != 0 && shared_origin != 1) return PVAMD_E_MODE;
    if (R == 0) return 0;
    if (!origins || !endpoints || !marks) return PVAMD_E_NULL;
    const Lattice L = lattice_of(*grid);
    hipStream_t s = (hipStream_t)stream;
    const dim3 gd(stream_grid(R, 256)), block(256);
    if (shared_origin) hipLaunchKernelGGL((ray_walk_kernel<true>), gd, block, 0, s, L, origins, endpoints, R, max_range, marks);
    else hipLaunchKernelGGL((ray_walk_kernel<false>), gd, block, 0, s, L, origins, endpoints, R, max_range, marks);
    if (shared_origin) {
        if (grid->index_f64) hipLaunchKernelGGL((ray_hit_kernel<true, true>), gd, block, 0, s, *grid, origins, endpoints, R, max_range, marks);
        else hipLaunchKernelGGL((ray_hit_kernel<true, false>), gd, block, 0, s, *grid, origins, endpoints, R, max_range, marks);
    } else {
        if (grid->index_f64) hipLaunchKernelGGL((ray_hit_kernel<false, true>), gd, block, 0, s, *grid, origins, endpoints, R, max_range, marks);
        else hipLaunchKernelGGL((ray_hit_kernel<false, false>), gd, block, 0, s, *grid, origins, endpoints, R, max_range, marks);
    }
    return (int)hipGetLastError();
}

extern "C" int pvamd_occupancy_update(uint8_t* marks, int64_t n, float l_hit, float l_miss, float l_min, float l_max,
                                      float* log_odds, uint8_t* observed, void* stream) {
    if (n < 0) return PVAMD_E_SHAPE;
    if (l_hit != l_hit || l_miss != l_miss || !(l_min <= l_max)) return PVAMD_E_MODE;
    if (n == 0) return 0;
    if (!marks || !log_odds) return PVAMD_E_NULL;
    if (!aligned_to(log_odds, 16) || !aligned_to(marks, 4) || !aligned_to(observed, 4)) return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(occupancy_update_kernel, dim3(stream_grid((n >> 2) + 1, 256)), dim3(256), 0, (hipStream_t)stream, marks, n,
                       l_hit, l_miss, l_min, l_max, log_odds, observed);
    return (int)hipGetLastError();
}
