// Fused hinge penalty over points of a ComposedSDF / RobotSDF query (include/pvamd.h "Hinge penalty over points"): for every
// pair (configuration a, z) -- z = 0 over all leaves (the composed value), or z = s for leaf s alone -- the sum over points of
// max(m - v, 0) ** power, and the number of points with v < m.  Nothing of size A x P is written.
//
//   pass 1 (hop_partial_kernel)  workgroup (chunk, a, z): the pair's value at each point of a 4096-point chunk (mop_point, the
//                                 fused forwards' own statements), the term rounded in the query dtype as torch rounds
//                                 (m - v).clamp(min=0) ** power, added in float64: per lane in point order, then a wave
//                                 butterfly, then the four waves in order; one (sum, count) per (pair, chunk)
//   pass 2 (hop_finish_kernel)    one wave per pair: the chunks' sums added in chunk order, rounded once to the query dtype
// Every order depends only on (S, A, P): the result repeats bit for bit.  No float atomics, no host synchronisation.
// The backward is composed_backward_kernel's HINGE policy (backward.hip).
#include "common.h"
#include "composed_point.h"

namespace pvamd {

// ---- pass 1: workgroup (chunk, a, z) -> part[(a * Z + z) * nchunks + chunk] ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(kHopBlock) void hop_partial_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                const T* __restrict__ tf, int A, const T* __restrict__ pts,
                                                                int64_t P, int per_leaf, T m, int power, int64_t nchunks,
                                                                HopPart* __restrict__ part) {
    __shared__ double ws[kHopBlock / 64];
    __shared__ int wc[kHopBlock / 64];
    const int64_t chunk = blockIdx.x;
    const int z = blockIdx.z, Z = per_leaf ? S : 1;
    const int s0 = per_leaf ? z : 0, s1 = per_leaf ? z + 1 : S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int a = blockIdx.y; a < A; a += gridDim.y) {
        double sum = 0.0;
        int cnt = 0;
#pragma unroll 1
        for (int k = 0; k < kHopK; ++k) {
            const int64_t i = chunk * PVAMD_MOP_CHUNK + (int64_t)k * kHopBlock + threadIdx.x;
            if (i < P) {
                const T p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
                T v, g[3];
                int s;
                mop_point<T, INTERP>(grids, s0, s1, tf, A, a, p, v, g, s);
                const T d = m - v;
                const T h = (d > T(0) || d != d) ? d : T(0);  // clamp(min=0): NaN stays NaN
                sum += (double)(power == 2 ? h * h : h);
                cnt += v < m;
            }
        }
        sum = hop_wave_sum<double>(sum);
        cnt = hop_wave_sum<int>(cnt);
        if (lane == 0) { ws[wave] = sum; wc[wave] = cnt; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kHopBlock / 64; ++w) { sum += ws[w]; cnt += wc[w]; }
            HopPart r;
            r.sum = sum; r.count = cnt;
            part[((int64_t)a * Z + z) * nchunks + chunk] = r;
        }
        __syncthreads();
    }
}

// ---- pass 2: one wave per pair; 64 chunks loaded at a time, added in chunk order ----
template <typename T>
__global__ __launch_bounds__(64) void hop_finish_kernel(int64_t npairs, int64_t nchunks, const HopPart* __restrict__ part,
                                                        T* __restrict__ out_val, int64_t* __restrict__ out_count) {
    for (int64_t pr = blockIdx.x; pr < npairs; pr += gridDim.x) {
        double sum = 0.0;
        int64_t cnt = 0;
        for (int64_t base = 0; base < nchunks; base += 64) {
            const int64_t c = base + threadIdx.x;
            HopPart q;
            q.sum = 0.0; q.count = 0;
            if (c < nchunks) q = part[pr * nchunks + c];
            cnt += q.count;
            const int n = (nchunks - base) < 64 ? (int)(nchunks - base) : 64;
            for (int j = 0; j < n; ++j) sum += __shfl(q.sum, j, 64);  // every lane: the same sum in chunk order
        }
        cnt = hop_wave_sum<int64_t>(cnt);
        if (threadIdx.x == 0) {
            out_val[pr] = (T)sum;
            out_count[pr] = cnt;
        }
    }
}

template <typename T, bool INTERP>
static void hop_launch(const pvamd_grid_t* grids, int S, const T* tf, int A, const T* points, int64_t P, int per_leaf, T m,
                       int power, T* out_val, int64_t* out_count, HopPart* part, hipStream_t st) {
    const int64_t nchunks = (P + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK;
    const int Z = per_leaf ? S : 1;
    const int64_t npairs = (int64_t)A * Z;
    hipLaunchKernelGGL((hop_partial_kernel<T, INTERP>), dim3((unsigned)nchunks, grid_rows(A), (unsigned)Z),
                       dim3(kHopBlock), 0, st, grids, S, tf, A, points, P, per_leaf, m, power, nchunks, part);
    hipLaunchKernelGGL(hop_finish_kernel<T>, dim3((unsigned)(npairs < 0x7fffffff ? npairs : 0x7fffffff)), dim3(64), 0, st, npairs,
                       nchunks, part, out_val, out_count);
}

template <typename T>
static int hinge_over_points(const pvamd_grid_t* grids, int32_t S, const T* tf, int32_t A, const T* points, int64_t P, int32_t mode,
                             int32_t per_leaf, T margin, int32_t power, T* out_val, int64_t* out_count, void* scratch, void* stream) {
    if (S < 1 || A < 1 || P < 1 || (per_leaf && S > kMaxGridRows) || (P + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK > 0x7fffffff)
        return PVAMD_E_SHAPE;
    if ((mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) || (per_leaf != 0 && per_leaf != 1) ||
        (power != 1 && power != 2))
        return PVAMD_E_MODE;
    if (!grids || !tf || !points || !out_val || !out_count || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(points, sizeof(T)) || !aligned_to(grids, 8) || !aligned_to(out_val, sizeof(T)) ||
        !aligned_to(out_count, 8) || !aligned_to(scratch, 16))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    HopPart* part = (HopPart*)scratch;
    if (mode == PVAMD_LEAF_TRILINEAR)
        hop_launch<T, true>(grids, S, tf, A, points, P, per_leaf, margin, power, out_val, out_count, part, st);
    else
        hop_launch<T, false>(grids, S, tf, A, points, P, per_leaf, margin, power, out_val, out_count, part, st);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_hinge_over_points_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t per_leaf) {
    if (S < 1 || A < 1 || P < 1) return 0;
    return PVAMD_HINGE_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf);
}

extern "C" int pvamd_composed_hinge_over_points(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                                int64_t P, int32_t mode, int32_t per_leaf, float margin, int32_t power,
                                                float* out_val, int64_t* out_count, void* scratch, void* stream) {
    return hinge_over_points<float>(grids, S, tf, A, points, P, mode, per_leaf, margin, power, out_val, out_count, scratch, stream);
}

extern "C" int pvamd_composed_hinge_over_points_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                    const double* points, int64_t P, int32_t mode, int32_t per_leaf, double margin,
                                                    int32_t power, double* out_val, int64_t* out_count, void* scratch,
                                                    void* stream) {
    return hinge_over_points<double>(grids, S, tf, A, points, P, mode, per_leaf, margin, power, out_val, out_count, scratch,
                                     stream);
}
