// Fused minimum over points of a ComposedSDF / RobotSDF query (include/pvamd.h "Minimum over points"): for every pair
// (configuration a, z) -- z = 0 over all leaves (the composed first minimum), or z = s for leaf s alone -- the smallest point
// index p that minimises the pair's value, and the value and gradient at p.  Nothing of size A x P is written.
//
//   pass 1 (mop_partial_kernel)  workgroup (chunk, a, z): the pair's value at each point of a 4096-point chunk, kept per lane
//                                 as (value, first index) and reduced over the workgroup to one key; one key per (pair, chunk)
//   pass 2 (mop_finish_kernel)    one wave per pair: the minimum key over the chunks, then the pair's value, gradient and
//                                 winning leaf recomputed at that point with the same statements (the exact bits)
// The key of a value v is its order-preserving bit pattern (NaN lowest, -0 as +0) followed by the point index; the order of
// keys is total and min is exact, so the result does not depend on the launch geometry and repeats bit for bit.
//
// The leaf statements are the fused forwards' own: float32 nearest = cached_lookup (the cached kernels' fast index with the
// exact fallback, the bounding-box branch), float32 trilinear = composed_interp_kernel's leaf, float64 = leaf_f64; then the
// first minimum over leaves and R^T rotation back of pvamd_composed_query_interp / _f64.
//
// Backward (mop_backward_kernel): one lane per pair, the VJP of composed_backward_kernel (backward.hip) for that single pair
// (the leaf VJPs of leaf_vjp.h).  Every dtf row belongs to at most one pair, so it is written, not summed; dpoints rows are
// summed over the pairs that selected them, in pair order (mop_scatter_kernel).  No float atomics anywhere.
#include "common.h"
#include "grid_lookup.h"
#include "interp.h"
#include "leaf_vjp.h"
#include "composed_point.h"

namespace pvamd {

constexpr int kMopBlock = 256;
constexpr int kMopK = PVAMD_MOP_CHUNK / kMopBlock;  // points per lane per chunk
static_assert(kMopK * kMopBlock == PVAMD_MOP_CHUNK, "whole lanes per chunk");
// ---- pass 1: workgroup (chunk, a, z) -> part[(a * Z + z) * nchunks + chunk] ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(kMopBlock) void mop_partial_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                const T* __restrict__ tf, int A, const T* __restrict__ pts,
                                                                int64_t P, int per_leaf, int64_t nchunks,
                                                                MopKey* __restrict__ part) {
    __shared__ uint64_t wk[kMopBlock / 64];
    __shared__ uint32_t wi[kMopBlock / 64];
    const int64_t chunk = blockIdx.x;
    const int z = blockIdx.z, Z = per_leaf ? S : 1;
    const int s0 = per_leaf ? z : 0, s1 = per_leaf ? z + 1 : S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int a = blockIdx.y; a < A; a += gridDim.y) {
        T bv = T(0);
        uint32_t bi = kNoIndex;
        // lane order = point order: the lane keeps the first of its points that reaches its minimum
#pragma unroll 1
        for (int k = 0; k < kMopK; ++k) {
            const int64_t i = chunk * PVAMD_MOP_CHUNK + (int64_t)k * kMopBlock + threadIdx.x;
            if (i < P) {
                const T p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
                T v, g[3];
                int s;
                mop_point<T, INTERP>(grids, s0, s1, tf, A, a, p, v, g, s);
                const bool take = (bi == kNoIndex) | (!(v >= bv) & (bv == bv));
                bv = take ? v : bv;
                bi = take ? (uint32_t)i : bi;
            }
        }
        uint64_t key = bi == kNoIndex ? ~0ull : mop_key(bv);
        mop_wave_min(key, bi);
        if (lane == 0) { wk[wave] = key; wi[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kMopBlock / 64; ++w)
                if (mop_less(wk[w], wi[w], key, bi)) { key = wk[w]; bi = wi[w]; }
            MopKey r;
            r.key = key; r.idx = bi; r.pad = 0;
            part[((int64_t)a * Z + z) * nchunks + chunk] = r;
        }
        __syncthreads();
    }
}

// ---- pass 2: one wave per pair; the answer at the chosen point ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(64) void mop_finish_kernel(const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ tf,
                                                        int A, const T* __restrict__ pts, int64_t P, int per_leaf, int64_t nchunks,
                                                        const MopKey* __restrict__ part, T* __restrict__ out_val,
                                                        T* __restrict__ out_grad, int64_t* __restrict__ out_index,
                                                        int32_t* __restrict__ out_leaf) {
    const int Z = per_leaf ? S : 1;
    const int64_t npairs = (int64_t)A * Z;
    for (int64_t pr = blockIdx.x; pr < npairs; pr += gridDim.x) {
        uint64_t key = ~0ull;
        uint32_t idx = kNoIndex;
        for (int64_t c = threadIdx.x; c < nchunks; c += 64) {
            const MopKey m = part[pr * nchunks + c];
            if (mop_less(m.key, m.idx, key, idx)) { key = m.key; idx = m.idx; }
        }
        mop_wave_min(key, idx);
        if (threadIdx.x == 0) {
            const int a = (int)(pr / Z), z = (int)(pr - (int64_t)a * Z);
            const int64_t i = idx < (uint64_t)P ? (int64_t)idx : 0;  // always true for P >= 1; keeps the load in bounds
            const T p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
            T v, g[3];
            int s;
            mop_point<T, INTERP>(grids, per_leaf ? z : 0, per_leaf ? z + 1 : S, tf, A, a, p, v, g, s);
            out_val[pr] = v;
            out_grad[3 * pr] = g[0];
            out_grad[3 * pr + 1] = g[1];
            out_grad[3 * pr + 2] = g[2];
            out_index[pr] = i;
            if (out_leaf) out_leaf[pr] = s;
        }
    }
}

// ---- backward: one lane per pair (a, z) with its point index[pr] and winning leaf leaf[pr] ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(256) void mop_backward_kernel(const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ tf,
                                                           int A, const T* __restrict__ pts, int64_t P, int per_leaf,
                                                           const int64_t* __restrict__ index, const int32_t* __restrict__ leaf,
                                                           const T* __restrict__ dval, const T* __restrict__ dgrad,
                                                           T* __restrict__ dtf, T* __restrict__ dp_pair) {
    const int Z = per_leaf ? S : 1;
    const int64_t npairs = (int64_t)A * Z;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pr < npairs; pr += stride) {
        const int a = (int)(pr / Z);
        const int64_t i = index[pr];
        int s = leaf[pr];
        T dp[3] = {0, 0, 0};
        // a malformed index / leaf id contributes nothing (and is never dereferenced)
        if (i >= 0 && i < P && s >= 0 && s < S) {
            const pvamd_grid_t& g = grids[s];
            const T* M = tf + 16 * ((int64_t)s * A + a);
            const T p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
            const bool has_g = dgrad != nullptr;
            const T dv = dval ? dval[pr] : T(0);
            T dgg[3] = {0, 0, 0}, dg[3] = {0, 0, 0};
            if (has_g) {
                dgg[0] = dgrad[3 * pr]; dgg[1] = dgrad[3 * pr + 1]; dgg[2] = dgrad[3 * pr + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r) dg[r] = M[4 * r] * dgg[0] + M[4 * r + 1] * dgg[1] + M[4 * r + 2] * dgg[2];
            }
            T x[3], gr[3] = {0, 0, 0}, dx[3] = {0, 0, 0};
            LeafOps<T>::xform(M, p, x);
            bool live = true;
            if (LeafOps<T>::inside(g, x)) {
                if constexpr (INTERP) InterpOps<T>::leaf(g, x, dv, dg, has_g, gr, dx);
                else if (has_g) LeafOps<T>::record_grad(g, x, gr);
                else live = false;  // value-only upstream: an in-range nearest winner contributes nothing
            } else {
                box_backward<T>(g, x, dv, dg, has_g, gr, dx);
            }
            if (live) {
#pragma unroll
                for (int j = 0; j < 3; ++j) dp[j] = M[j] * dx[0] + M[4 + j] * dx[1] + M[8 + j] * dx[2];
                if (dtf) {
                    // without a gradient upstream gr[r] * dgg[j] is no term at all (gr may be 0 / 0 inside the box)
                    T* row = dtf + 16 * ((int64_t)s * A + a);
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) row[4 * r + j] = has_g ? dx[r] * p[j] + gr[r] * dgg[j] : dx[r] * p[j];
                        row[4 * r + 3] = dx[r];
                    }
                }
            }
        }
        if (dp_pair) {
            dp_pair[3 * pr] = dp[0];
            dp_pair[3 * pr + 1] = dp[1];
            dp_pair[3 * pr + 2] = dp[2];
        }
    }
}

// dpoints[index[pr]] = the sum, in pair order, of dp_pair over the pairs that selected that point: the first such pair writes it
template <typename T>
__global__ __launch_bounds__(256) void mop_scatter_kernel(const int64_t* __restrict__ index, int64_t npairs, int64_t P,
                                                          const T* __restrict__ dp_pair, T* __restrict__ dpoints) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pr < npairs; pr += stride) {
        const int64_t i = index[pr];
        if (i < 0 || i >= P) continue;
        bool first = true;
        for (int64_t q = 0; q < pr && first; ++q) first = index[q] != i;
        if (!first) continue;
        T s[3] = {dp_pair[3 * pr], dp_pair[3 * pr + 1], dp_pair[3 * pr + 2]};
        for (int64_t q = pr + 1; q < npairs; ++q)
            if (index[q] == i) {
                s[0] += dp_pair[3 * q];
                s[1] += dp_pair[3 * q + 1];
                s[2] += dp_pair[3 * q + 2];
            }
        dpoints[3 * i] = s[0];
        dpoints[3 * i + 1] = s[1];
        dpoints[3 * i + 2] = s[2];
    }
}

template <typename T>
static int mop_check(const pvamd_grid_t* grids, int S, const T* tf, int A, const T* points, int64_t P, int mode, int per_leaf) {
    if (S < 1 || A < 1 || P < 1 || P > (int64_t)0xfffffffe || (per_leaf && S > kMaxGridRows)) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    if (per_leaf != 0 && per_leaf != 1) return PVAMD_E_MODE;
    if (!grids || !tf || !points) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(points, sizeof(T)) || !aligned_to(grids, 8)) return PVAMD_E_ALIGN;
    return 0;
}

template <typename T, bool INTERP>
static void mop_launch(const pvamd_grid_t* grids, int S, const T* tf, int A, const T* points, int64_t P, int per_leaf,
                       T* out_val, T* out_grad, int64_t* out_index, int32_t* out_leaf, MopKey* part, hipStream_t st) {
    const int64_t nchunks = (P + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK;
    const int Z = per_leaf ? S : 1;
    const int64_t npairs = (int64_t)A * Z;
    hipLaunchKernelGGL((mop_partial_kernel<T, INTERP>), dim3((unsigned)nchunks, grid_rows(A), (unsigned)Z),
                       dim3(kMopBlock), 0, st, grids, S, tf, A, points, P, per_leaf, nchunks, part);
    hipLaunchKernelGGL((mop_finish_kernel<T, INTERP>), dim3((unsigned)(npairs < 0x7fffffff ? npairs : 0x7fffffff)), dim3(64), 0, st,
                       grids, S, tf, A, points, P, per_leaf, nchunks, part, out_val, out_grad, out_index, out_leaf);
}

template <typename T>
static int min_over_points(const pvamd_grid_t* grids, int32_t S, const T* tf, int32_t A, const T* points, int64_t P, int32_t mode,
                           int32_t per_leaf, T* out_val, T* out_grad, int64_t* out_index, int32_t* out_leaf, void* scratch,
                           void* stream) {
    if (int e = mop_check<T>(grids, S, tf, A, points, P, mode, per_leaf)) return e;
    if (!out_val || !out_grad || !out_index || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(out_val, sizeof(T)) || !aligned_to(out_grad, sizeof(T)) || !aligned_to(out_index, 8) ||
        (out_leaf && !aligned_to(out_leaf, 4)) || !aligned_to(scratch, 16))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    MopKey* part = (MopKey*)scratch;
    if (mode == PVAMD_LEAF_TRILINEAR)
        mop_launch<T, true>(grids, S, tf, A, points, P, per_leaf, out_val, out_grad, out_index, out_leaf, part, st);
    else
        mop_launch<T, false>(grids, S, tf, A, points, P, per_leaf, out_val, out_grad, out_index, out_leaf, part, st);
    return (int)hipGetLastError();
}

template <typename T>
static int min_over_points_backward(const pvamd_grid_t* grids, int32_t S, const T* tf, int32_t A, const T* points, int64_t P,
                                    int32_t mode, int32_t per_leaf, const int64_t* index, const int32_t* leaf, const T* dval,
                                    const T* dgrad, T* dpoints, T* dtf, void* scratch, void* stream) {
    if (int e = mop_check<T>(grids, S, tf, A, points, P, mode, per_leaf)) return e;
    if (S > 64) return PVAMD_E_SHAPE;  // the limit of every composed backward
    if (!dpoints && !dtf) return 0;
    if (!index || !leaf || (dpoints && !scratch)) return PVAMD_E_NULL;
    if (!aligned_to(index, 8) || !aligned_to(leaf, 4) || (dval && !aligned_to(dval, sizeof(T))) ||
        (dgrad && !aligned_to(dgrad, sizeof(T))) || (dpoints && !aligned_to(dpoints, sizeof(T))) ||
        (dtf && !aligned_to(dtf, sizeof(T))) || (scratch && !aligned_to(scratch, 16)))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t npairs = (int64_t)A * (per_leaf ? S : 1);
    if (dtf && hipMemsetAsync(dtf, 0, (size_t)S * A * 16 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
    if (dpoints && hipMemsetAsync(dpoints, 0, (size_t)P * 3 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
    if (!dval && !dgrad) return (int)hipGetLastError();  // nothing flows back: zeros
    T* dp_pair = dpoints ? (T*)scratch : nullptr;
    const dim3 grd(stream_grid(npairs, 256));
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((mop_backward_kernel<T, true>), grd, dim3(256), 0, st, grids, S, tf, A, points, P, per_leaf, index, leaf,
                           dval, dgrad, dtf, dp_pair);
    else
        hipLaunchKernelGGL((mop_backward_kernel<T, false>), grd, dim3(256), 0, st, grids, S, tf, A, points, P, per_leaf, index, leaf,
                           dval, dgrad, dtf, dp_pair);
    if (dpoints)
        hipLaunchKernelGGL(mop_scatter_kernel<T>, grd, dim3(256), 0, st, index, npairs, P, dp_pair, dpoints);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_min_over_points_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t per_leaf) {
    if (S < 1 || A < 1 || P < 1) return 0;
    return PVAMD_MIN_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf);
}

// the backward's dp_pair: three values of either element size per pair
static_assert(PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(1, 1, 0) == 3 * sizeof(double), "dp_pair holds [pairs][3] doubles");
extern "C" int64_t pvamd_min_over_points_backward_scratch_bytes(int32_t S, int32_t A, int32_t per_leaf) {
    if (S < 0 || A < 0) return 0;
    return PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(S, A, per_leaf);
}

extern "C" int pvamd_composed_min_over_points(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                              int64_t P, int32_t mode, int32_t per_leaf, float* out_val, float* out_grad,
                                              int64_t* out_index, int32_t* out_leaf, void* scratch, void* stream) {
    return min_over_points<float>(grids, S, tf, A, points, P, mode, per_leaf, out_val, out_grad, out_index, out_leaf, scratch,
                                  stream);
}

extern "C" int pvamd_composed_min_over_points_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                  const double* points, int64_t P, int32_t mode, int32_t per_leaf, double* out_val,
                                                  double* out_grad, int64_t* out_index, int32_t* out_leaf, void* scratch,
                                                  void* stream) {
    return min_over_points<double>(grids, S, tf, A, points, P, mode, per_leaf, out_val, out_grad, out_index, out_leaf, scratch,
                                   stream);
}

extern "C" int pvamd_composed_min_over_points_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A,
                                                       const float* points, int64_t P, int32_t mode, int32_t per_leaf,
                                                       const int64_t* index, const int32_t* leaf, const float* dval,
                                                       const float* dgrad, float* dpoints, float* dtf, void* scratch, void* stream) {
    return min_over_points_backward<float>(grids, S, tf, A, points, P, mode, per_leaf, index, leaf, dval, dgrad, dpoints, dtf,
                                           scratch, stream);
}

extern "C" int pvamd_composed_min_over_points_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                           const double* points, int64_t P, int32_t mode, int32_t per_leaf,
                                                           const int64_t* index, const int32_t* leaf, const double* dval,
                                                           const double* dgrad, double* dpoints, double* dtf, void* scratch,
                                                           void* stream) {
    return min_over_points_backward<double>(grids, S, tf, A, points, P, mode, per_leaf, index, leaf, dval, dgrad, dpoints, dtf,
                                            scratch, stream);
}
