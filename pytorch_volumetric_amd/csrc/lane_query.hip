// One-point-per-lane cached and composed forwards: the float64 queries of both leaf modes (nearest and trilinear) and the
// float32 trilinear ones.  The tuned float32 nearest kernels are cached.hip's and composed.hip's.
//   float64 (sdf.py:545-547: output dtype = query dtype; torch promotion makes the leaf transform, the index arithmetic, the range
//   test and the BOUNDING_BOX branch float64): ONE kernel per query kind, templated on the leaf mode -- in range the record
//   widened exactly (nearest) or the interpolation of the eight corner records (trilinear, interp.h); out of range the
//   bounding-box statements in float64 (zeros for LOOKUP_GT_SDF).  24 B read + 32 B written per point and configuration, fp64
//   VALU: a correctness path for the dtype contract, not a tuned one.
//   float32 trilinear: the range decision and the out-of-range branch are the nearest mode's, bit for bit (include/pvamd.h
//   "Interpolated queries").
#include "common.h"
#include "grid_lookup.h"
#include "interp.h"

namespace pvamd {

constexpr int kLaneBlock = 256;

// ---- CachedSDF.__call__, float64 points: one point per lane (a grid-stride loop costs the trilinear leaf 14 VGPRs and a wave
// per SIMD) ----
template <bool INTERP>
__global__ __launch_bounds__(kLaneBlock) void cached_query_f64_kernel(const pvamd_grid_t g, const double* __restrict__ pts, int64_t P,
                                                                         double* __restrict__ val, double* __restrict__ grad,
                                                                         uint8_t* __restrict__ oob) {
    const int64_t i = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
    if (i >= P) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double o[4];
    const bool valid = leaf_f64<INTERP>(g, p, o);
    val[i] = o[0];
    grad[3 * i] = o[1];
    grad[3 * i + 1] = o[2];
    grad[3 * i + 2] = o[3];
    if (oob) oob[i] = valid ? 0 : 1;
}

// ---- ComposedSDF.__call__, float64 points and transform stack (a RobotSDF over a float64 chain): sdf.py:399 transforms in
// float64, every leaf answers in the query dtype, sdf.py:421 takes the first minimum (NaN counts as the minimum), sdf.py:409
// rotates the winner's float64 gradient back.  One (configuration, point) per lane, configuration fastest: blockIdx.x = a. ----
template <bool INTERP>
__global__ __launch_bounds__(256) void composed_query_f64_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                  const double* __restrict__ tf, int A,
                                                                  const double* __restrict__ pts, int64_t P,
                                                                  double* __restrict__ val, double* __restrict__ grad,
                                                                  int* __restrict__ leaf) {
    const int a = blockIdx.x;
    const int64_t stride = (int64_t)gridDim.y * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < P; i += stride) {
        const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        double bv = 0.0, bg[3] = {0.0, 0.0, 0.0};
        int bs = -1;
        for (int s = 0; s < S; ++s) {
            const double* M = tf + 16 * ((int64_t)s * A + a);  // wave-uniform: scalar loads
            double x[3], o[4];
            LeafOps<double>::xform(M, p, x);
            leaf_f64<INTERP>(grids[s], x, o);
            if ((bs < 0) || (o[0] < bv) || (o[0] != o[0] && bv == bv)) {
                bv = o[0];
                bs = s;
#pragma unroll
                for (int j = 0; j < 3; ++j) bg[j] = __builtin_fma(M[8 + j], o[3], __builtin_fma(M[4 + j], o[2], M[j] * o[1]));
            }
        }
        const int64_t o = (int64_t)a * P + i;
        val[o] = bv;
        grad[3 * o] = bg[0];
        grad[3 * o + 1] = bg[1];
        grad[3 * o + 2] = bg[2];
        if (leaf) leaf[o] = bs;
    }
}

// ---- CachedSDF.__call__ with interpolation="trilinear", float32 points: one point per lane, 12-byte point loads, eight 16-byte
// gathers in flight ----
template <bool WRITE_OOB>
__global__ __launch_bounds__(kLaneBlock) void cached_interp_kernel(const pvamd_grid_t g, const float* __restrict__ pts, int64_t P,
                                                                     float* __restrict__ val, float* __restrict__ grad,
                                                                     uint8_t* __restrict__ oob) {
    const int64_t i = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
    if (i >= P) return;
    const float x[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const bool valid = in_range(g, x[0], x[1], x[2]);
    float o[4];
    if (valid) {
        InterpCell<float> c;
        interp_cell<float>(g, x, c);
        float4 r[8];
        interp_gather(g, c.base, r);
        interp_combine<float>(r, c.f, o);
    } else if (g.oob_mode == PVAMD_OOB_BOUNDING_BOX) {
        const float4 b = bounding_box_sdf(g, x[0], x[1], x[2]);
        o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
    } else {
        o[0] = o[1] = o[2] = o[3] = 0.f;  // LOOKUP_GT_SDF: zeros, the caller fills in the ground truth
    }
    __builtin_nontemporal_store(o[0], val + i);
    __builtin_nontemporal_store(o[1], grad + 3 * i);
    __builtin_nontemporal_store(o[2], grad + 3 * i + 1);
    __builtin_nontemporal_store(o[3], grad + 3 * i + 2);
    if constexpr (WRITE_OOB) oob[i] = valid ? 0 : 1;
}

// ---- ComposedSDF.__call__ over trilinear BOUNDING_BOX leaves, float32: a point per lane; blockIdx.y strides the configurations.
// Per leaf: x = L p + t (affine_row, the nearest kernels' statement), the leaf's answer, the first minimum over leaves
// (keep_first_minimum's comparison), the winner's gradient rotated back with R^T (rotate_back's statement). ----
__global__ __launch_bounds__(kLaneBlock) void composed_interp_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                       const float* __restrict__ tf, int A,
                                                                       const float* __restrict__ pts, int64_t P,
                                                                       float* __restrict__ val, float* __restrict__ grad,
                                                                       int32_t* __restrict__ leaf) {
    const int64_t stride = (int64_t)gridDim.x * kLaneBlock;
    for (int64_t i = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x; i < P; i += stride) {
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        for (int a = blockIdx.y; a < A; a += gridDim.y) {
            // the state before any leaf (best_init): +inf loses to every finite value and to NaN; NaN gradient
            float bv = __builtin_inff(), bg[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
            int bs = 0;
            for (int s = 0; s < S; ++s) {
                const pvamd_grid_t& g = grids[s];
                const float* M = tf + 16 * ((int64_t)s * A + a);  // wave-uniform: scalar loads
                const float x[3] = {affine_row(M[0], M[1], M[2], M[3], px, py, pz), affine_row(M[4], M[5], M[6], M[7], px, py, pz),
                                    affine_row(M[8], M[9], M[10], M[11], px, py, pz)};
                float o[4];
                if (in_range(g, x[0], x[1], x[2])) {
                    InterpCell<float> c;
                    interp_cell<float>(g, x, c);
                    float4 r[8];
                    interp_gather(g, c.base, r);
                    interp_combine<float>(r, c.f, o);
                } else {
                    const float4 b = bounding_box_sdf(g, x[0], x[1], x[2]);
                    o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
                }
                const bool take = !(o[0] >= bv) & (bv == bv);  // torch.argmin: first minimum, NaN counts as the minimum
                bv = take ? o[0] : bv;
                bg[0] = take ? o[1] : bg[0];
                bg[1] = take ? o[2] : bg[1];
                bg[2] = take ? o[3] : bg[2];
                bs = take ? s : bs;
            }
            const float* M = tf + 16 * ((int64_t)bs * A + a);
            const int64_t o = (int64_t)a * P + i;
            __builtin_nontemporal_store(bv, val + o);
            __builtin_nontemporal_store(fmaf(M[8], bg[2], fmaf(M[4], bg[1], mul_rn(M[0], bg[0]))), grad + 3 * o);
            __builtin_nontemporal_store(fmaf(M[9], bg[2], fmaf(M[5], bg[1], mul_rn(M[1], bg[0]))), grad + 3 * o + 1);
            __builtin_nontemporal_store(fmaf(M[10], bg[2], fmaf(M[6], bg[1], mul_rn(M[2], bg[0]))), grad + 3 * o + 2);
            if (leaf) leaf[o] = bs;
        }
    }
}

// ---- argument checks of the entry points below (T: the point dtype); 0 also for P == 0, which the caller returns on ----
template <typename T>
static int check_cached(const pvamd_grid_t* grid, const T* points, int64_t P, const T* out_val, const T* out_grad) {
    if (P < 0) return PVAMD_E_SHAPE;
    if (P == 0) return 0;  // empty query: nothing to read or write (torch hands out NULL for empty tensors)
    if (!grid || !out_val || !out_grad || !points) return PVAMD_E_NULL;
    if (int e = check_grid(*grid)) return e;
    if (!aligned_to(points, sizeof(T)) || !aligned_to(out_val, sizeof(T)) || !aligned_to(out_grad, sizeof(T))) return PVAMD_E_ALIGN;
    return 0;
}

template <typename T>
static int check_composed(const pvamd_grid_t* grids, int S, const T* tf, int A, const T* points, int64_t P, const T* out_val,
                          const T* out_grad) {
    if (S < 1 || A < 1 || P < 0) return PVAMD_E_SHAPE;
    if (P == 0) return 0;
    if (!grids || !tf || !points || !out_val || !out_grad) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(points, sizeof(T)) || !aligned_to(out_val, sizeof(T)) ||
        !aligned_to(out_grad, sizeof(T)) || !aligned_to(grids, 8))
        return PVAMD_E_ALIGN;
    return 0;
}

// grid of the one-point-per-lane cached kernels: as many blocks as the points need (at most the 2^31 - 1 HIP allows)
static int cached_lane_blocks(int64_t P, dim3& grid) {
    const int64_t blocks = (P + kLaneBlock - 1) / kLaneBlock;
    if (blocks > 0x7fffffff) return PVAMD_E_SHAPE;
    grid = dim3((unsigned)blocks);
    return 0;
}

template <bool INTERP>
static int cached_f64(const pvamd_grid_t* grid, const double* points, int64_t P, double* out_val, double* out_grad, uint8_t* out_oob,
                      void* stream) {
    if (int e = check_cached<double>(grid, points, P, out_val, out_grad)) return e;
    if (P == 0) return 0;
    dim3 blocks;
    if (int e = cached_lane_blocks(P, blocks)) return e;
    hipLaunchKernelGGL(cached_query_f64_kernel<INTERP>, blocks, dim3(kLaneBlock), 0, (hipStream_t)stream, *grid, points, P, out_val,
                       out_grad, out_oob);
    return (int)hipGetLastError();
}

template <bool INTERP>
static int composed_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* points, int64_t P,
                        double* out_val, double* out_grad, int32_t* out_leaf, void* stream) {
    if (int e = check_composed<double>(grids, S, tf, A, points, P, out_val, out_grad)) return e;
    if (P == 0) return 0;
    // the kernel grid-strides over the points
    hipLaunchKernelGGL(composed_query_f64_kernel<INTERP>, dim3(A, config_rows(A, (P + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       grids, S, tf, A, points, P, out_val, out_grad, out_leaf);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int pvamd_cached_query_f64(const pvamd_grid_t* grid, const double* points, int64_t P, double* out_val,
                                      double* out_grad, uint8_t* out_oob, void* stream) {
    return cached_f64<false>(grid, points, P, out_val, out_grad, out_oob, stream);
}

extern "C" int pvamd_cached_query_interp_f64(const pvamd_grid_t* grid, const double* points, int64_t P, double* out_val,
                                             double* out_grad, uint8_t* out_oob, void* stream) {
    return cached_f64<true>(grid, points, P, out_val, out_grad, out_oob, stream);
}

extern "C" int pvamd_cached_query_interp(const pvamd_grid_t* grid, const float* points, int64_t P, float* out_val,
                                         float* out_grad, uint8_t* out_oob, void* stream) {
    if (int e = check_cached<float>(grid, points, P, out_val, out_grad)) return e;
    if (P == 0) return 0;
    dim3 blocks;
    if (int e = cached_lane_blocks(P, blocks)) return e;
    hipStream_t s = (hipStream_t)stream;
    if (out_oob)
        hipLaunchKernelGGL(cached_interp_kernel<true>, blocks, dim3(kLaneBlock), 0, s, *grid, points, P, out_val, out_grad, out_oob);
    else
        hipLaunchKernelGGL(cached_interp_kernel<false>, blocks, dim3(kLaneBlock), 0, s, *grid, points, P, out_val, out_grad, out_oob);
    return (int)hipGetLastError();
}

extern "C" int pvamd_composed_query_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                        const double* points, int64_t P, double* out_val, double* out_grad,
                                        int32_t* out_leaf, void* stream) {
    return composed_f64<false>(grids, S, tf, A, points, P, out_val, out_grad, out_leaf, stream);
}

extern "C" int pvamd_composed_query_interp_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                               const double* points, int64_t P, double* out_val, double* out_grad, int32_t* out_leaf,
                                               void* stream) {
    return composed_f64<true>(grids, S, tf, A, points, P, out_val, out_grad, out_leaf, stream);
}

extern "C" int pvamd_composed_query_interp(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                           int64_t P, float* out_val, float* out_grad, int32_t* out_leaf, void* stream) {
    if (int e = check_composed<float>(grids, S, tf, A, points, P, out_val, out_grad)) return e;
    if (P == 0) return 0;
    // point blocks in x (as many as the points need, at most the 2^31 - 1 HIP allows), configurations in y (grid_rows; more
    // are strided)
    int64_t bx = (P + kLaneBlock - 1) / kLaneBlock;
    if (bx > 0x7fffffff) bx = 0x7fffffff;
    hipLaunchKernelGGL(composed_interp_kernel, dim3((unsigned)bx, grid_rows(A)), dim3(kLaneBlock), 0,
                       (hipStream_t)stream, grids, S, tf, A, points, P, out_val, out_grad, out_leaf);
    return (int)hipGetLastError();
}
