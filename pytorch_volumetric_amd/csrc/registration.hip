// Gauss-Newton pose refinement against a cached voxel grid (include/pvamd.h "Chamfer normal equations"): the normal equations
// of sum_i (sdf(W[b] p_i))^2 over a left-multiplied twist of each pose, and the Levenberg-Marquardt step that uses them.
//
//   pass 1 (reg_partial_kernel)  workgroup (chunk, b): x = W[b] p (affine_row, the chamfer kernel's statements), (v, n) = the
//                                 cache's answer at x (MopLeaf, the leaf layer the queries share), j = (n, x cross n) in float64;
//                                 per lane 28 float64 accumulators (s0 = v v, s1 = v j, the upper triangle of j j^T) in point
//                                 order, one fused multiply-add per term; a wave butterfly, the four waves in order; one slab
//                                 row per (chunk, b)
//   pass 2 (reg_finish_kernel)   one thread per (b, entry): the chunks' rows added in chunk order
//   pose_lm_step_kernel          one thread per pose, float64: accept / reject, damped Cholesky solve, retraction
//   sem_partial_kernel, sem_finish_kernel ("Semantic normal equations")  passes 1 and 2 with a kind and a target distance per
//                                 point and Huber weights, in the same order; five counts per pose beside the 28 sums
// Every order depends only on (B, N): the result repeats bit for bit.  No float atomics, no host synchronisation.  The (B, N, 3)
// transformed cloud and the (B, N) field never reach HBM.
#include "common.h"
#include "composed_point.h"

namespace pvamd {

constexpr int kRegBlock = 256;
constexpr int kRegK = PVAMD_REG_CHUNK / kRegBlock;  // points per lane per chunk
static_assert(kRegK * kRegBlock == PVAMD_REG_CHUNK, "whole lanes per chunk");
constexpr int kRegSums = PVAMD_REG_SUMS;  // 1 + 6 + 21

// slab: double [nchunks][B][28], then int64 [nchunks][B].  The kernel does not read nchunks (the grid's x is the chunk); the
// argument stays: without it (one s_load narrower, other scalar registers) the nearest form ran 20.29 us against 20.15 at 64 x 16,384
// and 170.48 against 170.34 at 1 x 2^20, where a second build of the same source stood 0.02 and 0.01 us away
// (profiles/argument_prune.md).  Measured with ROCm 7.2 (clang 22) only: time it again after a compiler change
template <bool INTERP>
__global__ __launch_bounds__(kRegBlock) void reg_partial_kernel(const pvamd_grid_t g, const float* __restrict__ W, int B,
                                                                const float* __restrict__ pts, int64_t N, int64_t /*nchunks*/,
                                                                double* __restrict__ slab, int64_t* __restrict__ slab_count) {
    __shared__ double ws[kRegBlock / 64][kRegSums];
    __shared__ int wc[kRegBlock / 64];
    const int64_t chunk = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* M = W + 16 * (int64_t)b;  // wave-uniform: scalar loads
        double acc[kRegSums];
#pragma unroll
        for (int e = 0; e < kRegSums; ++e) acc[e] = 0.0;
        int cnt = 0;
#pragma unroll 1
        for (int k = 0; k < kRegK; ++k) {
            const int64_t i = chunk * PVAMD_REG_CHUNK + (int64_t)k * kRegBlock + threadIdx.x;
            if (i < N) {
                const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
                float x[3], o[4];
                LeafOps<float>::xform(M, p, x);
                MopLeaf<float, INTERP>::eval(g, x, o);
                cnt += in_range(g, x[0], x[1], x[2]);
                const double v = (double)o[0];
                double j[6];
                j[0] = (double)o[1]; j[1] = (double)o[2]; j[2] = (double)o[3];
                // x cross n: each product of two float32 values is exact in float64, so each component rounds once
                j[3] = (double)x[1] * j[2] - (double)x[2] * j[1];
                j[4] = (double)x[2] * j[0] - (double)x[0] * j[2];
                j[5] = (double)x[0] * j[1] - (double)x[1] * j[0];
                acc[0] = __builtin_fma(v, v, acc[0]);
                int e = 7;
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    acc[1 + r] = __builtin_fma(v, j[r], acc[1 + r]);
#pragma unroll
                    for (int c = r; c < 6; ++c, ++e) acc[e] = __builtin_fma(j[r], j[c], acc[e]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < kRegSums; ++e) acc[e] = hop_wave_sum<double>(acc[e]);
        cnt = hop_wave_sum<int>(cnt);
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < kRegSums; ++e) ws[wave][e] = acc[e];
            wc[wave] = cnt;
        }
        __syncthreads();
        if (threadIdx.x < kRegSums) {
            double s = ws[0][threadIdx.x];
            for (int w = 1; w < kRegBlock / 64; ++w) s += ws[w][threadIdx.x];
            slab[(chunk * B + b) * kRegSums + threadIdx.x] = s;
        } else if (threadIdx.x == kRegSums) {
            int c = wc[0];
            for (int w = 1; w < kRegBlock / 64; ++w) c += wc[w];
            slab_count[chunk * B + b] = c;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void reg_finish_kernel(int B, int64_t nchunks, const double* __restrict__ slab,
                                                         const int64_t* __restrict__ slab_count, double* __restrict__ out_sums,
                                                         int64_t* __restrict__ out_counts) {
    const int64_t per = kRegSums + 1, total = (int64_t)B * per;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / per;
        const int e = (int)(t - b * per);
        if (e < kRegSums) {
            double s = 0.0;
            for (int64_t c = 0; c < nchunks; ++c) s += slab[(c * B + b) * kRegSums + e];
            out_sums[b * kRegSums + e] = s;
        } else {
            int64_t n = 0;
            for (int64_t c = 0; c < nchunks; ++c) n += slab_count[c * B + b];
            out_counts[b] = n;
        }
    }
}

// ---- "Semantic normal equations": reg_partial_kernel with a kind and a target per point and Huber weights ----
// The same workgroup, chunk and lane-to-point assignment, so the same order of summation; per point one byte and one float more
// are loaded (a NULL kinds / targets is a wave-uniform branch).  An inactive pair skips its 28 statements; an active one enters
// them as (q, u) = (r, j) or, past delta, (w r, w j): with q = r and u = j they are reg_partial_kernel's own, bit for bit.
// slab: double [nchunks][B][28], then int64 [nchunks][B][5]
constexpr int kSemCounts = PVAMD_SEM_COUNTS;

template <bool INTERP>
__global__ __launch_bounds__(kRegBlock) void sem_partial_kernel(const pvamd_grid_t g, const float* __restrict__ W, int B,
                                                                const float* __restrict__ pts, int64_t N,
                                                                const uint8_t* __restrict__ kinds,
                                                                const float* __restrict__ targets, double delta,
                                                                double* __restrict__ slab, int64_t* __restrict__ slab_count) {
    __shared__ double ws[kRegBlock / 64][kRegSums];
    __shared__ int wc[kRegBlock / 64][kSemCounts];
    const int64_t chunk = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* M = W + 16 * (int64_t)b;  // wave-uniform: scalar loads
        double acc[kRegSums];
#pragma unroll
        for (int e = 0; e < kRegSums; ++e) acc[e] = 0.0;
        int cnt[kSemCounts];
#pragma unroll
        for (int e = 0; e < kSemCounts; ++e) cnt[e] = 0;
#pragma unroll 1
        for (int k = 0; k < kRegK; ++k) {
            const int64_t i = chunk * PVAMD_REG_CHUNK + (int64_t)k * kRegBlock + threadIdx.x;
            if (i < N) {
                const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
                const int kind = kinds ? (int)kinds[i] : PVAMD_POINT_SURFACE;
                const float target = targets ? targets[i] : 0.f;
                float x[3], o[4];
                LeafOps<float>::xform(M, p, x);
                MopLeaf<float, INTERP>::eval(g, x, o);
                cnt[0] += in_range(g, x[0], x[1], x[2]);
                const double r = (double)o[0] - (double)target;
                // written as the contract's inactive cases negated: a NaN r fails both comparisons and stays active
                const bool active = kind == PVAMD_POINT_SURFACE || (kind == PVAMD_POINT_FREE && !(r >= 0.0)) ||
                                    (kind == PVAMD_POINT_OCCUPIED && !(r <= 0.0));
                if (active) {
                    double j[6], u[6];
                    j[0] = (double)o[1]; j[1] = (double)o[2]; j[2] = (double)o[3];
                    // x cross n: each product of two float32 values is exact in float64, so each component rounds once
                    j[3] = (double)x[1] * j[2] - (double)x[2] * j[1];
                    j[4] = (double)x[2] * j[0] - (double)x[0] * j[2];
                    j[5] = (double)x[0] * j[1] - (double)x[1] * j[0];
                    const double a = __builtin_fabs(r);
                    double q = r;
#pragma unroll
                    for (int c = 0; c < 6; ++c) u[c] = j[c];
                    const bool outlier = a > delta;
                    if (outlier) {  // per lane: the one float64 division of the pass
                        const double w = delta / a;
                        acc[0] = __builtin_fma(delta, (a + a) - delta, acc[0]);
                        q = w * r;
#pragma unroll
                        for (int c = 0; c < 6; ++c) u[c] = w * j[c];
                    } else {
                        acc[0] = __builtin_fma(r, r, acc[0]);
                    }
                    cnt[1] += kind == PVAMD_POINT_SURFACE;
                    cnt[2] += kind == PVAMD_POINT_FREE;
                    cnt[3] += kind == PVAMD_POINT_OCCUPIED;
                    cnt[4] += outlier;
                    int e = 7;
#pragma unroll
                    for (int rr = 0; rr < 6; ++rr) {
                        acc[1 + rr] = __builtin_fma(q, j[rr], acc[1 + rr]);
#pragma unroll
                        for (int c = rr; c < 6; ++c, ++e) acc[e] = __builtin_fma(u[rr], j[c], acc[e]);
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < kRegSums; ++e) acc[e] = hop_wave_sum<double>(acc[e]);
#pragma unroll
        for (int e = 0; e < kSemCounts; ++e) cnt[e] = hop_wave_sum<int>(cnt[e]);
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < kRegSums; ++e) ws[wave][e] = acc[e];
#pragma unroll
            for (int e = 0; e < kSemCounts; ++e) wc[wave][e] = cnt[e];
        }
        __syncthreads();
        if (threadIdx.x < kRegSums) {
            double s = ws[0][threadIdx.x];
            for (int w = 1; w < kRegBlock / 64; ++w) s += ws[w][threadIdx.x];
            slab[(chunk * B + b) * kRegSums + threadIdx.x] = s;
        } else if (threadIdx.x < kRegSums + kSemCounts) {
            const int e = threadIdx.x - kRegSums;
            int c = wc[0][e];
            for (int w = 1; w < kRegBlock / 64; ++w) c += wc[w][e];
            slab_count[(chunk * B + b) * kSemCounts + e] = c;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void sem_finish_kernel(int B, int64_t nchunks, const double* __restrict__ slab,
                                                         const int64_t* __restrict__ slab_count, double* __restrict__ out_sums,
                                                         int64_t* __restrict__ out_counts) {
    const int64_t per = kRegSums + kSemCounts, total = (int64_t)B * per;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / per;
        const int e = (int)(t - b * per);
        if (e < kRegSums) {
            double s = 0.0;
            for (int64_t c = 0; c < nchunks; ++c) s += slab[(c * B + b) * kRegSums + e];
            out_sums[b * kRegSums + e] = s;
        } else {
            int64_t n = 0;
            for (int64_t c = 0; c < nchunks; ++c) n += slab_count[(c * B + b) * kSemCounts + (e - kRegSums)];
            out_counts[b * kSemCounts + (e - kRegSums)] = n;
        }
    }
}

// ---- the Levenberg-Marquardt step: one thread per pose, float64, every order fixed ----
__global__ __launch_bounds__(64) void pose_lm_step_kernel(int B, const double* __restrict__ sums, int first,
                                                          double* __restrict__ Wacc, double* __restrict__ sums_acc,
                                                          double* __restrict__ lambda, int32_t* __restrict__ accepted,
                                                          double* __restrict__ Wtry, float* __restrict__ W_next, double up,
                                                          double down, double lambda_min, double lambda_max) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* S = sums + (int64_t)b * kRegSums;
    double* SA = sums_acc + (int64_t)b * kRegSums;
    double* WA = Wacc + (int64_t)b * 12;
    double* WT = Wtry + (int64_t)b * 12;
    // 1. accept: strict, so a NaN never accepts
    double lam = lambda[b];
    if (first || S[0] < SA[0]) {
        for (int e = 0; e < 12; ++e) WA[e] = WT[e];
        for (int e = 0; e < kRegSums; ++e) SA[e] = S[e];
        lam = lam * down;
        lam = lam > lambda_min ? lam : lambda_min;
        accepted[b] += 1;
    } else {
        lam = lam * up;
        lam = lam < lambda_max ? lam : lambda_max;
    }
    // 2. solve (S2 + lam D) xi = -S1 with the accepted sums: Cholesky without pivoting
    double A[6][6], L[6][6], xi[6];
    {
        int e = 7;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c, ++e) A[r][c] = A[c][r] = SA[e];
    }
    for (int k = 0; k < 6; ++k) {
        const double d = A[k][k] > 0.0 ? A[k][k] : 1.0;  // an axis no point observes gets the unit: a zero step, not a failed pivot
        A[k][k] = __builtin_fma(lam, d, A[k][k]);
    }
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d = __builtin_fma(-L[j][k], L[j][k], d);
        if (!(d > 0.0) || !(d < __builtin_inf())) ok = false;
        const double ljj = __builtin_sqrt(d);
        L[j][j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = __builtin_fma(-L[i][k], L[j][k], s);
            L[i][j] = s / ljj;
        }
    }
    for (int i = 0; i < 6; ++i) {  // L y = -S1
        double s = -SA[1 + i];
        for (int k = 0; k < i; ++k) s = __builtin_fma(-L[i][k], xi[k], s);
        xi[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {  // L^T xi = y
        double s = xi[i];
        for (int k = i + 1; k < 6; ++k) s = __builtin_fma(-L[k][i], xi[k], s);
        xi[i] = s / L[i][i];
    }
    for (int i = 0; i < 6; ++i) ok = ok && (__builtin_fabs(xi[i]) < __builtin_inf());
    if (!ok) {
        for (int i = 0; i < 6; ++i) xi[i] = 0.0;
        lam = lam * up;
        lam = lam < lambda_max ? lam : lambda_max;
    }
    lambda[b] = lam;
    // 3. retract: Wtry = [Exp(w) R, Exp(w) t + u]; a zero step copies Wacc (adding zeros would turn a -0.0 entry into +0.0)
    bool zero = true;
    for (int i = 0; i < 6; ++i) zero = zero && (xi[i] == 0.0);
    if (zero) {
        for (int e = 0; e < 12; ++e) WT[e] = WA[e];
    } else {
        const double wx = xi[3], wy = xi[4], wz = xi[5];
        const double th2 = __builtin_fma(wz, wz, __builtin_fma(wy, wy, wx * wx));
        const double th = __builtin_sqrt(th2);
        double a, c;  // Exp(w) = I + a K + c K^2, a = sin th / th, c = (1 - cos th) / th^2 = (sin(th / 2) / (th / 2))^2 / 2
        if (th < 1e-8) {
            a = 1.0 - th2 / 6.0;
            c = 0.5 - th2 / 24.0;
        } else {
            a = sin(th) / th;
            const double h = 0.5 * th, q = sin(h) / h;
            c = 0.5 * (q * q);
        }
        // K = [[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]]; K^2 = w w^T - th^2 I
        double E[3][3];
        const double w[3] = {wx, wy, wz};
        for (int r = 0; r < 3; ++r)
            for (int s = 0; s < 3; ++s) E[r][s] = c * (w[r] * w[s]);
        E[0][0] = 1.0 - c * __builtin_fma(wz, wz, wy * wy);
        E[1][1] = 1.0 - c * __builtin_fma(wz, wz, wx * wx);
        E[2][2] = 1.0 - c * __builtin_fma(wy, wy, wx * wx);
        E[0][1] = __builtin_fma(-a, wz, E[0][1]); E[1][0] = __builtin_fma(a, wz, E[1][0]);
        E[0][2] = __builtin_fma(a, wy, E[0][2]);  E[2][0] = __builtin_fma(-a, wy, E[2][0]);
        E[1][2] = __builtin_fma(-a, wx, E[1][2]); E[2][1] = __builtin_fma(a, wx, E[2][1]);
        double T[12];
        for (int r = 0; r < 3; ++r) {
            for (int s = 0; s < 4; ++s)
                T[4 * r + s] = __builtin_fma(E[r][2], WA[8 + s], __builtin_fma(E[r][1], WA[4 + s], E[r][0] * WA[s]));
            T[4 * r + 3] += xi[r];
        }
        for (int e = 0; e < 12; ++e) WT[e] = T[e];
    }
    float* O = W_next + (int64_t)b * 16;
    for (int e = 0; e < 12; ++e) O[e] = (float)WT[e];
    O[12] = 0.f; O[13] = 0.f; O[14] = 0.f; O[15] = 1.f;
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_chamfer_normal_eq_scratch_bytes(int32_t B, int64_t N) {
    if (B < 1 || N < 1) return 0;
    return PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES(B, N);
}

extern "C" int pvamd_chamfer_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points,
                                       int64_t N, double* out_sums, int64_t* out_counts, void* scratch, void* stream) {
    if (B < 0 || N < 1 || (N + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK > 0x7fffffff) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    if (!grid) return PVAMD_E_NULL;
    if (int e = check_grid(*grid)) return e;
    if (grid->oob_mode != PVAMD_OOB_BOUNDING_BOX) return PVAMD_E_MODE;
    if (B == 0) return 0;
    if (!W || !points || !out_sums || !out_counts || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(W, 4) || !aligned_to(points, 4) || !aligned_to(out_sums, 8) || !aligned_to(out_counts, 8) ||
        !aligned_to(scratch, 8))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunks = (N + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK;
    double* slab = (double*)scratch;
    int64_t* slab_count = (int64_t*)(slab + nchunks * (int64_t)B * kRegSums);
    const dim3 grid_dim((unsigned)nchunks, grid_rows(B));
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((reg_partial_kernel<true>), grid_dim, dim3(kRegBlock), 0, st, *grid, W, B, points, N, nchunks, slab,
                           slab_count);
    else
        hipLaunchKernelGGL((reg_partial_kernel<false>), grid_dim, dim3(kRegBlock), 0, st, *grid, W, B, points, N, nchunks, slab,
                           slab_count);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(stream_grid((int64_t)B * (kRegSums + 1), 256)), dim3(256), 0, st, B, nchunks, slab,
                       slab_count, out_sums, out_counts);
    return (int)hipGetLastError();
}

extern "C" int64_t pvamd_semantic_normal_eq_scratch_bytes(int32_t B, int64_t N) {
    if (B < 1 || N < 1) return 0;
    return 8 * (int64_t)(kRegSums + kSemCounts) * B * ((N + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK);
}

extern "C" int pvamd_semantic_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points,
                                        int64_t N, const uint8_t* kinds, const float* targets, double huber_delta,
                                        double* out_sums, int64_t* out_counts, void* scratch, void* stream) {
    if (B < 0 || N < 1 || (N + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK > 0x7fffffff) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    if (!grid) return PVAMD_E_NULL;
    if (int e = check_grid(*grid)) return e;
    if (grid->oob_mode != PVAMD_OOB_BOUNDING_BOX) return PVAMD_E_MODE;
    if (!(huber_delta > 0.0)) return PVAMD_E_MODE;  // a NaN too
    if (B == 0) return 0;
    if (!W || !points || !out_sums || !out_counts || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(W, 4) || !aligned_to(points, 4) || !aligned_to(targets, 4) || !aligned_to(out_sums, 8) ||
        !aligned_to(out_counts, 8) || !aligned_to(scratch, 8))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunks = (N + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK;
    double* slab = (double*)scratch;
    int64_t* slab_count = (int64_t*)(slab + nchunks * (int64_t)B * kRegSums);
    const dim3 grid_dim((unsigned)nchunks, grid_rows(B));
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((sem_partial_kernel<true>), grid_dim, dim3(kRegBlock), 0, st, *grid, W, B, points, N, kinds, targets,
                           huber_delta, slab, slab_count);
    else
        hipLaunchKernelGGL((sem_partial_kernel<false>), grid_dim, dim3(kRegBlock), 0, st, *grid, W, B, points, N, kinds, targets,
                           huber_delta, slab, slab_count);
    hipLaunchKernelGGL(sem_finish_kernel, dim3(stream_grid((int64_t)B * (kRegSums + kSemCounts), 256)), dim3(256), 0, st, B,
                       nchunks, slab, slab_count, out_sums, out_counts);
    return (int)hipGetLastError();
}

extern "C" int pvamd_pose_lm_step(int32_t B, const double* sums, int32_t first, double* Wacc, double* sums_acc, double* lambda,
                                  int32_t* accepted, double* Wtry, float* W_next, double up, double down, double lambda_min,
                                  double lambda_max, void* stream) {
    if (B < 0) return PVAMD_E_SHAPE;
    if ((first != 0 && first != 1) || !(up > 1.0) || !(down > 0.0 && down <= 1.0) || !(lambda_min > 0.0) ||
        !(lambda_max >= lambda_min) || !(lambda_max < __builtin_inf()))
        return PVAMD_E_MODE;
    if (B == 0) return 0;
    if (!sums || !Wacc || !sums_acc || !lambda || !accepted || !Wtry || !W_next) return PVAMD_E_NULL;
    if (!aligned_to(sums, 8) || !aligned_to(Wacc, 8) || !aligned_to(sums_acc, 8) || !aligned_to(lambda, 8) ||
        !aligned_to(accepted, 4) || !aligned_to(Wtry, 8) || !aligned_to(W_next, 4))
        return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(pose_lm_step_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, B, sums, first, Wacc,
                       sums_acc, lambda, accepted, Wtry, W_next, up, down, lambda_min, lambda_max);
    return (int)hipGetLastError();
}
