// Gauss-Newton pose refinement against a cached voxel grid (include/pvamd.h "Chamfer normal equations"): the normal equations
// of sum_i (sdf(W[b] p_i))^2 over a left-multiplied twist of each pose, and the Levenberg-Marquardt step that uses them.
//
//   pass 1 (reg_partial_kernel)  workgroup (chunk, b): x = W[b] p (affine_row, the chamfer kernel's statements), (v, n) = the
//                                 cache's answer at x (MopLeaf, the leaf layer the queries share), j = (n, x cross n) in float64;
//                                 per lane 28 float64 accumulators (s0 = v v, s1 = v j, the upper triangle of j j^T) in point
//                                 order, one fused multiply-add per term; a wave butterfly, the four waves in order; one slab
//                                 row per (chunk, b)
//   pass 2 (normal_eq_finish_kernel, normal_eq.h)  one thread per (b, entry): the chunks' rows added in chunk order
//   pose_lm_step_kernel          one thread per pose, float64: accept / reject, damped Cholesky solve, retraction
//   sem_partial_kernel ("Semantic normal equations")  pass 1 with a kind and a target distance per point and Huber weights, in
//                                 the same order (one body, rigid_partial; the pair's statements are pair_sums, normal_eq.h);
//                                 five counts per pose beside the 28 sums
// Every order depends only on (B, N): the result repeats bit for bit.  No float atomics, no host synchronisation.  The (B, N, 3)
// transformed cloud and the (B, N) field never reach HBM.
#include "common.h"
#include "composed_point.h"
#include "normal_eq.h"

namespace pvamd {

constexpr int kRegBlock = 256;
constexpr int kRegK = PVAMD_REG_CHUNK / kRegBlock;  // points per lane per chunk
static_assert(kRegK * kRegBlock == PVAMD_REG_CHUNK, "whole lanes per chunk");
constexpr int kRegSums = kNeSums;

// Pass 1 of both rigid forms: the same workgroup, chunk and lane-to-point assignment, so the same order of summation.  SEMANTIC
// loads one byte and one float more per point (a NULL kinds / targets is a wave-uniform branch) and keeps five counts, not one.
// slab: double [nchunks][B][28], then int64 [nchunks][B][NC]
template <bool INTERP, bool SEMANTIC>
PVAMD_DEV void rigid_partial(const pvamd_grid_t& g, const float* __restrict__ W, int B, const float* __restrict__ pts, int64_t N,
                             const uint8_t* __restrict__ kinds, const float* __restrict__ targets, double delta,
                             double* __restrict__ slab, int64_t* __restrict__ slab_count) {
    constexpr int NC = SEMANTIC ? kSemCounts : 1;
    __shared__ double ws[kRegBlock / 64][kRegSums];
    __shared__ int wc[kRegBlock / 64][NC];
    const int64_t chunk = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* M = W + 16 * (int64_t)b;  // wave-uniform: scalar loads
        double acc[kRegSums];
#pragma unroll
        for (int e = 0; e < kRegSums; ++e) acc[e] = 0.0;
        int cnt[NC];
#pragma unroll
        for (int e = 0; e < NC; ++e) cnt[e] = 0;
#pragma unroll 1
        for (int k = 0; k < kRegK; ++k) {
            const int64_t i = chunk * PVAMD_REG_CHUNK + (int64_t)k * kRegBlock + threadIdx.x;
            if (i < N) {
                const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
                const int kind = SEMANTIC && kinds ? (int)kinds[i] : PVAMD_POINT_SURFACE;
                const float target = SEMANTIC && targets ? targets[i] : 0.f;
                float x[3], o[4];
                LeafOps<float>::xform(M, p, x);
                MopLeaf<float, INTERP>::eval(g, x, o);
                cnt[0] += in_range(g, x[0], x[1], x[2]);
                const double r = SEMANTIC ? (double)o[0] - (double)target : (double)o[0];
                pair_sums<SEMANTIC>(kind, r, x, o[1], o[2], o[3], delta, acc, cnt);
            }
        }
#pragma unroll
        for (int e = 0; e < kRegSums; ++e) acc[e] = hop_wave_sum<double>(acc[e]);
#pragma unroll
        for (int e = 0; e < NC; ++e) cnt[e] = hop_wave_sum<int>(cnt[e]);
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < kRegSums; ++e) ws[wave][e] = acc[e];
#pragma unroll
            for (int e = 0; e < NC; ++e) wc[wave][e] = cnt[e];
        }
        __syncthreads();
        if (threadIdx.x < kRegSums) {
            double s = ws[0][threadIdx.x];
            for (int w = 1; w < kRegBlock / 64; ++w) s += ws[w][threadIdx.x];
            slab[(chunk * B + b) * kRegSums + threadIdx.x] = s;
        } else if (threadIdx.x < kRegSums + NC) {
            const int e = threadIdx.x - kRegSums;
            int c = wc[0][e];
            for (int w = 1; w < kRegBlock / 64; ++w) c += wc[w][e];
            slab_count[(chunk * B + b) * NC + e] = c;
        }
        __syncthreads();
    }
}

// The kernel does not read nchunks (the grid's x is the chunk); the argument stays: without it (one s_load narrower, other
// scalar registers) the nearest form ran 20.29 us against 20.15 at 64 x 16,384 and 170.48 against 170.34 at 1 x 2^20, where a
// second build of the same source stood 0.02 and 0.01 us away (profiles/argument_prune.md).  Measured with ROCm 7.2 (clang 22)
// only: time it again after a compiler change
template <bool INTERP>
__global__ __launch_bounds__(kRegBlock) void reg_partial_kernel(const pvamd_grid_t g, const float* __restrict__ W, int B,
                                                                const float* __restrict__ pts, int64_t N, int64_t /*nchunks*/,
                                                                double* __restrict__ slab, int64_t* __restrict__ slab_count) {
    rigid_partial<INTERP, false>(g, W, B, pts, N, nullptr, nullptr, 0.0, slab, slab_count);
}

// "Semantic normal equations": a kind and a target per point and Huber weights
template <bool INTERP>
__global__ __launch_bounds__(kRegBlock) void sem_partial_kernel(const pvamd_grid_t g, const float* __restrict__ W, int B,
                                                                const float* __restrict__ pts, int64_t N,
                                                                const uint8_t* __restrict__ kinds,
                                                                const float* __restrict__ targets, double delta,
                                                                double* __restrict__ slab, int64_t* __restrict__ slab_count) {
    rigid_partial<INTERP, true>(g, W, B, pts, N, kinds, targets, delta, slab, slab_count);
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

// the validation and the two launches of both rigid entry points; the plain one has no kinds, no targets and delta = inf
template <bool SEMANTIC>
static int rigid_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points, int64_t N,
                           const uint8_t* kinds, const float* targets, double huber_delta, double* out_sums, int64_t* out_counts,
                           void* scratch, hipStream_t st) {
    if (B < 0 || N < 1 || normal_eq_chunks(N) > 0x7fffffff) return PVAMD_E_SHAPE;
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
    const int64_t nchunks = normal_eq_chunks(N);
    double* slab = (double*)scratch;
    int64_t* slab_count = normal_eq_slab_counts(scratch, B, N);
    const dim3 grid_dim((unsigned)nchunks, grid_rows(B));
    const bool interp = mode == PVAMD_LEAF_TRILINEAR;
    if constexpr (SEMANTIC) {
        hipLaunchKernelGGL(interp ? sem_partial_kernel<true> : sem_partial_kernel<false>, grid_dim, dim3(kRegBlock), 0, st, *grid, W, B,
                           points, N, kinds, targets, huber_delta, slab, slab_count);
    } else {
        hipLaunchKernelGGL(interp ? reg_partial_kernel<true> : reg_partial_kernel<false>, grid_dim, dim3(kRegBlock), 0, st, *grid, W, B,
                           points, N, nchunks, slab, slab_count);
    }
    launch_normal_eq_finish<SEMANTIC ? kSemCounts : 1>(B, N, scratch, out_sums, out_counts, st);
    return (int)hipGetLastError();
}

extern "C" int64_t pvamd_chamfer_normal_eq_scratch_bytes(int32_t B, int64_t N) {
    return B < 1 || N < 1 ? 0 : normal_eq_slab_bytes(B, 1, N);
}

extern "C" int pvamd_chamfer_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points,
                                       int64_t N, double* out_sums, int64_t* out_counts, void* scratch, void* stream) {
    return rigid_normal_eq<false>(grid, mode, W, B, points, N, nullptr, nullptr, __builtin_inf(), out_sums, out_counts, scratch,
                                  (hipStream_t)stream);
}

extern "C" int64_t pvamd_semantic_normal_eq_scratch_bytes(int32_t B, int64_t N) {
    return B < 1 || N < 1 ? 0 : normal_eq_slab_bytes(B, kSemCounts, N);
}

extern "C" int pvamd_semantic_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points,
                                        int64_t N, const uint8_t* kinds, const float* targets, double huber_delta,
                                        double* out_sums, int64_t* out_counts, void* scratch, void* stream) {
    return rigid_normal_eq<true>(grid, mode, W, B, points, N, kinds, targets, huber_delta, out_sums, out_counts, scratch,
                                 (hipStream_t)stream);
}

extern "C" int pvamd_pose_lm_step(int32_t B, const double* sums, int32_t first, double* Wacc, double* sums_acc, double* lambda,
                                  int32_t* accepted, double* Wtry, float* W_next, double up, double down, double lambda_min,
                                  double lambda_max, void* stream) {
    if (B < 0) return PVAMD_E_SHAPE;
    if (!lm_args_ok(first, up, down, lambda_min, lambda_max)) return PVAMD_E_MODE;
    if (B == 0) return 0;
    if (!sums || !Wacc || !sums_acc || !lambda || !accepted || !Wtry || !W_next) return PVAMD_E_NULL;
    if (!aligned_to(sums, 8) || !aligned_to(Wacc, 8) || !aligned_to(sums_acc, 8) || !aligned_to(lambda, 8) ||
        !aligned_to(accepted, 4) || !aligned_to(Wtry, 8) || !aligned_to(W_next, 4))
        return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(pose_lm_step_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, B, sums, first, Wacc,
                       sums_acc, lambda, accepted, Wtry, W_next, up, down, lambda_min, lambda_max);
    return (int)hipGetLastError();
}
