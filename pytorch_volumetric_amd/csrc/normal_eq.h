// What the normal-equation kernels of registration.hip and articulated.hip share (include/pvamd.h "Chamfer normal equations",
// "Semantic normal equations", "Joint-space normal equations"): the statements of one pair, the second pass over the slab, and
// the host's arithmetic on chunks and slab bytes.  profiles/normal_eq_shared.md holds the per-kernel comparison with the copies.
#pragma once
#include "common.h"

namespace pvamd {

constexpr int kNeSums = PVAMD_REG_SUMS;      // 1 + 6 + 21: s0, s1, the upper triangle of s2
constexpr int kSemCounts = PVAMD_SEM_COUNTS;

// One (pose or leaf, point) pair: r the residual, x the point in the grid's frame, (n0, n1, n2) the record's gradient there.
// An inactive pair adds nothing; an active one enters as (q, u) = (r, j) or, past delta, (w r, w j): 28 fused multiply-adds
// into acc and the counts 1..4 (cnt[0], the range count, is the caller's).  Without SEMANTIC every pair is an active surface
// pair inside delta: kind, delta and cnt are not read, and what remains is s0 += r r, s1 += r j, s2 += j j^T.
template <bool SEMANTIC>
PVAMD_DEV void pair_sums(int kind, double r, const float* x, float n0, float n1, float n2, double delta, double* acc, int* cnt) {
    // written as the contract's inactive cases negated: a NaN r fails both comparisons and stays active
    const bool active = !SEMANTIC || kind == PVAMD_POINT_SURFACE || (kind == PVAMD_POINT_FREE && !(r >= 0.0)) ||
                        (kind == PVAMD_POINT_OCCUPIED && !(r <= 0.0));
    if (active) {
        double j[6], u[6];
        j[0] = (double)n0; j[1] = (double)n1; j[2] = (double)n2;
        // x cross n: each product of two float32 values is exact in float64, so each component rounds once
        j[3] = (double)x[1] * j[2] - (double)x[2] * j[1];
        j[4] = (double)x[2] * j[0] - (double)x[0] * j[2];
        j[5] = (double)x[0] * j[1] - (double)x[1] * j[0];
        const double a = __builtin_fabs(r);
        double q = r;
#pragma unroll
        for (int c = 0; c < 6; ++c) u[c] = j[c];
        const bool outlier = SEMANTIC && a > delta;
        if (outlier) {  // per lane: the one float64 division of the pass
            const double w = delta / a;
            acc[0] = __builtin_fma(delta, (a + a) - delta, acc[0]);
            q = w * r;
#pragma unroll
            for (int c = 0; c < 6; ++c) u[c] = w * j[c];
        } else {
            acc[0] = __builtin_fma(r, r, acc[0]);
        }
        if (SEMANTIC) {
            cnt[1] += kind == PVAMD_POINT_SURFACE;
            cnt[2] += kind == PVAMD_POINT_FREE;
            cnt[3] += kind == PVAMD_POINT_OCCUPIED;
            cnt[4] += outlier;
        }
        int e = 7;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            acc[1 + rr] = __builtin_fma(q, j[rr], acc[1 + rr]);
#pragma unroll
            for (int c = rr; c < 6; ++c, ++e) acc[e] = __builtin_fma(u[rr], j[c], acc[e]);
        }
    }
}

// Pass 2, one thread per (row, entry): the chunks' slab rows added in chunk order.  A row is a pose, or a (configuration, leaf)
// pair.  slab: double [nchunks][rows][28], slab_count: int64 [nchunks][rows][NCOUNTS]
template <int NCOUNTS>
__global__ __launch_bounds__(256) void normal_eq_finish_kernel(int64_t rows, int64_t nchunks, const double* __restrict__ slab,
                                                               const int64_t* __restrict__ slab_count,
                                                               double* __restrict__ out_sums, int64_t* __restrict__ out_counts) {
    const int64_t per = kNeSums + NCOUNTS, total = rows * per;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / per;
        const int e = (int)(t - b * per);
        if (e < kNeSums) {
            double s = 0.0;
            for (int64_t c = 0; c < nchunks; ++c) s += slab[(c * rows + b) * kNeSums + e];
            out_sums[b * kNeSums + e] = s;
        } else {
            int64_t n = 0;
            for (int64_t c = 0; c < nchunks; ++c) n += slab_count[(c * rows + b) * NCOUNTS + (e - kNeSums)];
            out_counts[b * NCOUNTS + (e - kNeSums)] = n;
        }
    }
}

// ---- host ----
constexpr int64_t normal_eq_chunks(int64_t N) { return (N + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK; }

// the slab of `rows` rows with `ncounts` counts each over N points: the doubles of every chunk, then the counts
constexpr int64_t normal_eq_slab_bytes(int64_t rows, int ncounts, int64_t N) {
    return 8 * (int64_t)(kNeSums + ncounts) * rows * normal_eq_chunks(N);
}
static_assert(PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES(3, 2 * PVAMD_REG_CHUNK + 1) == normal_eq_slab_bytes(3, 1, 2 * PVAMD_REG_CHUNK + 1) &&
                  PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES(1, PVAMD_REG_CHUNK) == normal_eq_slab_bytes(1, 1, PVAMD_REG_CHUNK),
              "the C interface's macro is this expression with one count");

static inline int64_t* normal_eq_slab_counts(void* scratch, int64_t rows, int64_t N) {
    return (int64_t*)((double*)scratch + normal_eq_chunks(N) * rows * kNeSums);
}

template <int NCOUNTS>
static inline void launch_normal_eq_finish(int64_t rows, int64_t N, void* scratch, double* out_sums, int64_t* out_counts,
                                           hipStream_t st) {
    hipLaunchKernelGGL(normal_eq_finish_kernel<NCOUNTS>, dim3(stream_grid(rows * (kNeSums + NCOUNTS), 256)), dim3(256), 0, st, rows,
                       normal_eq_chunks(N), (const double*)scratch, normal_eq_slab_counts(scratch, rows, N), out_sums, out_counts);
}

// the arguments the two Levenberg-Marquardt step entry points share
static inline bool lm_args_ok(int first, double up, double down, double lambda_min, double lambda_max) {
    return (first == 0 || first == 1) && up > 1.0 && down > 0.0 && down <= 1.0 && lambda_min > 0.0 &&
           lambda_max >= lambda_min && lambda_max < __builtin_inf();
}

}  // namespace pvamd
