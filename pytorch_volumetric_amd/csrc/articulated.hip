// Gauss-Newton refinement of a robot's joint values against a point cloud (include/pvamd.h "Joint-space normal equations"):
// the articulated sibling of registration.hip.  Every point is won by exactly one leaf and a link's twist Jacobian does not
// depend on the point, so the joint-space normal equations factor exactly over the leaves,
//     H_q = sum_s J_s^T H6_s J_s,   g_q = sum_s J_s^T g6_s,   cost = sum_s c_s,
// with (c_s, g6_s, H6_s) the 28 sums of "Semantic normal equations" over the points leaf s wins, in leaf s's frame.
//
//   joint_partial_kernel   workgroup (chunk, a): per point one composed walk (mop_point's statements) that keeps the winner and
//                          its record; then, per leaf that won a point of the wave, the 28 statements of pair_sums over the
//                          lane's points of that leaf in point order, a wave butterfly, the four waves in order; one slab row
//                          per (chunk, a, leaf).  A wave without a point of leaf s adds +0.0 and skips that leaf's butterflies
//   normal_eq_finish_kernel (normal_eq.h)  one thread per (a, leaf, entry): the chunks' rows added in chunk order
//   chain_twists_kernel    lane = configuration, blockIdx.y = leaf: the float64 chain walk and the 6 x M twist Jacobian J[a][s]
//   joint_assemble_kernel  one thread per (a, entry of cost | gradient | upper triangle): the leaves in order, fused multiply-adds
//   joint_lm_step_kernel   one wave per configuration, the damped matrix in LDS: pose_lm_step_kernel's decisions in joint space
// Every order depends only on (A, S, M, N): the result repeats bit for bit.  No float atomics, no host synchronisation; no
// (A, N) buffer reaches HBM.
#include "common.h"
#include "composed_point.h"
#include "normal_eq.h"

namespace pvamd {

constexpr int kJntBlock = 256;
constexpr int kJntK = PVAMD_REG_CHUNK / kJntBlock;  // points per lane per chunk
static_assert(kJntK * kJntBlock == PVAMD_REG_CHUNK, "whole lanes per chunk");
constexpr int kJntSums = kNeSums;
constexpr int kJntCounts = kSemCounts;
constexpr int kJntWaves = kJntBlock / 64;
static_assert(PVAMD_JOINT_MAX_LEAVES <= 64, "the leaves a wave saw are one 64-bit mask");
static_assert(PVAMD_JOINT_MAX_LEAVES < 255, "winner and range bit share one register");

// the OR of a 64-bit mask over the wave, as two scalar halves
PVAMD_DEV uint64_t wave_or(uint64_t m) {
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, off, 64);
        hi |= (uint32_t)__shfl_xor((int)hi, off, 64);
    }
    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
    return ((uint64_t)hi << 32) | lo;
}

// The composed walk of kJntWalk of a lane's points at once: mop_point's float32 statements, keeping per point the value, the
// winner's own record gradient and (winner | in range << 8).  All eight points of a lane are in flight at once: the kernel
// runs one wave per SIMD (the binning below holds the registers, whatever this width is), so the gathers are hidden by these
constexpr int kJntWalk = 8;
static_assert(kJntK % kJntWalk == 0, "whole walks per lane");

template <bool INTERP>
PVAMD_DEV void walk_points(const pvamd_grid_t* __restrict__ grids, int S, const float* __restrict__ tf, int A, int a,
                           const float (*p)[3], float* bv, float (*lg)[3], int* win) {
    for (int s = 0; s < S; ++s) {
        const float* M = tf + 16 * ((int64_t)s * A + a);  // wave-uniform: scalar loads
#pragma unroll
        for (int k = 0; k < kJntWalk; ++k) {
            float x[3], o[4];
            LeafOps<float>::xform(M, p[k], x);
            MopLeaf<float, INTERP>::eval(grids[s], x, o);
            const bool take = !(o[0] >= bv[k]) & (bv[k] == bv[k]);
            const int cand = s | ((int)in_range(grids[s], x[0], x[1], x[2]) << 8);
            bv[k] = take ? o[0] : bv[k];
            lg[k][0] = take ? o[1] : lg[k][0];
            lg[k][1] = take ? o[2] : lg[k][1];
            lg[k][2] = take ? o[3] : lg[k][2];
            win[k] = take ? cand : win[k];
        }
    }
}

// slab: double [nchunks][A][S][28], then int64 [nchunks][A][S][5].  LDS: double ws[4][S][28], then int wc[4][S][5]
template <bool INTERP>
__global__ __launch_bounds__(kJntBlock) void joint_partial_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                  const float* __restrict__ tf, int A,
                                                                  const float* __restrict__ pts, int64_t N,
                                                                  const uint8_t* __restrict__ kinds,
                                                                  const float* __restrict__ targets, double delta,
                                                                  double* __restrict__ slab, int64_t* __restrict__ slab_count) {
    extern __shared__ double jnt_lds[];
    double* ws = jnt_lds;
    int* wc = reinterpret_cast<int*>(ws + kJntWaves * S * kJntSums);
    const int64_t chunk = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the lane's points: the same for every configuration
    float p[kJntK][3], tg[kJntK];
    uint32_t kindbits = 0;  // two bits per point: every kind from PVAMD_POINT_IGNORE up is IGNORE
    bool live[kJntK];
#pragma unroll
    for (int k = 0; k < kJntK; ++k) {
        const int64_t i = chunk * PVAMD_REG_CHUNK + (int64_t)k * kJntBlock + threadIdx.x;
        live[k] = i < N;
        const int64_t ic = live[k] ? i : N - 1;  // a lane past the end walks the last point and bins nothing
        p[k][0] = pts[3 * ic]; p[k][1] = pts[3 * ic + 1]; p[k][2] = pts[3 * ic + 2];
        const uint32_t kd = kinds ? (uint32_t)kinds[ic] : (uint32_t)PVAMD_POINT_SURFACE;
        kindbits |= (kd < PVAMD_POINT_IGNORE ? kd : (uint32_t)PVAMD_POINT_IGNORE) << (2 * k);
        tg[k] = targets ? targets[ic] : 0.f;
    }
    for (int a = blockIdx.y; a < A; a += gridDim.y) {
        for (int e = threadIdx.x; e < kJntWaves * S * kJntSums; e += kJntBlock) ws[e] = 0.0;
        for (int e = threadIdx.x; e < kJntWaves * S * kJntCounts; e += kJntBlock) wc[e] = 0;
        // 1. the walk: first minimum, a NaN counts as the minimum; kept per point: the value, the winner's own record gradient,
        //    and (winner | in range << 8)
        float bv[kJntK], lg[kJntK][3];
        int win[kJntK];
#pragma unroll
        for (int k = 0; k < kJntK; ++k) {
            bv[k] = __builtin_inff();
            lg[k][0] = lg[k][1] = lg[k][2] = __builtin_nanf("");
            win[k] = 0;
        }
#pragma unroll
        for (int k0 = 0; k0 < kJntK; k0 += kJntWalk) walk_points<INTERP>(grids, S, tf, A, a, p + k0, bv + k0, lg + k0, win + k0);
        uint64_t seen = 0;
#pragma unroll
        for (int k = 0; k < kJntK; ++k) {
            seen |= live[k] ? (1ull << (win[k] & 63)) : 0ull;
            win[k] = live[k] ? win[k] : -1;
        }
        seen = wave_or(seen);
        __syncthreads();  // the zeroes above, before any wave's sums
        // 2. per leaf the wave saw, in leaf order: the lane's pairs of that leaf in point order
        while (seen) {
            const int s = __builtin_ctzll(seen);
            seen &= seen - 1;
            const float* M = tf + 16 * ((int64_t)s * A + a);
            double acc[kJntSums];
#pragma unroll
            for (int e = 0; e < kJntSums; ++e) acc[e] = 0.0;
            int cnt[kJntCounts];
#pragma unroll
            for (int e = 0; e < kJntCounts; ++e) cnt[e] = 0;
#pragma unroll
            for (int k = 0; k < kJntK; ++k) {
                if ((win[k] & 0xff) == s && win[k] >= 0) {
                    const int kind = (int)((kindbits >> (2 * k)) & 3u);
                    const float target = tg[k];
                    float x[3];
                    LeafOps<float>::xform(M, p[k], x);  // the walk's own statement: the same bits
                    cnt[0] += win[k] >> 8;
                    // the float32 record as this iteration's own values: without the empty statements the widening to float64
                    // of all eight points' records is hoisted out of the leaf loop, 64 registers held across it
                    float v = bv[k], n0 = lg[k][0], n1 = lg[k][1], n2 = lg[k][2];
                    asm volatile("" : "+v"(v), "+v"(n0), "+v"(n1), "+v"(n2));
                    pair_sums<true>(kind, (double)v - (double)target, x, n0, n1, n2, delta, acc, cnt);
                }
            }
#pragma unroll
            for (int e = 0; e < kJntSums; ++e) acc[e] = hop_wave_sum<double>(acc[e]);
#pragma unroll
            for (int e = 0; e < kJntCounts; ++e) cnt[e] = hop_wave_sum<int>(cnt[e]);
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < kJntSums; ++e) ws[(wave * S + s) * kJntSums + e] = acc[e];
#pragma unroll
                for (int e = 0; e < kJntCounts; ++e) wc[(wave * S + s) * kJntCounts + e] = cnt[e];
            }
        }
        __syncthreads();
        const int64_t row = (chunk * A + a) * S;
        for (int t = threadIdx.x; t < S * kJntSums; t += kJntBlock) {
            double sum = ws[t];
            for (int w = 1; w < kJntWaves; ++w) sum += ws[w * S * kJntSums + t];
            slab[row * kJntSums + t] = sum;
        }
        for (int t = threadIdx.x; t < S * kJntCounts; t += kJntBlock) {
            int c = wc[t];
            for (int w = 1; w < kJntWaves; ++w) c += wc[w * S * kJntCounts + t];
            slab_count[row * kJntCounts + t] = c;
        }
        __syncthreads();
    }
}

// ---- the twist Jacobian: a float64 chain walk per (configuration, leaf) ----
// W = W @ B for 3x4 affine matrices (implicit last row 0 0 0 1), k-ordered fused multiply-adds
PVAMD_DEV void compose64(double* W, const double* B) {
    double C[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double acc = W[4 * i] * B[j];
            acc = __builtin_fma(W[4 * i + 1], B[4 + j], acc);
            acc = __builtin_fma(W[4 * i + 2], B[8 + j], acc);
            if (j == 3) acc += W[4 * i + 3];
            C[4 * i + j] = acc;
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) W[e] = C[e];
}

// W = W @ origin @ motion(q) of one record: chain_fk_kernel's statements in float64, sin and cos in float64
PVAMD_DEV void walk_record(const pvamd_joint_t& R, const float* __restrict__ q, int64_t a, int M, double* W) {
    double B[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) B[e] = (double)R.origin[e];
    compose64(W, B);
    if (R.jtype == 1) {
        const double th = (double)q[a * M + R.jcol];
        const double s = sin(th), c = cos(th);
        const double x = (double)R.axis[0], y = (double)R.axis[1], z = (double)R.axis[2];
        const double t = 1.0 - c;
        const double tx = t * x, ty = t * y, tz = t * z;
        B[0] = __builtin_fma(tx, x, c);        B[1] = __builtin_fma(tx, y, -(s * z)); B[2] = __builtin_fma(tx, z, s * y);    B[3] = 0.0;
        B[4] = __builtin_fma(tx, y, s * z);    B[5] = __builtin_fma(ty, y, c);        B[6] = __builtin_fma(ty, z, -(s * x)); B[7] = 0.0;
        B[8] = __builtin_fma(tx, z, -(s * y)); B[9] = __builtin_fma(ty, z, s * x);    B[10] = __builtin_fma(tz, z, c);       B[11] = 0.0;
        compose64(W, B);
    } else if (R.jtype == 2) {
        const double d = (double)q[a * M + R.jcol];
#pragma unroll
        for (int e = 0; e < 12; ++e) B[e] = (e % 5 == 0) ? 1.0 : 0.0;
        B[3] = (double)R.axis[0] * d; B[7] = (double)R.axis[1] * d; B[11] = (double)R.axis[2] * d;
        compose64(W, B);
    }
}

PVAMD_DEV void rotate64(const double* T, const double v[3], double o[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = __builtin_fma(T[4 * r + 2], v[2], __builtin_fma(T[4 * r + 1], v[1], T[4 * r] * v[0]));
}

PVAMD_DEV void cross64(const double a[3], const double b[3], double o[3]) {
    o[0] = __builtin_fma(a[1], b[2], -(a[2] * b[1]));
    o[1] = __builtin_fma(a[2], b[0], -(a[0] * b[2]));
    o[2] = __builtin_fma(a[0], b[1], -(a[1] * b[0]));
}

// J: double [A][S][6][M].  LDS: the records of the leaf's frame and its ancestors, leaf first
__global__ __launch_bounds__(64) void chain_twists_kernel(const pvamd_joint_t* __restrict__ joints, int F,
                                                          const float* __restrict__ q, int A, int M,
                                                          const float* __restrict__ offset_inv, int S, double* __restrict__ J) {
    extern __shared__ int path[];
    __shared__ int depth_lds;
    const int s = blockIdx.y;
    if (threadIdx.x == 0) {
        int f = -1;
        for (int i = 0; i < F; ++i) f = joints[i].leaf_slot == s ? i : f;
        int d = 0;
        for (; f >= 0 && d < F; f = joints[f].parent) path[d++] = f;
        depth_lds = d;
    }
    __syncthreads();
    const int depth = depth_lds;
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    double* out = J + (a * S + s) * 6 * (int64_t)M;
    for (int e = 0; e < 6 * M; ++e) out[e] = 0.0;  // the joints that are no ancestor of the leaf
    // pass 1: the leaf's frame, and T = offset_inv[s] @ rigid_inverse(world)
    double W[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) W[e] = (e % 5 == 0) ? 1.0 : 0.0;
    for (int d = depth - 1; d >= 0; --d) walk_record(joints[path[d]], q, a, M, W);
    double T[12];
    {
        double B[12];  // rigid_inverse(world): R^T, -(R^T t)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) B[4 * r + c] = W[4 * c + r];
            B[4 * r + 3] = -__builtin_fma(W[8 + r], W[11], __builtin_fma(W[4 + r], W[7], W[r] * W[3]));
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = (double)offset_inv[16 * (int64_t)s + e];
        compose64(T, B);
    }
    const double t[3] = {T[3], T[7], T[11]};
    // pass 2: the same walk; at every moving joint on the way its twist in the object frame, carried into the leaf frame
#pragma unroll
    for (int e = 0; e < 12; ++e) W[e] = (e % 5 == 0) ? 1.0 : 0.0;
    for (int d = depth - 1; d >= 0; --d) {
        const pvamd_joint_t& R = joints[path[d]];
        walk_record(R, q, a, M, W);
        if (R.jtype != 1 && R.jtype != 2) continue;
        const double ax[3] = {(double)R.axis[0], (double)R.axis[1], (double)R.axis[2]};
        double ah[3], u[3], w[3];
        rotate64(W, ax, ah);
        if (R.jtype == 1) {  // revolute / continuous: (o cross a, a)
            const double o[3] = {W[3], W[7], W[11]};
            cross64(o, ah, u);
            w[0] = ah[0]; w[1] = ah[1]; w[2] = ah[2];
        } else {  // prismatic: (a, 0)
            u[0] = ah[0]; u[1] = ah[1]; u[2] = ah[2];
            w[0] = w[1] = w[2] = 0.0;
        }
        double Ru[3], Rw[3], tw[3];
        rotate64(T, u, Ru);
        rotate64(T, w, Rw);
        cross64(t, Rw, tw);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out[(int64_t)r * M + R.jcol] = -(Ru[r] + tw[r]);
            out[(int64_t)(3 + r) * M + R.jcol] = -Rw[r];
        }
    }
}

// ---- assembly: sums [A][1 + M + M (M + 1) / 2], counts [A][5 + S] ----
PVAMD_DEV int tri6(int r, int c) {  // the packed upper triangle of the 6 x 6 sums, row-major, r <= c
    return r * 6 - r * (r - 1) / 2 + (c - r);
}

__global__ __launch_bounds__(256) void joint_assemble_kernel(const double* __restrict__ leaf_sums,
                                                             const int64_t* __restrict__ leaf_counts,
                                                             const double* __restrict__ J, int A, int S, int M,
                                                             double* __restrict__ sums, int64_t* __restrict__ counts) {
    const int64_t P = 1 + (int64_t)M + (int64_t)M * (M + 1) / 2, C = kJntCounts + S, per = P + C;
    const int64_t total = (int64_t)A * per;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = t / per;
        const int64_t e = t - a * per;
        const double* L = leaf_sums + a * S * kJntSums;
        const int64_t* LC = leaf_counts + a * S * kJntCounts;
        const double* Ja = J + a * S * 6 * (int64_t)M;
        if (e == 0) {
            double c = 0.0;
            for (int s = 0; s < S; ++s) c += L[s * kJntSums];
            sums[a * P] = c;
        } else if (e <= M) {
            const int k = (int)e - 1;
            double g = 0.0;
            for (int s = 0; s < S; ++s)
                for (int r = 0; r < 6; ++r) g = __builtin_fma(Ja[((int64_t)s * 6 + r) * M + k], L[s * kJntSums + 1 + r], g);
            sums[a * P + e] = g;
        } else if (e < P) {
            // entry (i, j), i <= j, of the packed upper triangle, row-major
            int i = 0, rest = (int)(e - 1 - M);
            while (rest >= M - i) { rest -= M - i; ++i; }
            const int j = i + rest;
            double h = 0.0;
            for (int s = 0; s < S; ++s) {
                const double* Js = Ja + (int64_t)s * 6 * M;
                const double* H6 = L + s * kJntSums + 7;
                for (int r = 0; r < 6; ++r) {
                    double v = 0.0;  // (H6 J)[r][j]
                    for (int c = 0; c < 6; ++c) v = __builtin_fma(H6[r <= c ? tri6(r, c) : tri6(c, r)], Js[(int64_t)c * M + j], v);
                    h = __builtin_fma(Js[(int64_t)r * M + i], v, h);
                }
            }
            sums[a * P + e] = h;
        } else {
            const int c = (int)(e - P);
            int64_t n = 0;
            if (c < kJntCounts) {
                for (int s = 0; s < S; ++s) n += LC[s * kJntCounts + c];
            } else {
                const int s = c - kJntCounts;
                n = LC[s * kJntCounts + 1] + LC[s * kJntCounts + 2] + LC[s * kJntCounts + 3];
            }
            counts[a * C + c] = n;
        }
    }
}

// ---- the Levenberg-Marquardt step in joint space: one wave per configuration, lane = joint ----
constexpr int kStepLd = PVAMD_JOINT_MAX + 1;  // row stride of the matrix in LDS

__global__ __launch_bounds__(64) void joint_lm_step_kernel(int M, const double* __restrict__ sums, int first,
                                                           double* __restrict__ q_acc, double* __restrict__ sums_acc,
                                                           double* __restrict__ lambda, int32_t* __restrict__ accepted,
                                                           double* __restrict__ q_try, float* __restrict__ q_next,
                                                           const double* __restrict__ limits, double up, double down,
                                                           double lambda_min, double lambda_max) {
    __shared__ double Lm[PVAMD_JOINT_MAX * kStepLd];  // the damped matrix, then its Cholesky factor in the lower triangle
    __shared__ double xi[PVAMD_JOINT_MAX];
    const int a = blockIdx.x, k = threadIdx.x;
    const int64_t P = 1 + (int64_t)M + (int64_t)M * (M + 1) / 2;
    const double* Sn = sums + a * P;
    double* SA = sums_acc + a * P;
    // 1. accept: strict, so a NaN never accepts
    const bool accept = first || Sn[0] < SA[0];
    double lam = lambda[a];
    if (accept) {
        lam = lam * down;
        lam = lam > lambda_min ? lam : lambda_min;
    } else {
        lam = lam * up;
        lam = lam < lambda_max ? lam : lambda_max;
    }
    const double* src = accept ? Sn : SA;  // the accepted sums
    double qa = 0.0;
    if (k < M) {
        qa = accept ? q_try[(int64_t)a * M + k] : q_acc[(int64_t)a * M + k];
        int e = 1 + M;
        for (int i = 0; i < k; ++i) e += M - i;
        for (int c = k; c < M; ++c, ++e) Lm[k * kStepLd + c] = Lm[c * kStepLd + k] = src[e];
    }
    const double gk = k < M ? src[1 + k] : 0.0;
    __syncthreads();
    if (accept) {  // (after every lane has read the old sums_acc row it needed: none does when accepting)
        for (int64_t e = k; e < P; e += 64) SA[e] = Sn[e];
        if (k < M) q_acc[(int64_t)a * M + k] = qa;
        if (k == 0) accepted[a] += 1;
    }
    // 2. (H + lam D) dq = -g with the accepted sums: Cholesky without pivoting, row i on lane i, each entry's own chain in order
    if (k < M) {
        const double d0 = Lm[k * kStepLd + k];
        const double d = d0 > 0.0 ? d0 : 1.0;  // a joint no point observes gets the unit: a zero step, not a failed pivot
        Lm[k * kStepLd + k] = __builtin_fma(lam, d, d0);
    }
    __syncthreads();
    bool ok = true;
    for (int j = 0; j < M; ++j) {
        double d = Lm[j * kStepLd + j];
        for (int c = 0; c < j; ++c) d = __builtin_fma(-Lm[j * kStepLd + c], Lm[j * kStepLd + c], d);
        if (!(d > 0.0) || !(d < __builtin_inf())) ok = false;
        const double ljj = __builtin_sqrt(d);
        double lij = 0.0;
        if (k > j && k < M) {
            double s = Lm[k * kStepLd + j];
            for (int c = 0; c < j; ++c) s = __builtin_fma(-Lm[k * kStepLd + c], Lm[j * kStepLd + c], s);
            lij = s / ljj;
        }
        __syncthreads();  // every lane has read row j's diagonal
        if (k == j) Lm[j * kStepLd + j] = ljj;
        if (k > j && k < M) Lm[k * kStepLd + j] = lij;
        __syncthreads();
    }
    // L y = -g, then L^T dq = y: every lane walks both in the serial order (the values are wave-uniform LDS reads)
    for (int i = 0; i < M; ++i) {
        double s = -__shfl(gk, i, 64);
        for (int c = 0; c < i; ++c) s = __builtin_fma(-Lm[i * kStepLd + c], xi[c], s);
        __syncthreads();
        if (k == 0) xi[i] = s / Lm[i * kStepLd + i];
        __syncthreads();
    }
    for (int i = M - 1; i >= 0; --i) {
        double s = xi[i];
        for (int c = i + 1; c < M; ++c) s = __builtin_fma(-Lm[c * kStepLd + i], xi[c], s);
        __syncthreads();
        if (k == 0) xi[i] = s / Lm[i * kStepLd + i];
        __syncthreads();
    }
    bool zero = true;
    for (int i = 0; i < M; ++i) {
        ok = ok && (__builtin_fabs(xi[i]) < __builtin_inf());
        zero = zero && (xi[i] == 0.0);
    }
    if (!ok) {
        zero = true;
        lam = lam * up;
        lam = lam < lambda_max ? lam : lambda_max;
    }
    if (k == 0) lambda[a] = lam;
    // 3. q_try = q_acc + dq, clamped; a zero step copies q_acc
    if (k < M) {
        double qt = qa;
        if (!zero) {
            qt = qa + xi[k];
            if (limits) {
                const double lo = limits[2 * k], hi = limits[2 * k + 1];
                qt = qt < lo ? lo : qt;
                qt = qt > hi ? hi : qt;
            }
        }
        q_try[(int64_t)a * M + k] = qt;
        q_next[(int64_t)a * M + k] = (float)qt;
    }
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_joint_normal_eq_scratch_bytes(int32_t A, int32_t S, int64_t N) {
    return A < 1 || S < 1 || N < 1 ? 0 : normal_eq_slab_bytes((int64_t)A * S, kJntCounts, N);
}

extern "C" int pvamd_joint_normal_eq(const pvamd_grid_t* grids, int32_t S, int32_t mode, const float* stack, int32_t A,
                                     const float* points, int64_t N, const uint8_t* kinds, const float* targets,
                                     double huber_delta, double* leaf_sums, int64_t* leaf_counts, void* scratch, void* stream) {
    if (A < 0 || S < 1 || S > PVAMD_JOINT_MAX_LEAVES || N < 1 || normal_eq_chunks(N) > 0x7fffffff) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    if (!(huber_delta > 0.0)) return PVAMD_E_MODE;  // a NaN too
    if (A == 0) return 0;
    if (!grids || !stack || !points || !leaf_sums || !leaf_counts || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(grids, 8) || !aligned_to(stack, 4) || !aligned_to(points, 4) || !aligned_to(targets, 4) ||
        !aligned_to(leaf_sums, 8) || !aligned_to(leaf_counts, 8) || !aligned_to(scratch, 8))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)A * S;
    double* slab = (double*)scratch;
    int64_t* slab_count = normal_eq_slab_counts(scratch, rows, N);
    const dim3 grid_dim((unsigned)normal_eq_chunks(N), grid_rows(A));
    const size_t lds = (size_t)kJntWaves * S * (kJntSums * sizeof(double) + kJntCounts * sizeof(int));
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((joint_partial_kernel<true>), grid_dim, dim3(kJntBlock), lds, st, grids, S, stack, A, points, N, kinds,
                           targets, huber_delta, slab, slab_count);
    else
        hipLaunchKernelGGL((joint_partial_kernel<false>), grid_dim, dim3(kJntBlock), lds, st, grids, S, stack, A, points, N, kinds,
                           targets, huber_delta, slab, slab_count);
    launch_normal_eq_finish<kJntCounts>(rows, N, scratch, leaf_sums, leaf_counts, st);
    return (int)hipGetLastError();
}

extern "C" int pvamd_chain_twists(const pvamd_joint_t* joints, int32_t F, const float* q, int32_t A, int32_t M,
                                  const float* offset_inv, int32_t S, double* J, void* stream) {
    if (F < 1 || A < 0 || M < 0 || M > PVAMD_JOINT_MAX || S < 1 || S > PVAMD_JOINT_MAX_LEAVES) return PVAMD_E_SHAPE;
    if (A == 0 || M == 0) return 0;  // J holds nothing
    if (!joints || !q || !offset_inv || !J) return PVAMD_E_NULL;
    if (!aligned_to(joints, 4) || !aligned_to(q, 4) || !aligned_to(offset_inv, 4) || !aligned_to(J, 8)) return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(chain_twists_kernel, dim3((unsigned)((A + 63) / 64), (unsigned)S), dim3(64), (size_t)F * sizeof(int),
                       (hipStream_t)stream, joints, F, q, A, M, offset_inv, S, J);
    return (int)hipGetLastError();
}

extern "C" int pvamd_joint_assemble(const double* leaf_sums, const int64_t* leaf_counts, const double* J, int32_t A, int32_t S,
                                    int32_t M, double* sums, int64_t* counts, void* stream) {
    if (A < 0 || S < 1 || S > PVAMD_JOINT_MAX_LEAVES || M < 0 || M > PVAMD_JOINT_MAX) return PVAMD_E_SHAPE;
    if (A == 0) return 0;
    if (!leaf_sums || !leaf_counts || !sums || !counts || (M > 0 && !J)) return PVAMD_E_NULL;
    if (!aligned_to(leaf_sums, 8) || !aligned_to(leaf_counts, 8) || !aligned_to(J, 8) || !aligned_to(sums, 8) ||
        !aligned_to(counts, 8))
        return PVAMD_E_ALIGN;
    const int64_t per = 1 + (int64_t)M + (int64_t)M * (M + 1) / 2 + kJntCounts + S;
    hipLaunchKernelGGL(joint_assemble_kernel, dim3(stream_grid((int64_t)A * per, 256)), dim3(256), 0, (hipStream_t)stream, leaf_sums,
                       leaf_counts, J, A, S, M, sums, counts);
    return (int)hipGetLastError();
}

extern "C" int pvamd_joint_lm_step(int32_t A, int32_t M, const double* sums, int32_t first, double* q_acc, double* sums_acc,
                                   double* lambda, int32_t* accepted, double* q_try, float* q_next, const double* limits,
                                   double up, double down, double lambda_min, double lambda_max, void* stream) {
    if (A < 0 || M < 0 || M > PVAMD_JOINT_MAX) return PVAMD_E_SHAPE;
    if (!lm_args_ok(first, up, down, lambda_min, lambda_max)) return PVAMD_E_MODE;
    if (A == 0) return 0;
    if (!sums || !sums_acc || !lambda || !accepted) return PVAMD_E_NULL;
    if (M > 0 && (!q_acc || !q_try || !q_next)) return PVAMD_E_NULL;
    if (!aligned_to(sums, 8) || !aligned_to(q_acc, 8) || !aligned_to(sums_acc, 8) || !aligned_to(lambda, 8) ||
        !aligned_to(accepted, 4) || !aligned_to(q_try, 8) || !aligned_to(q_next, 4) || !aligned_to(limits, 8))
        return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(joint_lm_step_kernel, dim3((unsigned)A), dim3(64), 0, (hipStream_t)stream, M, sums, first, q_acc, sums_acc,
                       lambda, accepted, q_try, q_next, limits, up, down, lambda_min, lambda_max);
    return (int)hipGetLastError();
}
