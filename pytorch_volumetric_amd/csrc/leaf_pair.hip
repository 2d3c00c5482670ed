// Fused leaf-pair distance of a ComposedSDF / RobotSDF (include/pvamd.h "Leaf-pair distance"): for every ordered pair k = (s, t)
// and configuration a, the point of leaf t's set (given in leaf t's frame) where leaf s's SDF comes closest -- the bits of the
// one-leaf composition ComposedSDF([sdfs[s]], C[:, k]).min_over_points(points of t).  Nothing of size A x K x P is written.
//
//   lp_transform_kernel       one lane per (k, a): C[k][a] = Ms Mt^-1 (leaf t frame -> leaf s frame) with the rigid inverse
//   lp_partial_kernel         workgroup (chunk, a, k): mop_point of leaf s under C[k][a] at each point of a 4096-point chunk of
//                             set t, kept per lane as (value, first index) and reduced over the workgroup to one key.  When
//                             every set fits one chunk (FINISH, the common case) the same workgroup recomputes the answer at the
//                             winner and writes it: one launch after the transforms, no scratch
//   lp_finish_kernel          (sets above one chunk) one wave per (a, k): the minimum key over the pair's chunks, the answer
//                             recomputed at that point with the same statements
// Keys are min_over_points.hip's (order-preserving value bits, point index): exact, so the result does not depend on the launch
// geometry.  mop_point is called with the one-leaf arguments (grids + s, leaves [0, 1), the stack C[k]) that the one-leaf
// composition's own reduction passes, so the statements are the same.
//
// Backward:
//   lp_backward_kernel        one lane per (a, k): mop_backward_kernel's single-pair VJP w.r.t. the pair's transform (dC), then
//                             the VJP of the pair-transform statements to the two stack rows (dMs, dMt), stored per pair
//   lp_accumulate_kernel      one lane per stack row (leaf u, a): the sum over k in increasing order of the pairs that use u as
//                             s or as t.  No float atomics anywhere.
#include "common.h"
#include "grid_lookup.h"
#include "interp.h"
#include "leaf_vjp.h"
#include "composed_point.h"
#include "tf_reduce.h"

namespace pvamd {

constexpr int kLpBlock = 256;

// pair k of the device table: (s, t, offset of set t in the packed points, P_t)
struct LpPair {
    int s, t;
    int64_t off, P;
};

PVAMD_DEV bool lp_pair(const int64_t* __restrict__ table, int k, int S, int64_t npoints, LpPair& q) {
    q.s = (int)table[4 * k];
    q.t = (int)table[4 * k + 1];
    q.off = table[4 * k + 2];
    q.P = table[4 * k + 3];
    // a malformed row is never dereferenced: no points, no leaf
    return q.s >= 0 && q.s < S && q.t >= 0 && q.t < S && q.off >= 0 && q.P >= 1 && q.P <= (int64_t)0xfffffffe &&
           q.off <= npoints - q.P;
}

// ---- pair transforms: C[k][a] from stack rows Ms = (s, a), Mt = (t, a) ----
template <typename T> PVAMD_DEV T lp_fma(T a, T b, T c) {
    if constexpr (sizeof(T) == 4) return fmaf(a, b, c);
    else return __builtin_fma(a, b, c);
}

template <typename T>
__global__ __launch_bounds__(256) void lp_transform_kernel(const T* __restrict__ tf, int S, int A, const int64_t* __restrict__ table,
                                                           int K, T* __restrict__ C) {
    const int64_t n = (int64_t)K * A;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        const int k = (int)(q / A), a = (int)(q - (int64_t)k * A);
        const int s = (int)table[4 * k], t = (int)table[4 * k + 1];
        T* out = C + 16 * q;
        if (s < 0 || s >= S || t < 0 || t >= S) {
            for (int e = 0; e < 16; ++e) out[e] = __builtin_nan("");
            continue;
        }
        const T* Ms = tf + 16 * ((int64_t)s * A + a);
        const T* Mt = tf + 16 * ((int64_t)t * A + a);
        T c[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                c[4 * i + j] = lp_fma(Ms[4 * i + 2], Mt[4 * j + 2], lp_fma(Ms[4 * i + 1], Mt[4 * j + 1], Ms[4 * i] * Mt[4 * j]));
            c[4 * i + 3] = Ms[4 * i + 3] - lp_fma(c[4 * i + 2], Mt[11], lp_fma(c[4 * i + 1], Mt[7], c[4 * i] * Mt[3]));
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) out[e] = c[e];
        out[12] = T(0); out[13] = T(0); out[14] = T(0); out[15] = T(1);
    }
}

// ---- forward, pass 1 (FINISH: the whole answer): workgroup (chunk, a, k) ----
template <typename T, bool INTERP, bool FINISH>
__global__ __launch_bounds__(kLpBlock) void lp_partial_kernel(const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ C,
                                                              int A, const T* __restrict__ pts, int64_t npoints,
                                                              const int64_t* __restrict__ table, int K, int64_t nchunks,
                                                              MopKey* __restrict__ part, T* __restrict__ out_val,
                                                              T* __restrict__ out_grad, int64_t* __restrict__ out_index) {
    __shared__ uint64_t wk[kLpBlock / 64];
    __shared__ uint32_t wi[kLpBlock / 64];
    const int64_t chunk = blockIdx.x;
    const int k = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    LpPair q;
    const bool ok = lp_pair(table, k, S, npoints, q);  // workgroup-uniform
    const pvamd_grid_t* g = grids + (ok ? q.s : 0);
    const T* tfk = C + 16 * (int64_t)k * A;          // the pair's [A][4][4] stack: a one-leaf composition's
    const T* p0 = pts + 3 * (ok ? q.off : 0);
    const int64_t c0 = chunk * PVAMD_MOP_CHUNK;
    const int64_t c1 = ok ? (q.P < c0 + PVAMD_MOP_CHUNK ? q.P : c0 + PVAMD_MOP_CHUNK) : 0;
    for (int a = blockIdx.y; a < A; a += gridDim.y) {
        T bv = T(0);
        uint32_t bi = kNoIndex;
        // lane order = point order: the lane keeps the first of its points that reaches its minimum
#pragma unroll 1
        for (int64_t i = c0 + threadIdx.x; i < c1; i += kLpBlock) {
            const T p[3] = {p0[3 * i], p0[3 * i + 1], p0[3 * i + 2]};
            T v, gr[3];
            int s;
            mop_point<T, INTERP>(g, 0, 1, tfk, A, a, p, v, gr, s);
            const bool take = (bi == kNoIndex) | (!(v >= bv) & (bv == bv));
            bv = take ? v : bv;
            bi = take ? (uint32_t)i : bi;
        }
        uint64_t key = bi == kNoIndex ? ~0ull : mop_key(bv);
        mop_wave_min(key, bi);
        if (lane == 0) { wk[wave] = key; wi[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kLpBlock / 64; ++w)
                if (mop_less(wk[w], wi[w], key, bi)) { key = wk[w]; bi = wi[w]; }
            if constexpr (FINISH) {
                const int64_t pr = (int64_t)a * K + k;
                if (ok && bi != kNoIndex) {
                    const int64_t i = (int64_t)bi;
                    const T p[3] = {p0[3 * i], p0[3 * i + 1], p0[3 * i + 2]};
                    T v, gr[3];
                    int s;
                    mop_point<T, INTERP>(g, 0, 1, tfk, A, a, p, v, gr, s);
                    out_val[pr] = v;
                    out_grad[3 * pr] = gr[0];
                    out_grad[3 * pr + 1] = gr[1];
                    out_grad[3 * pr + 2] = gr[2];
                    out_index[pr] = i;
                } else {
                    out_val[pr] = __builtin_nan("");
                    out_grad[3 * pr] = out_grad[3 * pr + 1] = out_grad[3 * pr + 2] = __builtin_nan("");
                    out_index[pr] = -1;
                }
            } else {
                MopKey r;
                r.key = key; r.idx = bi; r.pad = 0;
                part[((int64_t)k * A + a) * nchunks + chunk] = r;
            }
        }
        __syncthreads();
    }
}

// ---- forward, pass 2 (sets above one chunk): one wave per (a, k) ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(64) void lp_finish_kernel(const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ C, int A,
                                                       const T* __restrict__ pts, int64_t npoints, const int64_t* __restrict__ table,
                                                       int K, int64_t nchunks, const MopKey* __restrict__ part,
                                                       T* __restrict__ out_val, T* __restrict__ out_grad,
                                                       int64_t* __restrict__ out_index) {
    const int64_t npairs = (int64_t)A * K;
    for (int64_t pr = blockIdx.x; pr < npairs; pr += gridDim.x) {
        const int a = (int)(pr / K), k = (int)(pr - (int64_t)a * K);
        LpPair q;
        const bool ok = lp_pair(table, k, S, npoints, q);
        const int64_t nc = ok ? (q.P + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK : 0;  // the pair's own chunks
        uint64_t key = ~0ull;
        uint32_t idx = kNoIndex;
        for (int64_t c = threadIdx.x; c < nc && c < nchunks; c += 64) {
            const MopKey m = part[((int64_t)k * A + a) * nchunks + c];
            if (mop_less(m.key, m.idx, key, idx)) { key = m.key; idx = m.idx; }
        }
        mop_wave_min(key, idx);
        if (threadIdx.x == 0) {
            if (ok && idx < (uint64_t)q.P) {
                const T* p0 = pts + 3 * q.off;
                const int64_t i = (int64_t)idx;
                const T p[3] = {p0[3 * i], p0[3 * i + 1], p0[3 * i + 2]};
                T v, gr[3];
                int s;
                mop_point<T, INTERP>(grids + q.s, 0, 1, C + 16 * (int64_t)k * A, A, a, p, v, gr, s);
                out_val[pr] = v;
                out_grad[3 * pr] = gr[0];
                out_grad[3 * pr + 1] = gr[1];
                out_grad[3 * pr + 2] = gr[2];
                out_index[pr] = i;
            } else {
                out_val[pr] = __builtin_nan("");
                out_grad[3 * pr] = out_grad[3 * pr + 1] = out_grad[3 * pr + 2] = __builtin_nan("");
                out_index[pr] = -1;
            }
        }
    }
}

// The VJP of the pair transform (include/pvamd.h "Leaf-pair distance" 1): C_rot = Rs Rt^T, C_t = ts - C_rot tt.  dC = the
// upstream of C[k][a] rows 0-2 -> dMs, dMt = the upstream of stack rows (s, a) and (t, a), rows 0-2
template <typename T>
PVAMD_DEV void lp_pair_vjp(const LpPair& q, const T* tf, const T* C, int A, int a, int k, const T (&dC)[12], T (&dMs)[12],
                           T (&dMt)[12]) {
    const T* Ms = tf + 16 * ((int64_t)q.s * A + a);
    const T* Mt = tf + 16 * ((int64_t)q.t * A + a);
    const T* M = C + 16 * ((int64_t)k * A + a);
    T dR[9];  // the total upstream of C_rot: its own and that through C_t
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        dMs[4 * r + 3] = dC[4 * r + 3];
#pragma unroll
        for (int m = 0; m < 3; ++m) dR[3 * r + m] = dC[4 * r + m] - dC[4 * r + 3] * Mt[4 * m + 3];
    }
#pragma unroll
    for (int m = 0; m < 3; ++m)
        dMt[4 * m + 3] = -(dC[3] * M[m] + dC[7] * M[4 + m] + dC[11] * M[8 + m]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            dMs[4 * r + m] = dR[3 * r] * Mt[m] + dR[3 * r + 1] * Mt[4 + m] + dR[3 * r + 2] * Mt[8 + m];
            dMt[4 * r + m] = dR[r] * Ms[m] + dR[3 + r] * Ms[4 + m] + dR[6 + r] * Ms[8 + m];
        }
    }
}

// ---- backward: one lane per (a, k) -> dM[(k * A + a)][24] = (dMs rows 0-2, dMt rows 0-2) ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(256) void lp_backward_kernel(const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ tf,
                                                          const T* __restrict__ C, int A, const T* __restrict__ pts,
                                                          int64_t npoints, const int64_t* __restrict__ table, int K,
                                                          const int64_t* __restrict__ index, const T* __restrict__ dval,
                                                          const T* __restrict__ dgrad, T* __restrict__ dM) {
    const int64_t npairs = (int64_t)A * K;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pr < npairs; pr += stride) {
        const int a = (int)(pr / K), k = (int)(pr - (int64_t)a * K);
        T* out = dM + 24 * ((int64_t)k * A + a);
        T dC[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) dC[e] = T(0);
        LpPair q;
        const int64_t i = index[pr];
        const bool ok = lp_pair(table, k, S, npoints, q) && i >= 0 && i < q.P;
        if (ok) {
            // mop_backward_kernel's statements for the single pair of a one-leaf composition: grid s, transform C[k][a]
            const pvamd_grid_t& g = grids[q.s];
            const T* M = C + 16 * ((int64_t)k * A + a);
            const T* p0 = pts + 3 * (q.off + i);
            const T p[3] = {p0[0], p0[1], p0[2]};
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
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) dC[4 * r + j] = has_g ? dx[r] * p[j] + gr[r] * dgg[j] : dx[r] * p[j];
                    dC[4 * r + 3] = dx[r];
                }
            }
        }
        T dMs[12], dMt[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) { dMs[e] = T(0); dMt[e] = T(0); }
        if (ok) lp_pair_vjp<T>(q, tf, C, A, a, k, dC, dMs, dMt);
#pragma unroll
        for (int e = 0; e < 12; ++e) { out[e] = dMs[e]; out[12 + e] = dMt[e]; }
    }
}

// dtf[u * A + a] = the sum over k = 0, 1, ... of dMs[k][a] (s_k = u) and dMt[k][a] (t_k = u); row 3 zero
template <typename T>
__global__ __launch_bounds__(256) void lp_accumulate_kernel(const T* __restrict__ dM, int S, int A, const int64_t* __restrict__ table,
                                                            int K, T* __restrict__ dtf) {
    const int64_t n = (int64_t)S * A;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += stride) {
        const int u = (int)(row / A), a = (int)(row - (int64_t)u * A);
        T acc[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[e] = T(0);
        for (int k = 0; k < K; ++k) {
            const int s = (int)table[4 * k], t = (int)table[4 * k + 1];
            const int side = s == u ? 0 : (t == u ? 12 : -1);
            if (side < 0) continue;
            const T* d = dM + 24 * ((int64_t)k * A + a) + side;
#pragma unroll
            for (int e = 0; e < 12; ++e) acc[e] += d[e];
        }
        T* out = dtf + 16 * row;
#pragma unroll
        for (int e = 0; e < 12; ++e) out[e] = acc[e];
        out[12] = T(0); out[13] = T(0); out[14] = T(0); out[15] = T(0);
    }
}

// The scratch of the leaf-pair entry points: the size functions report `bytes`, the launch code carves at the same offsets.
//   forward (distance and hinge): one 16-byte partial per (k, a, chunk) at 0 when a set holds more than one chunk, else nothing
//   distance backward:            dM [K][A][24] at 0
//   hinge backward:               the dC slab [K][A][nchunks][12] at 0, then dM; configurations split over workgroups by
//                                 tf_split_plan (the split does not change any sum)
struct LpPlan : TfSplit {  // hinge backward: configurations per workgroup, workgroups per (chunk, k)
    int64_t nchunks;  // chunks of the largest set: PVAMD_MOP_CHUNK points forward, kBwdChunk points in the hinge backward
    int64_t dM_off;   // backward, bytes
    int64_t bytes;
};

static LpPlan lp_plan(int K, int A, int64_t max_points, size_t elem, bool hinge, bool backward) {
    LpPlan p = {};
    if (!backward) {
        p.nchunks = (max_points + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK;
        p.bytes = PVAMD_LEAF_PAIR_SCRATCH_BYTES(K, A, max_points, elem, 0);
        return p;
    }
    if (hinge) {
        p.nchunks = (max_points + kBwdChunk - 1) / kBwdChunk;
        static_cast<TfSplit&>(p) = tf_split_plan((int64_t)K * p.nchunks, A);
        p.dM_off = tf_slab_bytes(p.nchunks * K * A, elem);
    }
    p.bytes = p.dM_off + PVAMD_LEAF_PAIR_SCRATCH_BYTES(K, A, max_points, elem, 1);
    return p;
}

template <typename T>
static int leaf_pair_transforms(const T* tf, int32_t S, int32_t A, const int64_t* table, int32_t K, T* out, void* stream) {
    if (S < 1 || A < 1 || K < 0) return PVAMD_E_SHAPE;
    if (K == 0) return 0;
    if (!tf || !table || !out) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(table, 8) || !aligned_to(out, sizeof(T))) return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(lp_transform_kernel<T>, dim3(stream_grid((int64_t)K * A, 256)), dim3(256), 0, (hipStream_t)stream, tf, S, A,
                       table, K, out);
    return (int)hipGetLastError();
}

template <typename T>
static int lp_check(const pvamd_grid_t* grids, int32_t S, const T* C, int32_t A, const T* points, int64_t npoints,
                    const int64_t* table, int32_t K, int32_t mode) {
    if (S < 1 || A < 1 || K < 0 || npoints < 1) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    if (K > 0 && (!grids || !C || !points || !table)) return PVAMD_E_NULL;
    if (!aligned_to(C, sizeof(T)) || !aligned_to(points, sizeof(T)) || !aligned_to(grids, 8) || !aligned_to(table, 8))
        return PVAMD_E_ALIGN;
    return 0;
}

template <typename T, bool INTERP>
static void lp_launch(const pvamd_grid_t* grids, int S, const T* C, int A, const T* points, int64_t npoints, const int64_t* table,
                      int K, int64_t nchunks, T* out_val, T* out_grad, int64_t* out_index, MopKey* part, hipStream_t st) {
    // configurations per workgroup: enough workgroups to fill the chip (a few thousand), then each loops over its configurations
    // so that a set's points are read from L2 for many a
    const int64_t want = (4096 + (int64_t)K * nchunks - 1) / ((int64_t)K * nchunks);
    const unsigned ay = grid_rows(A < want ? A : want);
    const dim3 grd((unsigned)nchunks, ay, (unsigned)K);
    if (nchunks == 1) {
        hipLaunchKernelGGL((lp_partial_kernel<T, INTERP, true>), grd, dim3(kLpBlock), 0, st, grids, S, C, A, points, npoints, table, K,
                           nchunks, part, out_val, out_grad, out_index);
        return;
    }
    hipLaunchKernelGGL((lp_partial_kernel<T, INTERP, false>), grd, dim3(kLpBlock), 0, st, grids, S, C, A, points, npoints, table, K,
                       nchunks, part, out_val, out_grad, out_index);
    const int64_t npairs = (int64_t)A * K;
    hipLaunchKernelGGL((lp_finish_kernel<T, INTERP>), dim3((unsigned)(npairs < 0x7fffffff ? npairs : 0x7fffffff)), dim3(64), 0, st,
                       grids, S, C, A, points, npoints, table, K, nchunks, part, out_val, out_grad, out_index);
}

template <typename T>
static int leaf_pair_distance(const pvamd_grid_t* grids, int32_t S, const T* C, int32_t A, const T* points, int64_t npoints,
                              const int64_t* table, int32_t K, int64_t max_points, int32_t mode, T* out_val, T* out_grad,
                              int64_t* out_index, void* scratch, void* stream) {
    if (max_points < 1 || max_points > npoints || max_points > (int64_t)0xfffffffe || K > kMaxGridRows) return PVAMD_E_SHAPE;
    if (int e = lp_check<T>(grids, S, C, A, points, npoints, table, K, mode)) return e;
    if (K == 0) return 0;
    const int64_t nchunks = lp_plan(K, A, max_points, sizeof(T), false, false).nchunks;
    if (!out_val || !out_grad || !out_index || (nchunks > 1 && !scratch)) return PVAMD_E_NULL;
    if (!aligned_to(out_val, sizeof(T)) || !aligned_to(out_grad, sizeof(T)) || !aligned_to(out_index, 8) || !aligned_to(scratch, 16))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    MopKey* part = (MopKey*)scratch;
    if (mode == PVAMD_LEAF_TRILINEAR)
        lp_launch<T, true>(grids, S, C, A, points, npoints, table, K, nchunks, out_val, out_grad, out_index, part, st);
    else
        lp_launch<T, false>(grids, S, C, A, points, npoints, table, K, nchunks, out_val, out_grad, out_index, part, st);
    return (int)hipGetLastError();
}

template <typename T>
static int leaf_pair_distance_backward(const pvamd_grid_t* grids, int32_t S, const T* tf, const T* C, int32_t A, const T* points,
                                       int64_t npoints, const int64_t* table, int32_t K, int32_t mode, const int64_t* index,
                                       const T* dval, const T* dgrad, T* dtf, void* scratch, void* stream) {
    if (S > kTfMaxLeaves) return PVAMD_E_SHAPE;  // the limit of every composed backward
    if (int e = lp_check<T>(grids, S, C, A, points, npoints, table, K, mode)) return e;
    if (!dtf) return 0;
    if (!tf || (K > 0 && (!index || !scratch))) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(index, 8) || (dval && !aligned_to(dval, sizeof(T))) ||
        (dgrad && !aligned_to(dgrad, sizeof(T))) || !aligned_to(dtf, sizeof(T)) || !aligned_to(scratch, 16))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (K == 0 || (!dval && !dgrad))  // nothing flows back: zeros
        return hipMemsetAsync(dtf, 0, (size_t)S * A * 16 * sizeof(T), st) != hipSuccess ? (int)hipGetLastError() : 0;
    T* dM = (T*)((char*)scratch + lp_plan(K, A, 1, sizeof(T), false, true).dM_off);  // this layout does not depend on the set sizes
    const int64_t npairs = (int64_t)A * K;
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((lp_backward_kernel<T, true>), dim3(stream_grid(npairs, 256)), dim3(256), 0, st, grids, S, tf, C, A, points,
                           npoints, table, K, index, dval, dgrad, dM);
    else
        hipLaunchKernelGGL((lp_backward_kernel<T, false>), dim3(stream_grid(npairs, 256)), dim3(256), 0, st, grids, S, tf, C, A, points,
                           npoints, table, K, index, dval, dgrad, dM);
    hipLaunchKernelGGL(lp_accumulate_kernel<T>, dim3(stream_grid((int64_t)S * A, 256)), dim3(256), 0, st, dM, S, A, table, K, dtf);
    return (int)hipGetLastError();
}


// ==== Leaf-pair hinge (include/pvamd.h "Leaf-pair hinge") ====
// For every pair k = (s, t) and configuration a: the bits of ComposedSDF([sdfs[s]], C[:, k]).hinge_over_points(points of t),
// sum_p max(m - v, 0) ** power and the count of v < m, with hinge_over_points.hip's statements and order of summation.
//   lph_partial_kernel        workgroup (chunk, a, k): hop_partial_kernel's loop body over a 4096-point chunk of set t, leaf s
//                             under C[k][a].  FINISH (every set within one chunk): the workgroup writes the answer, 0.0 + sum
//                             rounded as hop_finish_kernel rounds it; else one HopPart per (k, a, chunk)
//   lph_finish_kernel         (sets above one chunk) one wave per (a, k): hop_finish_kernel over the pair's own chunks
//   lph_backward_kernel       workgroup (1024-chunk, a-split, k): composed_backward_kernel's HINGE statements for the one-leaf
//                             composition, then the same reduction (tf_reduce.h) -> dC slab [k][a][chunk][12]
//   lph_pair_vjp_kernel       one lane per (a, k): the slab's chunks in chunk order (tf_chunk_sum), then lp_pair_vjp -> dM
//   lp_accumulate_kernel      as for the leaf-pair distance
template <typename T, bool INTERP, bool FINISH>
__global__ __launch_bounds__(kHopBlock) void lph_partial_kernel(const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ C,
                                                                int A, const T* __restrict__ pts, int64_t npoints,
                                                                const int64_t* __restrict__ table, int K, T m, int power,
                                                                int64_t nchunks, HopPart* __restrict__ part, T* __restrict__ out_val,
                                                                int64_t* __restrict__ out_count) {
    __shared__ double ws[kHopBlock / 64];
    __shared__ int wc[kHopBlock / 64];
    const int64_t chunk = blockIdx.x;
    const int k = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    LpPair q;
    const bool ok = lp_pair(table, k, S, npoints, q);  // workgroup-uniform
    if (!FINISH && (!ok || chunk * PVAMD_MOP_CHUNK >= q.P)) return;  // beyond the pair's own chunks: never read
    const pvamd_grid_t* g = grids + (ok ? q.s : 0);
    const T* tfk = C + 16 * (int64_t)k * A;  // the pair's [A][4][4] stack: a one-leaf composition's
    const T* p0 = pts + 3 * (ok ? q.off : 0);
    const int64_t P = ok ? q.P : 0;
    for (int a = blockIdx.y; a < A; a += gridDim.y) {
        double sum = 0.0;
        int cnt = 0;
#pragma unroll 1
        for (int kk = 0; kk < kHopK; ++kk) {
            const int64_t i = chunk * PVAMD_MOP_CHUNK + (int64_t)kk * kHopBlock + threadIdx.x;
            if (i < P) {
                const T p[3] = {p0[3 * i], p0[3 * i + 1], p0[3 * i + 2]};
                T v, gr[3];
                int s;
                mop_point<T, INTERP>(g, 0, 1, tfk, A, a, p, v, gr, s);
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
            if constexpr (FINISH) {
                const int64_t pr = (int64_t)a * K + k;
                double tot = 0.0;
                tot += sum;  // hop_finish_kernel's first (and only) chunk
                out_val[pr] = ok ? (T)tot : (T)__builtin_nan("");
                out_count[pr] = ok ? (int64_t)cnt : 0;
            } else {
                HopPart r;
                r.sum = sum; r.count = cnt;
                part[((int64_t)k * A + a) * nchunks + chunk] = r;
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(64) void lph_finish_kernel(int S, int A, int64_t npoints, const int64_t* __restrict__ table, int K,
                                                        int64_t nchunks, const HopPart* __restrict__ part, T* __restrict__ out_val,
                                                        int64_t* __restrict__ out_count) {
    const int64_t npairs = (int64_t)A * K;
    for (int64_t pr = blockIdx.x; pr < npairs; pr += gridDim.x) {
        const int a = (int)(pr / K), k = (int)(pr - (int64_t)a * K);
        LpPair q;
        const bool ok = lp_pair(table, k, S, npoints, q);
        int64_t nc = ok ? (q.P + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK : 0;  // the pair's own chunks
        nc = nc < nchunks ? nc : nchunks;
        const HopPart* row = part + ((int64_t)k * A + a) * nchunks;
        double sum = 0.0;
        int64_t cnt = 0;
        for (int64_t base = 0; base < nc; base += 64) {
            const int64_t c = base + threadIdx.x;
            HopPart h;
            h.sum = 0.0; h.count = 0;
            if (c < nc) h = row[c];
            cnt += h.count;
            const int n = (nc - base) < 64 ? (int)(nc - base) : 64;
            for (int j = 0; j < n; ++j) sum += __shfl(h.sum, j, 64);  // every lane: the same sum in chunk order
        }
        cnt = hop_wave_sum<int64_t>(cnt);
        if (threadIdx.x == 0) {
            out_val[pr] = ok ? (T)sum : (T)__builtin_nan("");
            out_count[pr] = cnt;
        }
    }
}

// ---- backward, pass 1: workgroup (chunk, split, k) -> slab[((k * A + a) * nchunks + chunk)][12] ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(kBwdBlock) void lph_backward_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                 const T* __restrict__ C, int A, const T* __restrict__ pts,
                                                                 int64_t npoints, const int64_t* __restrict__ table, int K, T margin,
                                                                 int power, const T* __restrict__ up, int aper, int64_t nchunks,
                                                                 T* __restrict__ slab) {
    __shared__ T part[kTfWaves][1][12];  // one leaf
    __shared__ int present[kTfWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t chunk = blockIdx.x;
    const int k = blockIdx.z;
    LpPair q;
    if (!lp_pair(table, k, S, npoints, q) || chunk * kBwdChunk >= q.P) return;  // workgroup-uniform: never read
    const int a0 = blockIdx.y * aper;
    const int a1 = (a0 + aper) < A ? (a0 + aper) : A;
    const pvamd_grid_t& g = grids[q.s];
    const T* tfk = C + 16 * (int64_t)k * A;
    const T* p0 = pts + 3 * q.off;

    T p[kBwdK][3];
    bool live[kBwdK];
#pragma unroll
    for (int kk = 0; kk < kBwdK; ++kk) {
        const int64_t i = chunk * kBwdChunk + (int64_t)kk * kBwdBlock + threadIdx.x;
        live[kk] = i < q.P;
#pragma unroll
        for (int d = 0; d < 3; ++d) p[kk][d] = live[kk] ? p0[3 * i + d] : T(0);
    }

    for (int a = a0; a < a1; ++a) {
        if (lane == 0) present[wave] = 0;
        const T u = up[(int64_t)a * K + k];
#pragma unroll
        for (int kk = 0; kk < kBwdK; ++kk) {
            // composed_backward_kernel<T, true, false, true, false, INTERP, true> for the one-leaf composition (grids + s, C[k])
            int s = -1;
            T c[12] = {};
            if (live[kk]) {
                T v, gv[3];
                mop_point<T, INTERP>(&g, 0, 1, tfk, A, a, p[kk], v, gv, s);
                const T d = margin - v;
                const T h = (d > T(0) || d != d) ? d : T(0);
                const T hdv = -((d >= T(0)) ? (power == 2 ? u * (T(2) * h) : u) : T(0));
                if (s < 0 || s >= 1) s = -1;
                if (s >= 0) {
                    const T* M = tfk + 16 * (int64_t)a;
                    T dg[3] = {0, 0, 0};
                    T x[3], gr[3] = {0, 0, 0}, dx[3] = {0, 0, 0};
                    LeafOps<T>::xform(M, p[kk], x);
                    if (LeafOps<T>::inside(g, x)) {
                        if constexpr (INTERP) InterpOps<T>::leaf(g, x, hdv, dg, false, gr, dx);
                        else s = -1;  // a nearest leaf in range has no derivative
                    } else {
                        box_backward<T>(g, x, hdv, dg, false, gr, dx);
                    }
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) c[4 * r + j] = dx[r] * p[kk][j];
                        c[4 * r + 3] = dx[r];
                    }
                }
            }
            tf_wave_reduce(s, c, part, present, wave, lane);
        }
        tf_block_store(1, part, present, slab + (((int64_t)k * A + a) * nchunks + chunk) * 12, 0);
    }
}

// ---- backward, pass 2: one lane per (a, k): dC = the pair's chunks in chunk order, then the pair-transform VJP -> dM ----
template <typename T>
__global__ __launch_bounds__(256) void lph_pair_vjp_kernel(int S, const T* __restrict__ tf, const T* __restrict__ C, int A,
                                                           int64_t npoints, const int64_t* __restrict__ table, int K,
                                                           int64_t nchunks, const T* __restrict__ slab, T* __restrict__ dM) {
    const int64_t npairs = (int64_t)A * K;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pr < npairs; pr += stride) {
        const int a = (int)(pr / K), k = (int)(pr - (int64_t)a * K);
        LpPair q;
        const bool ok = lp_pair(table, k, S, npoints, q);
        int64_t nc = ok ? (q.P + kBwdChunk - 1) / kBwdChunk : 0;  // the pair's own chunks
        nc = nc < nchunks ? nc : nchunks;
        const T* row = slab + ((int64_t)k * A + a) * nchunks * 12;
        T dC[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) dC[e] = tf_chunk_sum<T>(row + e, nc, 12);
        T dMs[12], dMt[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) { dMs[e] = T(0); dMt[e] = T(0); }
        if (ok) lp_pair_vjp<T>(q, tf, C, A, a, k, dC, dMs, dMt);
        T* out = dM + 24 * ((int64_t)k * A + a);
#pragma unroll
        for (int e = 0; e < 12; ++e) { out[e] = dMs[e]; out[12 + e] = dMt[e]; }
    }
}

template <typename T>
static int lph_check(const pvamd_grid_t* grids, int32_t S, const T* C, int32_t A, const T* points, int64_t npoints,
                     const int64_t* table, int32_t K, int64_t max_points, int32_t mode, int32_t power) {
    if (max_points < 1 || max_points > npoints || max_points > (int64_t)0xfffffffe || K > kMaxGridRows) return PVAMD_E_SHAPE;
    if (S < 1 || A < 1 || K < 0) return PVAMD_E_SHAPE;
    if (power != 1 && power != 2) return PVAMD_E_MODE;
    return lp_check<T>(grids, S, C, A, points, npoints, table, K, mode);
}

template <typename T, bool INTERP>
static void lph_launch(const pvamd_grid_t* grids, int S, const T* C, int A, const T* points, int64_t npoints, const int64_t* table,
                       int K, int64_t nchunks, T m, int power, T* out_val, int64_t* out_count, HopPart* part, hipStream_t st) {
    // lp_launch's geometry: a few thousand workgroups, each looping over its configurations
    const int64_t want = (4096 + (int64_t)K * nchunks - 1) / ((int64_t)K * nchunks);
    const unsigned ay = grid_rows(A < want ? A : want);
    const dim3 grd((unsigned)nchunks, ay, (unsigned)K);
    if (nchunks == 1) {
        hipLaunchKernelGGL((lph_partial_kernel<T, INTERP, true>), grd, dim3(kHopBlock), 0, st, grids, S, C, A, points, npoints, table,
                           K, m, power, nchunks, part, out_val, out_count);
        return;
    }
    hipLaunchKernelGGL((lph_partial_kernel<T, INTERP, false>), grd, dim3(kHopBlock), 0, st, grids, S, C, A, points, npoints, table, K,
                       m, power, nchunks, part, out_val, out_count);
    const int64_t npairs = (int64_t)A * K;
    hipLaunchKernelGGL(lph_finish_kernel<T>, dim3((unsigned)(npairs < 0x7fffffff ? npairs : 0x7fffffff)), dim3(64), 0, st, S, A,
                       npoints, table, K, nchunks, part, out_val, out_count);
}

template <typename T>
static int leaf_pair_hinge(const pvamd_grid_t* grids, int32_t S, const T* C, int32_t A, const T* points, int64_t npoints,
                           const int64_t* table, int32_t K, int64_t max_points, int32_t mode, T margin, int32_t power, T* out_val,
                           int64_t* out_count, void* scratch, void* stream) {
    if (int e = lph_check<T>(grids, S, C, A, points, npoints, table, K, max_points, mode, power)) return e;
    if (K == 0) return 0;
    const int64_t nchunks = lp_plan(K, A, max_points, sizeof(T), true, false).nchunks;
    if (!out_val || !out_count || (nchunks > 1 && !scratch)) return PVAMD_E_NULL;
    if (!aligned_to(out_val, sizeof(T)) || !aligned_to(out_count, 8) || !aligned_to(scratch, 16)) return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    HopPart* part = (HopPart*)scratch;
    if (mode == PVAMD_LEAF_TRILINEAR)
        lph_launch<T, true>(grids, S, C, A, points, npoints, table, K, nchunks, margin, power, out_val, out_count, part, st);
    else
        lph_launch<T, false>(grids, S, C, A, points, npoints, table, K, nchunks, margin, power, out_val, out_count, part, st);
    return (int)hipGetLastError();
}

template <typename T>
static int leaf_pair_hinge_backward(const pvamd_grid_t* grids, int32_t S, const T* tf, const T* C, int32_t A, const T* points,
                                    int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode, T margin,
                                    int32_t power, const T* up, T* dtf, void* scratch, void* stream) {
    if (S > kTfMaxLeaves) return PVAMD_E_SHAPE;  // the limit of every composed backward
    if (int e = lph_check<T>(grids, S, C, A, points, npoints, table, K, max_points, mode, power)) return e;
    if (!dtf) return 0;
    if (!tf || (K > 0 && (!up || !scratch))) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(up, sizeof(T)) || !aligned_to(dtf, sizeof(T)) || !aligned_to(scratch, 16))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (K == 0)  // nothing flows back: zeros
        return hipMemsetAsync(dtf, 0, (size_t)S * A * 16 * sizeof(T), st) != hipSuccess ? (int)hipGetLastError() : 0;
    const LpPlan p = lp_plan(K, A, max_points, sizeof(T), true, true);
    T* slab = (T*)scratch;
    T* dM = (T*)((char*)scratch + p.dM_off);
    const dim3 grd((unsigned)p.nchunks, (unsigned)p.nsplit, (unsigned)K);
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((lph_backward_kernel<T, true>), grd, dim3(kBwdBlock), 0, st, grids, S, C, A, points, npoints, table, K,
                           margin, power, up, p.aper, p.nchunks, slab);
    else
        hipLaunchKernelGGL((lph_backward_kernel<T, false>), grd, dim3(kBwdBlock), 0, st, grids, S, C, A, points, npoints, table, K,
                           margin, power, up, p.aper, p.nchunks, slab);
    const int64_t npairs = (int64_t)A * K;
    hipLaunchKernelGGL(lph_pair_vjp_kernel<T>, dim3(stream_grid(npairs, 256)), dim3(256), 0, st, S, tf, C, A, npoints, table, K,
                       p.nchunks, slab, dM);
    hipLaunchKernelGGL(lp_accumulate_kernel<T>, dim3(stream_grid((int64_t)S * A, 256)), dim3(256), 0, st, dM, S, A, table, K, dtf);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_leaf_pair_scratch_bytes(int32_t K, int32_t A, int64_t max_points, int32_t is_f64, int32_t backward) {
    if (K < 1 || A < 1 || max_points < 1) return 0;
    return lp_plan(K, A, max_points, is_f64 ? 8 : 4, false, backward != 0).bytes;
}

extern "C" int pvamd_leaf_pair_transforms(const float* tf, int32_t S, int32_t A, const int64_t* table, int32_t K, float* out,
                                          void* stream) {
    return leaf_pair_transforms<float>(tf, S, A, table, K, out, stream);
}

extern "C" int pvamd_leaf_pair_transforms_f64(const double* tf, int32_t S, int32_t A, const int64_t* table, int32_t K, double* out,
                                              void* stream) {
    return leaf_pair_transforms<double>(tf, S, A, table, K, out, stream);
}

extern "C" int pvamd_leaf_pair_distance(const pvamd_grid_t* grids, int32_t S, const float* C, int32_t A, const float* points,
                                        int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode,
                                        float* out_val, float* out_grad, int64_t* out_index, void* scratch, void* stream) {
    return leaf_pair_distance<float>(grids, S, C, A, points, npoints, table, K, max_points, mode, out_val, out_grad, out_index, scratch,
                                     stream);
}

extern "C" int pvamd_leaf_pair_distance_f64(const pvamd_grid_t* grids, int32_t S, const double* C, int32_t A, const double* points,
                                            int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode,
                                            double* out_val, double* out_grad, int64_t* out_index, void* scratch, void* stream) {
    return leaf_pair_distance<double>(grids, S, C, A, points, npoints, table, K, max_points, mode, out_val, out_grad, out_index,
                                      scratch, stream);
}

extern "C" int pvamd_leaf_pair_distance_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, const float* C, int32_t A,
                                                 const float* points, int64_t npoints, const int64_t* table, int32_t K, int32_t mode,
                                                 const int64_t* index, const float* dval, const float* dgrad, float* dtf,
                                                 void* scratch, void* stream) {
    return leaf_pair_distance_backward<float>(grids, S, tf, C, A, points, npoints, table, K, mode, index, dval, dgrad, dtf, scratch,
                                              stream);
}

extern "C" int pvamd_leaf_pair_distance_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, const double* C,
                                                     int32_t A, const double* points, int64_t npoints, const int64_t* table,
                                                     int32_t K, int32_t mode, const int64_t* index, const double* dval,
                                                     const double* dgrad, double* dtf, void* scratch, void* stream) {
    return leaf_pair_distance_backward<double>(grids, S, tf, C, A, points, npoints, table, K, mode, index, dval, dgrad, dtf, scratch,
                                               stream);
}

extern "C" int64_t pvamd_leaf_pair_hinge_scratch_bytes(int32_t K, int32_t A, int64_t max_points, int32_t is_f64, int32_t backward) {
    if (K < 1 || A < 1 || max_points < 1) return 0;
    return lp_plan(K, A, max_points, is_f64 ? 8 : 4, true, backward != 0).bytes;
}

extern "C" int pvamd_leaf_pair_hinge(const pvamd_grid_t* grids, int32_t S, const float* C, int32_t A, const float* points,
                                     int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode, float margin,
                                     int32_t power, float* out_val, int64_t* out_count, void* scratch, void* stream) {
    return leaf_pair_hinge<float>(grids, S, C, A, points, npoints, table, K, max_points, mode, margin, power, out_val, out_count,
                                  scratch, stream);
}

extern "C" int pvamd_leaf_pair_hinge_f64(const pvamd_grid_t* grids, int32_t S, const double* C, int32_t A, const double* points,
                                         int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode,
                                         double margin, int32_t power, double* out_val, int64_t* out_count, void* scratch,
                                         void* stream) {
    return leaf_pair_hinge<double>(grids, S, C, A, points, npoints, table, K, max_points, mode, margin, power, out_val, out_count,
                                   scratch, stream);
}

extern "C" int pvamd_leaf_pair_hinge_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, const float* C, int32_t A,
                                              const float* points, int64_t npoints, const int64_t* table, int32_t K, int64_t max_points,
                                              int32_t mode, float margin, int32_t power, const float* up, float* dtf, void* scratch,
                                              void* stream) {
    return leaf_pair_hinge_backward<float>(grids, S, tf, C, A, points, npoints, table, K, max_points, mode, margin, power, up, dtf,
                                           scratch, stream);
}

extern "C" int pvamd_leaf_pair_hinge_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, const double* C, int32_t A,
                                                  const double* points, int64_t npoints, const int64_t* table, int32_t K,
                                                  int64_t max_points, int32_t mode, double margin, int32_t power, const double* up,
                                                  double* dtf, void* scratch, void* stream) {
    return leaf_pair_hinge_backward<double>(grids, S, tf, C, A, points, npoints, table, K, max_points, mode, margin, power, up, dtf,
                                            scratch, stream);
}
