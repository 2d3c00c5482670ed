// Backward (vector-Jacobian products) of the cached, composed and grid-chamfer queries: what torch autograd computes
// through the reference's expressions (sdf.py:399,409,421-426,556-571; chamfer.py:82-94), given the forward's decisions.
//
// Per (configuration a, point p) with winning leaf s (out_leaf of the forward), M = tf[s*A+a], L = M[:3,:3]:
//   x  = L p + t                                 recomputed with the forward's own fma chain (affine_row), so the range
//                                                test, the active axes and the voxel index agree with the forward bit for bit
//   in range:  g = the grid record's gradient    no derivative w.r.t. x (sdf.py:549-550: a table lookup)
//   outside :  d = signed excess over the surface box, n = d / |d|, active_i = d_i != 0
//              dx_i = active_i ? dv n_i + (dg_i - n_i (n . dg)) / |d| : 0     (d val / dx = n, d n / dx = (I - n n^T) D / |d|)
//   gg = L^T g (the forward's rotation back)  =>  dg = L dgg,   dL[r][j] += g_r dgg_j
//   dp = L^T dx,   dL[r][j] += dx_r p_j,   dt_r = dx_r
// Every sum is a fixed-order reduction (no float atomics): dpoints over configurations in registers (configuration order) and,
// when the configurations are split over workgroups, over the splits in split order; dtf over the points of a workgroup by
// wave butterflies + per-wave LDS slots, then over the workgroups' slab rows in chunk order (tf_reduce.h, which the ray-cast and
// the leaf-pair hinge backward share).  Results are bitwise reproducible from run to run (float atomics would make the sums
// depend on arrival order).
#include "common.h"
#include "grid_lookup.h"
#include "interp.h"
#include "leaf_vjp.h"
#include "composed_point.h"
#include "tf_reduce.h"

namespace pvamd {

// ---- CachedSDF.__call__ backward: one point per lane, no reduction ----
template <typename T, bool HAS_V, bool HAS_G, bool INTERP>
__global__ __launch_bounds__(256) void cached_backward_kernel(const pvamd_grid_t g, const T* __restrict__ pts, int64_t P,
                                                              const T* __restrict__ dval, const T* __restrict__ dgrad,
                                                              T* __restrict__ dpts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride) {
        const T x[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        T dx[3] = {0, 0, 0};
        const bool inside = LeafOps<T>::inside(g, x);
        if (!inside || INTERP) {
            const T dv = HAS_V ? dval[i] : T(0);
            T dg[3] = {0, 0, 0};
            if (HAS_G) { dg[0] = dgrad[3 * i]; dg[1] = dgrad[3 * i + 1]; dg[2] = dgrad[3 * i + 2]; }
            T n[3];
            if (inside) InterpOps<T>::leaf(g, x, dv, dg, HAS_G, n, dx);
            else box_backward<T>(g, x, dv, dg, HAS_G, n, dx);
        }
        dpts[3 * i] = dx[0];
        dpts[3 * i + 1] = dx[1];
        dpts[3 * i + 2] = dx[2];
    }
}

// ---- ComposedSDF.__call__ / grid chamfer backward ----
// Workgroup (chunk, split): points [chunk * kBwdChunk, +kBwdChunk) x configurations [split * aper, +aper).  Each lane keeps the
// dpoints of its kBwdK points in registers over the configurations; per configuration the 12 dtf partials of every
// (configuration, leaf) go through tf_wave_reduce and tf_block_store (tf_reduce.h) and leave as one slab row
// [chunk][s*A + a][12].
// CHAMFER: one leaf (the grid g0), tf = the B world->object matrices, dv = dsum[a] * d(scale v)^2/dv = dsum[a] 2 scale^2 v.
// HINGE (the upstream policy of hinge_over_points): no leaf ids and no (A, P) upstream.  Per pair the composed value v and the
// winning leaf are recomputed with the forward's statements (mop_point, the same bits), and dv is torch's VJP of
// (m - v).clamp(min=0) ** power summed over p, with upstream up[a * up_stride]: -(up (2 h)) (power 2) or -up (power 1) where
// m - v >= 0, else -0.  A per-leaf hinge runs this kernel once per leaf as the one-leaf composition (hinge_backward).
template <typename T, bool HAS_V, bool HAS_G, bool WANT_TF, bool CHAMFER, bool INTERP, bool HINGE = false>
__global__ __launch_bounds__(kBwdBlock) void composed_backward_kernel(
    const pvamd_grid_t* __restrict__ grids, const pvamd_grid_t g0, int S, const T* __restrict__ tf, int A,
    const T* __restrict__ pts, int64_t P, const int32_t* __restrict__ leaf, const T* __restrict__ dval,
    const T* __restrict__ dgrad, T scale, int aper, T* __restrict__ dp_out, T* __restrict__ slab,
    const T* __restrict__ up = nullptr, int64_t up_stride = 0, T margin = T(0), int power = 0) {
    __shared__ T part[kTfWaves][kTfMaxLeaves][12];
    __shared__ uint64_t present[kTfWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t chunk = blockIdx.x;
    const int split = blockIdx.y;
    const int a0 = split * aper;
    const int a1 = (a0 + aper) < A ? (a0 + aper) : A;

    T p[kBwdK][3], dp[kBwdK][3];
    int64_t idx[kBwdK];
    bool live[kBwdK];
#pragma unroll
    for (int k = 0; k < kBwdK; ++k) {
        idx[k] = chunk * kBwdChunk + (int64_t)k * kBwdBlock + threadIdx.x;
        live[k] = idx[k] < P;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            p[k][d] = live[k] ? pts[3 * idx[k] + d] : T(0);
            dp[k][d] = T(0);
        }
    }

    for (int a = a0; a < a1; ++a) {
        if (WANT_TF && lane == 0) present[wave] = 0;
#pragma unroll
        for (int k = 0; k < kBwdK; ++k) {
            int s = -1;
            T c[12] = {};
            if (live[k]) {
                const int64_t o = (int64_t)a * P + idx[k];
                T hdv = T(0);
                if constexpr (HINGE) {
                    T v, g[3];
                    mop_point<T, INTERP>(grids, 0, S, tf, A, a, p[k], v, g, s);
                    const T d = margin - v;
                    const T u = up[(int64_t)a * up_stride];
                    const T h = (d > T(0) || d != d) ? d : T(0);
                    hdv = -((d >= T(0)) ? (power == 2 ? u * (T(2) * h) : u) : T(0));
                } else {
                    s = CHAMFER ? 0 : leaf[o];
                }
                if (s < 0 || s >= S) s = -1;  // a malformed leaf id contributes nothing (and is never dereferenced)
                if (s >= 0) {
                    const pvamd_grid_t& g = CHAMFER ? g0 : grids[s];
                    const T* M = tf + 16 * ((int64_t)s * A + a);
                    T dgg[3] = {0, 0, 0}, dg[3] = {0, 0, 0};
                    if (HAS_G) {
                        dgg[0] = dgrad[3 * o]; dgg[1] = dgrad[3 * o + 1]; dgg[2] = dgrad[3 * o + 2];
#pragma unroll
                        for (int r = 0; r < 3; ++r) dg[r] = M[4 * r] * dgg[0] + M[4 * r + 1] * dgg[1] + M[4 * r + 2] * dgg[2];
                    }
                    T x[3], gr[3] = {0, 0, 0}, dx[3] = {0, 0, 0};
                    LeafOps<T>::xform(M, p[k], x);
                    if (LeafOps<T>::inside(g, x)) {
                        if constexpr (INTERP) InterpOps<T>::leaf(g, x, HINGE ? hdv : (HAS_V ? dval[o] : T(0)), dg, HAS_G, gr, dx);
                        else if (HAS_G) LeafOps<T>::record_grad(g, x, gr);
                        else s = -1;  // value-only upstream: an in-range winner contributes nothing
                    } else if (CHAMFER) {
                        T t[3];
                        const T nrm = LeafOps<T>::box(g, x, t);
                        const T dv = dval[a] * (T(2) * scale) * (scale * nrm);
#pragma unroll
                        for (int d = 0; d < 3; ++d) dx[d] = (t[d] != T(0)) ? dv * LeafOps<T>::div(t[d], nrm) : T(0);
                    } else {
                        const T dv = HINGE ? hdv : (HAS_V ? dval[o] : T(0));
                        box_backward<T>(g, x, dv, dg, HAS_G, gr, dx);
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) dp[k][j] += M[j] * dx[0] + M[4 + j] * dx[1] + M[8 + j] * dx[2];
                    if (WANT_TF) {
                        // without a gradient upstream gr[r] * dgg[j] is no term at all: out of range but inside the box
                        // (|d| = 0) gr is 0 / 0, and NaN * 0 would reach dtf where torch gives 0
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
#pragma unroll
                            for (int j = 0; j < 3; ++j) c[4 * r + j] = HAS_G ? dx[r] * p[k][j] + gr[r] * dgg[j] : dx[r] * p[k][j];
                            c[4 * r + 3] = dx[r];
                        }
                    }
                }
            }
            if (WANT_TF) tf_wave_reduce(s, c, part, present, wave, lane);
        }
        if (WANT_TF) tf_block_store(S, part, present, slab + (chunk * ((int64_t)S * A) + a) * 12, (int64_t)A * 12);
    }
    if (dp_out) {
        T* out = dp_out + (int64_t)split * P * 3;
#pragma unroll
        for (int k = 0; k < kBwdK; ++k)
            if (live[k]) {
                out[3 * idx[k]] = dp[k][0];
                out[3 * idx[k] + 1] = dp[k][1];
                out[3 * idx[k] + 2] = dp[k][2];
            }
    }
}

// dpoints[i] = sum over splits, in split order, of part[split][i]
template <typename T>
__global__ __launch_bounds__(256) void reduce_splits_kernel(const T* __restrict__ part, int nsplit, int64_t n, T* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        T v = T(0);
        for (int sp = 0; sp < nsplit; ++sp) v += part[(int64_t)sp * n + i];
        out[i] = v;
    }
}

// The launch geometry and the scratch layout of one composed backward pass.  The size functions report `bytes` (the per-leaf
// hinge: `leaf_off` plus its leaf term) and the launch code carves at the same offsets: the slab at 0, the split rows, the leaf term.
struct BwdPlan : TfSplit {
    int64_t nchunks;
    int64_t split_off;  // bytes: past the slab [nchunks][S*A][12]; the dpoints rows [nsplit][P][3] when nsplit > 1
    int64_t bytes;      // slab and split rows
    int64_t leaf_off;   // bytes: past both; the per-leaf hinge's one [P][3] leaf term
};

static BwdPlan bwd_plan(int S, int A, int64_t P, size_t elem) {
    BwdPlan b;
    b.nchunks = (P + kBwdChunk - 1) / kBwdChunk;
    if (b.nchunks < 1) b.nchunks = 1;
    static_cast<TfSplit&>(b) = tf_split_plan(b.nchunks, A);
    b.split_off = tf_slab_bytes(b.nchunks * (int64_t)S * A, elem);
    b.bytes = b.split_off + (b.nsplit > 1 ? (int64_t)b.nsplit * P * 3 * (int64_t)elem : 0);
    b.leaf_off = round256(b.bytes);
    return b;
}

static int64_t bwd_scratch_bytes(int S, int A, int64_t P, size_t elem) { return bwd_plan(S, A, P, elem).bytes; }

template <typename T, bool HAS_V, bool HAS_G, bool CHAMFER, bool INTERP>
static void launch_composed_backward(const BwdPlan& b, hipStream_t st, const pvamd_grid_t* grids, const pvamd_grid_t& g0, int S,
                                     const T* tf, int A, const T* pts, int64_t P, const int32_t* leaf, const T* dval,
                                     const T* dgrad, T scale, T* dp_out, T* slab, bool want_tf) {
    const dim3 grid((unsigned)b.nchunks, (unsigned)b.nsplit);
    if (want_tf)
        hipLaunchKernelGGL((composed_backward_kernel<T, HAS_V, HAS_G, true, CHAMFER, INTERP>), grid, dim3(kBwdBlock), 0, st, grids, g0, S, tf,
                           A, pts, P, leaf, dval, dgrad, scale, b.aper, dp_out, slab);
    else
        hipLaunchKernelGGL((composed_backward_kernel<T, HAS_V, HAS_G, false, CHAMFER, INTERP>), grid, dim3(kBwdBlock), 0, st, grids, g0, S, tf,
                           A, pts, P, leaf, dval, dgrad, scale, b.aper, dp_out, slab);
}

template <typename T, bool INTERP = false>
static int composed_backward(const pvamd_grid_t* grids, const pvamd_grid_t* g0, int32_t S, const T* tf, int32_t A, const T* points,
                             int64_t P, const int32_t* leaf, const T* dval, const T* dgrad, T scale, T* dpoints, T* dtf,
                             void* scratch, void* stream, bool chamfer) {
    if (S < 1 || S > kTfMaxLeaves || A < 1 || P < 0) return PVAMD_E_SHAPE;
    if (!dpoints && !dtf) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t SA = (int64_t)S * A;
    if (P == 0 || (!dval && !dgrad)) {  // nothing flows back: zeros
        if (dtf && hipMemsetAsync(dtf, 0, (size_t)SA * 16 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
        if (dpoints && P > 0 && hipMemsetAsync(dpoints, 0, (size_t)P * 3 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
        return (int)hipGetLastError();
    }
    if (!tf || !points || (!chamfer && (!grids || !leaf))) return PVAMD_E_NULL;
    const BwdPlan b = bwd_plan(S, A, P, sizeof(T));
    if (!scratch && (dtf || b.nsplit > 1)) return PVAMD_E_NULL;
    if (!aligned_to(tf, sizeof(T)) || !aligned_to(points, sizeof(T)) || (scratch && !aligned_to(scratch, 16)) ||
        (dpoints && !aligned_to(dpoints, sizeof(T))) || (dtf && !aligned_to(dtf, sizeof(T))))
        return PVAMD_E_ALIGN;
    if (b.nchunks > 0x7fffffff) return PVAMD_E_SHAPE;
    T* slab = (T*)scratch;
    T* split_part = scratch ? (T*)((char*)scratch + b.split_off) : nullptr;
    T* dp_out = dpoints ? (b.nsplit > 1 ? split_part : dpoints) : nullptr;
    const pvamd_grid_t gz = chamfer ? *g0 : pvamd_grid_t{};
    if (chamfer)
        launch_composed_backward<T, true, false, true, false>(b, st, nullptr, gz, 1, tf, A, points, P, nullptr, dval, nullptr, scale,
                                                       dp_out, slab, dtf != nullptr);
    else if (dval && dgrad)
        launch_composed_backward<T, true, true, false, INTERP>(b, st, grids, gz, S, tf, A, points, P, leaf, dval, dgrad, scale, dp_out,
                                                       slab, dtf != nullptr);
    else if (dval)
        launch_composed_backward<T, true, false, false, INTERP>(b, st, grids, gz, S, tf, A, points, P, leaf, dval, nullptr, scale, dp_out,
                                                        slab, dtf != nullptr);
    else
        launch_composed_backward<T, false, true, false, INTERP>(b, st, grids, gz, S, tf, A, points, P, leaf, nullptr, dgrad, scale, dp_out,
                                                        slab, dtf != nullptr);
    if (dtf) launch_reduce_tf<T, T>(slab, b.nchunks, SA, dtf, st);
    if (dpoints && b.nsplit > 1)
        hipLaunchKernelGGL(reduce_splits_kernel<T>, dim3(stream_grid(P * 3, 256)), dim3(256), 0, st, split_part, b.nsplit, P * 3,
                           dpoints);
    return (int)hipGetLastError();
}

// sum[i] += add[i]: the per-leaf hinge's dpoints, leaf after leaf
template <typename T>
__global__ __launch_bounds__(256) void accumulate_kernel(const T* __restrict__ add, int64_t n, T* __restrict__ sum) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) sum[i] += add[i];
}

// pvamd_composed_hinge_over_points_backward: composed_backward_kernel under the HINGE policy.  per_leaf: one pass per leaf s as
// the one-leaf composition (grids + s, the stack rows of s, upstream column s), its dtf rows written in place and its dpoints
// added to the sum in leaf order.  Scratch: the plan's slab and split rows, then (per_leaf, S > 1) one [P][3] leaf term.
static int64_t hinge_bwd_scratch_bytes(int S, int A, int64_t P, int per_leaf, size_t elem) {
    const BwdPlan b = bwd_plan(per_leaf ? 1 : S, A, P, elem);
    return (per_leaf && S > 1) ? b.leaf_off + P * 3 * (int64_t)elem : b.bytes;
}

template <typename T, bool WANT_TF, bool INTERP>
static void launch_hinge_backward(const BwdPlan& b, hipStream_t st, const pvamd_grid_t* grids, int S, const T* tf, int A,
                                  const T* pts, int64_t P, const T* up, int64_t up_stride, T margin, int power, T* dp_out, T* slab) {
    hipLaunchKernelGGL((composed_backward_kernel<T, true, false, WANT_TF, false, INTERP, true>), dim3((unsigned)b.nchunks, (unsigned)b.nsplit),
                       dim3(kBwdBlock), 0, st, grids, pvamd_grid_t{}, S, tf, A, pts, P, nullptr, nullptr, nullptr, T(0), b.aper, dp_out,
                       slab, up, up_stride, margin, power);
}

template <typename T>
static int hinge_backward(const pvamd_grid_t* grids, int32_t S, const T* tf, int32_t A, const T* points, int64_t P, int32_t mode,
                          int32_t per_leaf, T margin, int32_t power, const T* up, T* dpoints, T* dtf, void* scratch, void* stream) {
    if (S < 1 || S > kTfMaxLeaves || A < 1 || P < 1) return PVAMD_E_SHAPE;
    if ((mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) || (per_leaf != 0 && per_leaf != 1) ||
        (power != 1 && power != 2))
        return PVAMD_E_MODE;
    if (!dpoints && !dtf) return 0;
    if (!grids || !tf || !points || !up || !scratch) return PVAMD_E_NULL;
    if (!aligned_to(grids, 8) || !aligned_to(tf, sizeof(T)) || !aligned_to(points, sizeof(T)) || !aligned_to(up, sizeof(T)) ||
        !aligned_to(scratch, 16) || (dpoints && !aligned_to(dpoints, sizeof(T))) || (dtf && !aligned_to(dtf, sizeof(T))))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int Z = per_leaf ? S : 1, Sg = per_leaf ? 1 : S;
    const BwdPlan b = bwd_plan(Sg, A, P, sizeof(T));
    if (b.nchunks > 0x7fffffff) return PVAMD_E_SHAPE;
    T* slab = (T*)scratch;
    T* split_part = (T*)((char*)scratch + b.split_off);
    T* leaf_dp = (T*)((char*)scratch + b.leaf_off);
    const int64_t SgA = (int64_t)Sg * A;
    for (int z = 0; z < Z; ++z) {
        const pvamd_grid_t* gz = grids + (per_leaf ? z : 0);
        const T* tz = tf + (per_leaf ? (int64_t)z * A * 16 : 0);
        T* target = z == 0 ? dpoints : leaf_dp;
        T* dp_out = dpoints ? (b.nsplit > 1 ? split_part : target) : nullptr;
        if (mode == PVAMD_LEAF_TRILINEAR) {
            if (dtf) launch_hinge_backward<T, true, true>(b, st, gz, Sg, tz, A, points, P, up + z, Z, margin, power, dp_out, slab);
            else launch_hinge_backward<T, false, true>(b, st, gz, Sg, tz, A, points, P, up + z, Z, margin, power, dp_out, slab);
        } else {
            if (dtf) launch_hinge_backward<T, true, false>(b, st, gz, Sg, tz, A, points, P, up + z, Z, margin, power, dp_out, slab);
            else launch_hinge_backward<T, false, false>(b, st, gz, Sg, tz, A, points, P, up + z, Z, margin, power, dp_out, slab);
        }
        if (dtf) launch_reduce_tf<T, T>(slab, b.nchunks, SgA, dtf + (per_leaf ? (int64_t)z * A * 16 : 0), st);
        if (dpoints && b.nsplit > 1)
            hipLaunchKernelGGL(reduce_splits_kernel<T>, dim3(stream_grid(P * 3, 256)), dim3(256), 0, st, split_part, b.nsplit, P * 3,
                               target);
        if (dpoints && z > 0)
            hipLaunchKernelGGL(accumulate_kernel<T>, dim3(stream_grid(P * 3, 256)), dim3(256), 0, st, leaf_dp, P * 3, dpoints);
    }
    return (int)hipGetLastError();
}

template <typename T, bool INTERP = false>
static int cached_backward(const pvamd_grid_t* grid, const T* points, int64_t P, const T* dval, const T* dgrad, T* dpoints,
                           void* stream) {
    if (!grid || !dpoints) return PVAMD_E_NULL;
    if (P < 0) return PVAMD_E_SHAPE;
    if (int e = check_grid(*grid)) return e;
    if (grid->oob_mode != PVAMD_OOB_BOUNDING_BOX) return PVAMD_E_MODE;
    if (P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (!dval && !dgrad) {
        if (hipMemsetAsync(dpoints, 0, (size_t)P * 3 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
        return 0;
    }
    if (!points) return PVAMD_E_NULL;
    const dim3 grd(stream_grid(P, 256));
    if (dval && dgrad) hipLaunchKernelGGL((cached_backward_kernel<T, true, true, INTERP>), grd, dim3(256), 0, st, *grid, points, P, dval, dgrad, dpoints);
    else if (dval) hipLaunchKernelGGL((cached_backward_kernel<T, true, false, INTERP>), grd, dim3(256), 0, st, *grid, points, P, dval, dgrad, dpoints);
    else hipLaunchKernelGGL((cached_backward_kernel<T, false, true, INTERP>), grd, dim3(256), 0, st, *grid, points, P, dval, dgrad, dpoints);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int pvamd_cached_query_backward(const pvamd_grid_t* grid, const float* points, int64_t P, const float* dval,
                                           const float* dgrad, float* dpoints, void* stream) {
    return cached_backward<float>(grid, points, P, dval, dgrad, dpoints, stream);
}

extern "C" int pvamd_cached_query_backward_f64(const pvamd_grid_t* grid, const double* points, int64_t P, const double* dval,
                                               const double* dgrad, double* dpoints, void* stream) {
    return cached_backward<double>(grid, points, P, dval, dgrad, dpoints, stream);
}

extern "C" int64_t pvamd_composed_backward_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t is_f64) {
    if (S < 1 || A < 1 || P < 0) return 0;
    return bwd_scratch_bytes(S, A, P, is_f64 ? sizeof(double) : sizeof(float));
}

extern "C" int pvamd_composed_query_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                             int64_t P, const int32_t* out_leaf, const float* dval, const float* dgrad,
                                             float* dpoints, float* dtf, void* scratch, void* stream) {
    return composed_backward<float>(grids, nullptr, S, tf, A, points, P, out_leaf, dval, dgrad, 0.f, dpoints, dtf, scratch, stream,
                                    false);
}

extern "C" int pvamd_composed_query_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                 const double* points, int64_t P, const int32_t* out_leaf, const double* dval,
                                                 const double* dgrad, double* dpoints, double* dtf, void* scratch, void* stream) {
    return composed_backward<double>(grids, nullptr, S, tf, A, points, P, out_leaf, dval, dgrad, 0.0, dpoints, dtf, scratch,
                                     stream, false);
}

extern "C" int pvamd_chamfer_grid_backward(const pvamd_grid_t* grid, const float* W, int32_t B, const float* points, int64_t N,
                                           float scale, const float* dsum, float* dW, float* dpoints, void* scratch,
                                           void* stream) {
    if (!grid) return PVAMD_E_NULL;
    if (int e = check_grid(*grid)) return e;
    if (grid->oob_mode != PVAMD_OOB_BOUNDING_BOX) return PVAMD_E_MODE;
    return composed_backward<float>(nullptr, grid, 1, W, B, points, N, nullptr, dsum, nullptr, scale, dpoints, dW, scratch, stream,
                                    true);
}

// ---- the interpolated leaf (interpolation="trilinear"): the same kernels, reductions and argument checks ----
extern "C" int pvamd_cached_query_interp_backward(const pvamd_grid_t* grid, const float* points, int64_t P, const float* dval,
                                                  const float* dgrad, float* dpoints, void* stream) {
    return cached_backward<float, true>(grid, points, P, dval, dgrad, dpoints, stream);
}

extern "C" int pvamd_cached_query_interp_backward_f64(const pvamd_grid_t* grid, const double* points, int64_t P, const double* dval,
                                                      const double* dgrad, double* dpoints, void* stream) {
    return cached_backward<double, true>(grid, points, P, dval, dgrad, dpoints, stream);
}

extern "C" int pvamd_composed_query_interp_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A,
                                                    const float* points, int64_t P, const int32_t* out_leaf, const float* dval,
                                                    const float* dgrad, float* dpoints, float* dtf, void* scratch, void* stream) {
    return composed_backward<float, true>(grids, nullptr, S, tf, A, points, P, out_leaf, dval, dgrad, 0.f, dpoints, dtf, scratch,
                                          stream, false);
}

extern "C" int pvamd_composed_query_interp_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                        const double* points, int64_t P, const int32_t* out_leaf,
                                                        const double* dval, const double* dgrad, double* dpoints, double* dtf,
                                                        void* scratch, void* stream) {
    return composed_backward<double, true>(grids, nullptr, S, tf, A, points, P, out_leaf, dval, dgrad, 0.0, dpoints, dtf, scratch,
                                           stream, false);
}

// ---- hinge_over_points (include/pvamd.h "Hinge penalty over points") ----
extern "C" int64_t pvamd_hinge_over_points_backward_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t per_leaf, int32_t is_f64) {
    if (S < 1 || A < 1 || P < 1) return 0;
    return hinge_bwd_scratch_bytes(S, A, P, per_leaf, is_f64 ? sizeof(double) : sizeof(float));
}

extern "C" int pvamd_composed_hinge_over_points_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A,
                                                         const float* points, int64_t P, int32_t mode, int32_t per_leaf, float margin,
                                                         int32_t power, const float* up, float* dpoints, float* dtf, void* scratch,
                                                         void* stream) {
    return hinge_backward<float>(grids, S, tf, A, points, P, mode, per_leaf, margin, power, up, dpoints, dtf, scratch, stream);
}

extern "C" int pvamd_composed_hinge_over_points_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                             const double* points, int64_t P, int32_t mode, int32_t per_leaf,
                                                             double margin, int32_t power, const double* up, double* dpoints,
                                                             double* dtf, void* scratch, void* stream) {
    return hinge_backward<double>(grids, S, tf, A, points, P, mode, per_leaf, margin, power, up, dpoints, dtf, scratch, stream);
}
