// Gradient of the ray-cast hit distance (include/pvamd.h "Ray casting: gradient of the hit distance"): the surface-normal
// linearisation at the hit point, decisions (status, step count, winning leaf) held fixed -- not autograd through the step loop.
//
// Per (configuration a, ray i) with t, status and n = the gradient the forward returned at x = o + t d, all terms in float64
// from the query-dtype inputs, every product and sum rounded separately, left to right:
//   c = n0 d0 + n1 d1 + n2 d2;  the pair contributes only when status == HIT, c < 0 and c finite;  w = -up / c
//   do_i += w n,  dd_i += (w t) n
//   composition, winner s, M = tf[s*A+a], gamma_r = M[r][0] n0 + M[r][1] n1 + M[r][2] n2 (the leaf-frame record gradient):
//   dM[r][j] += (w gamma_r) x_j,  dM[r][3] += w gamma_r,  x_j = o_j + t d_j in float64
// One grid: elementwise, a lane per ray, no lookup (n is the saved gradient).  A composition: a lane per (configuration, ray) in
// the forward's geometry; (v, n, s) are recomputed at the forward's own p (mul_rn / add_rn in T) with mop_point unchanged, so n is
// the forward's bits and no leaf ids are stored.  Sums are composed_backward_kernel's (backward.hip) in float64:
// do / dd in registers in configuration order, configuration splits added in split order; the 12 entries of dM[s, a] by the
// stack-gradient reduction of tf_reduce.h (a butterfly per winning leaf, the waves in order, one slab row per (ray chunk,
// s*A + a): restated in the kernel below; the rows in chunk order: the header's reduce_tf_kernel).  Each sum is rounded once to T.  No float atomics, no device -> host synchronisation.
#include "common.h"
#include "composed_point.h"
#include "tf_reduce.h"

namespace pvamd {

constexpr int kRayBwdBlock = PVAMD_RAY_BACKWARD_CHUNK;  // one ray per lane, four waves
static_assert(kRayBwdBlock == kTfWaves * 64, "four waves per workgroup");

// the forward's separately rounded product and sum in float64 (ray_cast.hip; exact_math.h states the float32 ones)
#pragma clang fp contract(off)
PVAMD_DEV double mul_rn(double a, double b) { return a * b; }
PVAMD_DEV double add_rn(double a, double b) { return a + b; }

// c = n . d, left to right
template <typename T>
PVAMD_DEV double ray_facing(const T n[3], const T d[3]) {
    return add_rn(add_rn(mul_rn((double)n[0], (double)d[0]), mul_rn((double)n[1], (double)d[1])), mul_rn((double)n[2], (double)d[2]));
}

PVAMD_DEV bool ray_contributes(int status, double c) { return status == PVAMD_RAY_HIT && c < 0.0 && c > -__builtin_inf(); }

// ---- one cached grid: a lane per ray, no reduction ----
template <typename T>
__global__ __launch_bounds__(kRayBwdBlock) void cached_ray_cast_backward_kernel(
    const T* __restrict__ directions, int64_t R, const T* __restrict__ t, const uint8_t* __restrict__ status,
    const T* __restrict__ grad, const T* __restrict__ up, T* __restrict__ dorigins, T* __restrict__ ddirections) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += stride) {
        const T d[3] = {directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]};
        const T n[3] = {grad[3 * i], grad[3 * i + 1], grad[3 * i + 2]};
        const double c = ray_facing<T>(n, d);
        double go[3] = {0.0, 0.0, 0.0}, gd[3] = {0.0, 0.0, 0.0};
        if (ray_contributes(status[i], c)) {
            const double w = -(double)up[i] / c;
            const double wt = mul_rn(w, (double)t[i]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                go[j] = mul_rn(w, (double)n[j]);
                gd[j] = mul_rn(wt, (double)n[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (dorigins) dorigins[3 * i + j] = (T)go[j];
            if (ddirections) ddirections[3 * i + j] = (T)gd[j];
        }
    }
}

// ---- a composition ----
// Workgroup (chunk, split): rays [chunk * 256, +256) x configurations [split * aper, +aper).  rows == nullptr (one split): the
// lane rounds its do / dd once and writes them; else it leaves the float64 partial in rows[split][ray][6] for the finish kernel.
// slab: [chunk][s*A + a][12] float64, every row written (zeros for leaves that win nowhere in the chunk): it needs no clearing.
template <typename T, bool INTERP, bool WANT_TF>
__global__ __launch_bounds__(kRayBwdBlock) void composed_ray_cast_backward_kernel(
    const pvamd_grid_t* __restrict__ grids, int S, const T* __restrict__ tf, int A, const T* __restrict__ origins,
    const T* __restrict__ directions, int64_t R, const T* __restrict__ t, const uint8_t* __restrict__ status,
    const T* __restrict__ up, int aper, T* __restrict__ dorigins, T* __restrict__ ddirections, double* __restrict__ rows,
    double* __restrict__ slab) {
    __shared__ double part[kTfWaves][kTfMaxLeaves][12];
    __shared__ uint64_t present[kTfWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t chunk = blockIdx.x;
    const int split = blockIdx.y;
    const int a0 = split * aper;
    const int a1 = (a0 + aper) < A ? (a0 + aper) : A;
    const int64_t i = chunk * kRayBwdBlock + threadIdx.x;
    const bool live = i < R;

    T o[3] = {T(0), T(0), T(0)}, d[3] = {T(0), T(0), T(0)};
    if (live) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            o[j] = origins[3 * i + j];
            d[j] = directions[3 * i + j];
        }
    }
    double go[3] = {0.0, 0.0, 0.0}, gd[3] = {0.0, 0.0, 0.0};

    for (int a = a0; a < a1; ++a) {
        if (WANT_TF && lane == 0) present[wave] = 0;
        int s = -1;
        double c12[12] = {};
        const int64_t q = (int64_t)a * R + i;
        if (live && status[q] == PVAMD_RAY_HIT) {
            const T tt = t[q];
            const T p[3] = {add_rn(o[0], mul_rn(tt, d[0])), add_rn(o[1], mul_rn(tt, d[1])), add_rn(o[2], mul_rn(tt, d[2]))};
            T v, n[3];
            int sw;
            mop_point<T, INTERP>(grids, 0, S, tf, A, a, p, v, n, sw);
            const double c = ray_facing<T>(n, d);
            if (ray_contributes(PVAMD_RAY_HIT, c) && sw >= 0 && sw < S) {
                const double w = -(double)up[q] / c;
                const double wt = mul_rn(w, (double)tt);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    go[j] = add_rn(go[j], mul_rn(w, (double)n[j]));
                    gd[j] = add_rn(gd[j], mul_rn(wt, (double)n[j]));
                }
                if (WANT_TF) {
                    s = sw;
                    const T* M = tf + 16 * ((int64_t)sw * A + a);
                    double x[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) x[j] = add_rn((double)o[j], mul_rn((double)tt, (double)d[j]));
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const double gamma = add_rn(add_rn(mul_rn((double)M[4 * r], (double)n[0]), mul_rn((double)M[4 * r + 1], (double)n[1])),
                                                    mul_rn((double)M[4 * r + 2], (double)n[2]));
                        const double wg = mul_rn(w, gamma);
#pragma unroll
                        for (int j = 0; j < 3; ++j) c12[4 * r + j] = mul_rn(wg, x[j]);
                        c12[4 * r + 3] = wg;
                    }
                }
            }
        }
        if (WANT_TF) {
            // This kernel keeps its own copy of tf_reduce.h's tf_wave_reduce (a wave meets a leaf once per configuration, so
            // the slot rule only assigns) and tf_block_store: through the shared functions its rows did not stay inside the
            // parent's own spread (profiles/tf_reduce_shared.md).  The statements below must equal those two functions.
            uint64_t todo = __builtin_amdgcn_ballot_w64(s >= 0);
            while (todo) {  // wave-uniform: one butterfly per leaf that wins somewhere in the wave
                const int first = __builtin_ctzll(todo);
                const int sl = __builtin_amdgcn_readlane(s, first);
                const bool mine = s == sl;
                todo &= ~__builtin_amdgcn_ballot_w64(mine);
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    const double v = hop_wave_sum<double>(mine ? c12[j] : 0.0);
                    if (lane == 0) part[wave][sl][j] = v;
                }
                if (lane == 0) present[wave] |= 1ull << sl;
                PVAMD_WAVE_SYNC();
            }
            __syncthreads();
            for (int e = threadIdx.x; e < S * 12; e += kRayBwdBlock) {
                const int sl = e / 12, j = e - 12 * (e / 12);
                double v = 0.0;
#pragma unroll
                for (int w = 0; w < kTfWaves; ++w)
                    if ((present[w] >> sl) & 1ull) v += part[w][sl][j];
                slab[(chunk * ((int64_t)S * A) + (int64_t)sl * A + a) * 12 + j] = v;
            }
            __syncthreads();
        }
    }
    if (live) {
        if (rows) {
            double* out = rows + ((int64_t)split * R + i) * 6;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                out[j] = go[j];
                out[3 + j] = gd[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (dorigins) dorigins[3 * i + j] = (T)go[j];
                if (ddirections) ddirections[3 * i + j] = (T)gd[j];
            }
        }
    }
}

// do / dd [i][j] = T(sum over splits, in split order, of rows[split][i][j] / rows[split][i][3 + j])
template <typename T>
__global__ __launch_bounds__(256) void ray_reduce_rows_kernel(const double* __restrict__ rows, int nsplit, int64_t R,
                                                              T* __restrict__ dorigins, T* __restrict__ ddirections) {
    const int64_t n = R * 6;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t i = e / 6;
        const int j = (int)(e - 6 * i);
        double v = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) v += rows[(int64_t)sp * n + e];
        if (j < 3) {
            if (dorigins) dorigins[3 * i + j] = (T)v;
        } else if (ddirections) {
            ddirections[3 * i + j - 3] = (T)v;
        }
    }
}

// The launch geometry and the scratch layout of one composed pass (every partial is float64 whatever T).  The size function
// reports `bytes` and the launch code carves at the same offsets: the slab at 0, then the split rows.
struct RayBwdPlan : TfSplit {
    int64_t nchunks;
    int64_t rows_off;  // bytes: past the slab [nchunks][S*A][12]; the rows [nsplit][R][6] when nsplit > 1
    int64_t bytes;
};

static RayBwdPlan ray_bwd_plan(int S, int A, int64_t R) {
    RayBwdPlan b;
    b.nchunks = (R + kRayBwdBlock - 1) / kRayBwdBlock;
    if (b.nchunks < 1) b.nchunks = 1;
    static_cast<TfSplit&>(b) = tf_split_plan(b.nchunks, A);
    b.rows_off = tf_slab_bytes(b.nchunks * (int64_t)S * A, sizeof(double));
    b.bytes = b.rows_off + (b.nsplit > 1 ? (int64_t)b.nsplit * R * 6 * (int64_t)sizeof(double) : 0);
    return b;
}

template <typename T>
static int ray_backward_zero(T* dorigins, T* ddirections, int64_t R, T* dtf, int64_t SA, hipStream_t st) {
    if (dorigins && R > 0 && hipMemsetAsync(dorigins, 0, (size_t)R * 3 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
    if (ddirections && R > 0 && hipMemsetAsync(ddirections, 0, (size_t)R * 3 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
    if (dtf && SA > 0 && hipMemsetAsync(dtf, 0, (size_t)SA * 16 * sizeof(T), st) != hipSuccess) return (int)hipGetLastError();
    return (int)hipGetLastError();
}

template <typename T>
static int cached_ray_cast_backward(const T* directions, int64_t R, const T* t, const uint8_t* status, const T* grad, const T* up,
                                    T* dorigins, T* ddirections, void* stream) {
    if (R < 0) return PVAMD_E_SHAPE;
    if ((!dorigins && !ddirections) || R == 0) return 0;
    if (!directions || !t || !status || !grad || !up) return PVAMD_E_NULL;
    if (!aligned_to(directions, sizeof(T)) || !aligned_to(t, sizeof(T)) || !aligned_to(grad, sizeof(T)) || !aligned_to(up, sizeof(T)) ||
        (dorigins && !aligned_to(dorigins, sizeof(T))) || (ddirections && !aligned_to(ddirections, sizeof(T))))
        return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(cached_ray_cast_backward_kernel<T>, dim3(stream_grid(R, kRayBwdBlock)), dim3(kRayBwdBlock), 0,
                       (hipStream_t)stream, directions, R, t, status, grad, up, dorigins, ddirections);
    return (int)hipGetLastError();
}

template <typename T, bool INTERP>
static void launch_composed_ray_backward(const RayBwdPlan& b, hipStream_t st, const pvamd_grid_t* grids, int S, const T* tf, int A,
                                         const T* origins, const T* directions, int64_t R, const T* t, const uint8_t* status,
                                         const T* up, T* dorigins, T* ddirections, double* rows, double* slab) {
    const dim3 grid((unsigned)b.nchunks, (unsigned)b.nsplit);
    if (slab)
        hipLaunchKernelGGL((composed_ray_cast_backward_kernel<T, INTERP, true>), grid, dim3(kRayBwdBlock), 0, st, grids, S, tf, A, origins,
                           directions, R, t, status, up, b.aper, dorigins, ddirections, rows, slab);
    else
        hipLaunchKernelGGL((composed_ray_cast_backward_kernel<T, INTERP, false>), grid, dim3(kRayBwdBlock), 0, st, grids, S, tf, A, origins,
                           directions, R, t, status, up, b.aper, dorigins, ddirections, rows, slab);
}

template <typename T>
static int composed_ray_cast_backward(const pvamd_grid_t* grids, int32_t S, const T* tf, int32_t A, const T* origins,
                                      const T* directions, int64_t R, int32_t mode, const T* t, const uint8_t* status, const T* up,
                                      T* dorigins, T* ddirections, T* dtf, void* scratch, void* stream) {
    if (S < 1 || S > kTfMaxLeaves || A < 0 || R < 0) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    if (!dorigins && !ddirections && !dtf) return 0;
    if ((dorigins && !aligned_to(dorigins, sizeof(T))) || (ddirections && !aligned_to(ddirections, sizeof(T))) ||
        (dtf && !aligned_to(dtf, sizeof(T))))
        return PVAMD_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (A == 0 || R == 0) return ray_backward_zero<T>(dorigins, ddirections, R, dtf, (int64_t)S * A, st);  // nothing flows back
    if (!grids || !tf || !origins || !directions || !t || !status || !up) return PVAMD_E_NULL;
    const RayBwdPlan b = ray_bwd_plan(S, A, R);
    if (b.nchunks > 0x7fffffff) return PVAMD_E_SHAPE;
    const bool want_rows = b.nsplit > 1 && (dorigins || ddirections);
    if (!scratch && (dtf || want_rows)) return PVAMD_E_NULL;
    if (!aligned_to(grids, 8) || !aligned_to(tf, sizeof(T)) || !aligned_to(origins, sizeof(T)) || !aligned_to(directions, sizeof(T)) ||
        !aligned_to(t, sizeof(T)) || !aligned_to(up, sizeof(T)) || (scratch && !aligned_to(scratch, 16)))
        return PVAMD_E_ALIGN;
    double* slab = dtf ? (double*)scratch : nullptr;
    double* rows = want_rows ? (double*)((char*)scratch + b.rows_off) : nullptr;
    if (mode == PVAMD_LEAF_TRILINEAR)
        launch_composed_ray_backward<T, true>(b, st, grids, S, tf, A, origins, directions, R, t, status, up, dorigins, ddirections, rows,
                                              slab);
    else
        launch_composed_ray_backward<T, false>(b, st, grids, S, tf, A, origins, directions, R, t, status, up, dorigins, ddirections, rows,
                                               slab);
    if (dtf) launch_reduce_tf<double, T>(slab, b.nchunks, (int64_t)S * A, dtf, st);
    if (want_rows)
        hipLaunchKernelGGL(ray_reduce_rows_kernel<T>, dim3(stream_grid(R * 6, 256)), dim3(256), 0, st, rows, b.nsplit, R, dorigins,
                           ddirections);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int64_t pvamd_ray_cast_backward_scratch_bytes(int32_t S, int32_t A, int64_t R, int32_t is_f64) {
    if (S < 1 || A < 1 || R < 1 || (is_f64 != 0 && is_f64 != 1)) return 0;
    return ray_bwd_plan(S, A, R).bytes;  // float64 partials for either element type
}

extern "C" int pvamd_cached_ray_cast_backward(const float* directions, int64_t R, const float* t, const uint8_t* status,
                                              const float* grad, const float* up, float* dorigins, float* ddirections, void* stream) {
    return cached_ray_cast_backward<float>(directions, R, t, status, grad, up, dorigins, ddirections, stream);
}

extern "C" int pvamd_cached_ray_cast_backward_f64(const double* directions, int64_t R, const double* t, const uint8_t* status,
                                                  const double* grad, const double* up, double* dorigins, double* ddirections,
                                                  void* stream) {
    return cached_ray_cast_backward<double>(directions, R, t, status, grad, up, dorigins, ddirections, stream);
}

extern "C" int pvamd_composed_ray_cast_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* origins,
                                                const float* directions, int64_t R, int32_t mode, const float* t,
                                                const uint8_t* status, const float* up, float* dorigins, float* ddirections,
                                                float* dtf, void* scratch, void* stream) {
    return composed_ray_cast_backward<float>(grids, S, tf, A, origins, directions, R, mode, t, status, up, dorigins, ddirections, dtf,
                                             scratch, stream);
}

extern "C" int pvamd_composed_ray_cast_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                    const double* origins, const double* directions, int64_t R, int32_t mode,
                                                    const double* t, const uint8_t* status, const double* up, double* dorigins,
                                                    double* ddirections, double* dtf, void* scratch, void* stream) {
    return composed_ray_cast_backward<double>(grids, S, tf, A, origins, directions, R, mode, t, status, up, dorigins, ddirections, dtf,
                                              scratch, stream);
}
