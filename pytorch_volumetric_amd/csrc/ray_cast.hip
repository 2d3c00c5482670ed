// Fused sphere tracing (include/pvamd.h "Ray casting"): where a ray o + t d first meets the surface of a cached grid or of a
// composition, without the per-step launches and the (A, R) value and gradient fields of a loop around the point queries.
//
//   one lane per (configuration a, ray i), rays in caller order: 256-lane workgroups over (ceil(R / 256), A), so a row-major
//   image gives each wave a 64-pixel row segment
//   the step loop is wave-uniform: it runs while a wave vote says some lane is still marching, finished lanes are predicated
//   the loop body is the shared leaf layer unchanged -- MopLeaf<T, INTERP>::eval on one grid, mop_point<T, INTERP> on a
//   composition (composed_point.h) -- so (v, g) are the bits the point queries return at p
//   outputs are written once per ray after the loop; 24 B per ray in, 4 + 1 + 4 + 12 + 4 B (float32) out
// The leaf layer votes (wave_any in grid_lookup.h: the rare exact-index and small-norm branches) but moves nothing across
// lanes, and neither does this file: a vote under a partial EXEC mask counts the lanes that take part.  Grid descriptors and
// transform rows are wave-uniform and stay on the scalar path (the cached grid is a kernel argument, the composed ones are read
// through uniform addresses).  No scratch, no device -> host synchronisation, no atomics.
#include "common.h"
#include "composed_point.h"

namespace pvamd {

constexpr int kRayBlock = 256;

// the contract's separately rounded product and sum in float64 (exact_math.h states the float32 ones)
#pragma clang fp contract(off)
PVAMD_DEV double mul_rn(double a, double b) { return a * b; }
PVAMD_DEV double add_rn(double a, double b) { return a + b; }

template <typename T> PVAMD_DEV T ray_nan();
template <> PVAMD_DEV float ray_nan<float>() { return __builtin_nanf(""); }
template <> PVAMD_DEV double ray_nan<double>() { return __builtin_nan(""); }

template <typename T>
struct RayParams {
    T t_min, t_max, eps, step_scale;
    int max_steps;
};

template <typename T>
struct RayOut {
    T* t;
    uint8_t* status;
    T* val;
    T* grad;
    int32_t* steps;
};

// The contract's loop for one lane.  `live`: the lane holds a ray (false past the end of a partial workgroup: it never marches
// and writes nothing).  sdf(p, v, g): the point query at p.
template <typename T, class Sdf>
PVAMD_DEV void ray_march(const Sdf& sdf, bool live, const T* __restrict__ origins, const T* __restrict__ directions, int64_t i,
                         const RayParams<T>& rp, const RayOut<T>& out, int64_t o_idx) {
    T o[3] = {T(0), T(0), T(0)}, d[3] = {T(0), T(0), T(0)};
    if (live) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            o[j] = origins[3 * i + j];
            d[j] = directions[3 * i + j];
        }
    }
    T t = rp.t_min, v = ray_nan<T>(), g[3] = {ray_nan<T>(), ray_nan<T>(), ray_nan<T>()};
    T t_read = rp.t_min;  // the parameter of the last evaluated point: what is reported (after max_steps, t itself has moved on)
    int steps = 0;
    int status = PVAMD_RAY_MAX_STEPS;
    bool active = live & (t <= rp.t_max);
    if (!active) status = PVAMD_RAY_MISS;
#pragma unroll 1
    for (int k = 0; k < rp.max_steps && wave_any(active); ++k) {
        if (active) {
            const T p[3] = {add_rn(o[0], mul_rn(t, d[0])), add_rn(o[1], mul_rn(t, d[1])), add_rn(o[2], mul_rn(t, d[2]))};
            sdf(p, v, g);
            t_read = t;
            ++steps;
            if (v != v) {
                status = PVAMD_RAY_INVALID;
                active = false;
            } else if (v <= rp.eps) {
                status = PVAMD_RAY_HIT;
                active = false;
            } else {
                const T tn = add_rn(t, mul_rn(rp.step_scale, v));
                if (tn <= rp.t_max) {
                    t = tn;
                } else {
                    status = PVAMD_RAY_MISS;
                    active = false;
                }
            }
        }
    }
    if (live) {
        out.t[o_idx] = t_read;
        out.status[o_idx] = (uint8_t)status;
        out.val[o_idx] = v;
        out.grad[3 * o_idx] = g[0];
        out.grad[3 * o_idx + 1] = g[1];
        out.grad[3 * o_idx + 2] = g[2];
        out.steps[o_idx] = steps;
    }
}

// ---- one cached grid: the descriptor is a kernel argument ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(kRayBlock) void cached_ray_cast_kernel(const pvamd_grid_t g, const T* __restrict__ origins,
                                                                    const T* __restrict__ directions, int64_t R,
                                                                    const RayParams<T> rp, const RayOut<T> out) {
    const int64_t i = (int64_t)blockIdx.x * kRayBlock + threadIdx.x;
    auto sdf = [&](const T p[3], T& v, T gr[3]) {
        T o[4];
        MopLeaf<T, INTERP>::eval(g, p, o);
        v = o[0]; gr[0] = o[1]; gr[1] = o[2]; gr[2] = o[3];
    };
    ray_march<T>(sdf, i < R, origins, directions, i, rp, out, i);
}

// ---- a composition: blockIdx.y strides the configurations, outputs [A][R] ----
template <typename T, bool INTERP>
__global__ __launch_bounds__(kRayBlock) void composed_ray_cast_kernel(const pvamd_grid_t* __restrict__ grids, int S,
                                                                      const T* __restrict__ tf, int A,
                                                                      const T* __restrict__ origins,
                                                                      const T* __restrict__ directions, int64_t R,
                                                                      const RayParams<T> rp, const RayOut<T> out) {
    const int64_t i = (int64_t)blockIdx.x * kRayBlock + threadIdx.x;
    for (int a = blockIdx.y; a < A; a += gridDim.y) {
        auto sdf = [&](const T p[3], T& v, T gr[3]) {
            int s;
            mop_point<T, INTERP>(grids, 0, S, tf, A, a, p, v, gr, s);
        };
        ray_march<T>(sdf, i < R, origins, directions, i, rp, out, (int64_t)a * R + i);
    }
}

// host: the scalars of the contract in T, or an error before any launch
template <typename T>
static int ray_params(T t_min, T t_max, T eps, T step_scale, int32_t max_steps, RayParams<T>& rp) {
    if (max_steps < 1 || max_steps > 65535) return PVAMD_E_SHAPE;
    const T inf = (T)__builtin_inf();
    if (t_min != t_min || t_max != t_max) return PVAMD_E_MODE;
    if (!(eps >= T(0)) || !(eps < inf)) return PVAMD_E_MODE;
    if (!(step_scale > T(0)) || !(step_scale < inf)) return PVAMD_E_MODE;
    rp.t_min = t_min; rp.t_max = t_max; rp.eps = eps; rp.step_scale = step_scale; rp.max_steps = max_steps;
    return 0;
}

template <typename T>
static int ray_buffers(const T* origins, const T* directions, const RayOut<T>& out) {
    if (!origins || !directions || !out.t || !out.status || !out.val || !out.grad || !out.steps) return PVAMD_E_NULL;
    if (!aligned_to(origins, sizeof(T)) || !aligned_to(directions, sizeof(T)) || !aligned_to(out.t, sizeof(T)) ||
        !aligned_to(out.val, sizeof(T)) || !aligned_to(out.grad, sizeof(T)) || !aligned_to(out.steps, 4))
        return PVAMD_E_ALIGN;
    return 0;
}

template <typename T>
static int cached_ray_cast(const pvamd_grid_t* grid, int32_t mode, const T* origins, const T* directions, int64_t R, T t_min,
                           T t_max, T eps, T step_scale, int32_t max_steps, const RayOut<T>& out, void* stream) {
    const int64_t blocks = (R + kRayBlock - 1) / kRayBlock;
    if (R < 0 || blocks > 0x7fffffff) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    RayParams<T> rp;
    if (int e = ray_params<T>(t_min, t_max, eps, step_scale, max_steps, rp)) return e;
    if (!grid) return PVAMD_E_NULL;
    if (int e = check_grid(*grid)) return e;
    if (grid->oob_mode != PVAMD_OOB_BOUNDING_BOX) return PVAMD_E_MODE;
    if (R == 0) return 0;
    if (int e = ray_buffers<T>(origins, directions, out)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((cached_ray_cast_kernel<T, true>), dim3((unsigned)blocks), dim3(kRayBlock), 0, st, *grid, origins,
                           directions, R, rp, out);
    else
        hipLaunchKernelGGL((cached_ray_cast_kernel<T, false>), dim3((unsigned)blocks), dim3(kRayBlock), 0, st, *grid, origins,
                           directions, R, rp, out);
    return (int)hipGetLastError();
}

template <typename T>
static int composed_ray_cast(const pvamd_grid_t* grids, int32_t S, const T* tf, int32_t A, const T* origins, const T* directions,
                             int64_t R, int32_t mode, T t_min, T t_max, T eps, T step_scale, int32_t max_steps,
                             const RayOut<T>& out, void* stream) {
    const int64_t blocks = (R + kRayBlock - 1) / kRayBlock;
    if (S < 1 || A < 0 || R < 0 || blocks > 0x7fffffff) return PVAMD_E_SHAPE;
    if (mode != PVAMD_LEAF_NEAREST && mode != PVAMD_LEAF_TRILINEAR) return PVAMD_E_MODE;
    RayParams<T> rp;
    if (int e = ray_params<T>(t_min, t_max, eps, step_scale, max_steps, rp)) return e;
    if (R == 0 || A == 0) return 0;
    if (!grids || !tf) return PVAMD_E_NULL;
    if (!aligned_to(grids, 8) || !aligned_to(tf, sizeof(T))) return PVAMD_E_ALIGN;
    if (int e = ray_buffers<T>(origins, directions, out)) return e;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grd((unsigned)blocks, grid_rows(A));
    if (mode == PVAMD_LEAF_TRILINEAR)
        hipLaunchKernelGGL((composed_ray_cast_kernel<T, true>), grd, dim3(kRayBlock), 0, st, grids, S, tf, A, origins, directions, R,
                           rp, out);
    else
        hipLaunchKernelGGL((composed_ray_cast_kernel<T, false>), grd, dim3(kRayBlock), 0, st, grids, S, tf, A, origins, directions, R,
                           rp, out);
    return (int)hipGetLastError();
}

}  // namespace pvamd

using namespace pvamd;

extern "C" int pvamd_cached_ray_cast(const pvamd_grid_t* grid, int32_t mode, const float* origins, const float* directions,
                                     int64_t R, float t_min, float t_max, float eps, float step_scale, int32_t max_steps,
                                     float* out_t, uint8_t* out_status, float* out_val, float* out_grad, int32_t* out_steps,
                                     void* stream) {
    return cached_ray_cast<float>(grid, mode, origins, directions, R, t_min, t_max, eps, step_scale, max_steps,
                                  RayOut<float>{out_t, out_status, out_val, out_grad, out_steps}, stream);
}

extern "C" int pvamd_cached_ray_cast_f64(const pvamd_grid_t* grid, int32_t mode, const double* origins, const double* directions,
                                         int64_t R, double t_min, double t_max, double eps, double step_scale, int32_t max_steps,
                                         double* out_t, uint8_t* out_status, double* out_val, double* out_grad,
                                         int32_t* out_steps, void* stream) {
    return cached_ray_cast<double>(grid, mode, origins, directions, R, t_min, t_max, eps, step_scale, max_steps,
                                   RayOut<double>{out_t, out_status, out_val, out_grad, out_steps}, stream);
}

extern "C" int pvamd_composed_ray_cast(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* origins,
                                       const float* directions, int64_t R, int32_t mode, float t_min, float t_max, float eps,
                                       float step_scale, int32_t max_steps, float* out_t, uint8_t* out_status, float* out_val,
                                       float* out_grad, int32_t* out_steps, void* stream) {
    return composed_ray_cast<float>(grids, S, tf, A, origins, directions, R, mode, t_min, t_max, eps, step_scale, max_steps,
                                    RayOut<float>{out_t, out_status, out_val, out_grad, out_steps}, stream);
}

extern "C" int pvamd_composed_ray_cast_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                           const double* origins, const double* directions, int64_t R, int32_t mode, double t_min,
                                           double t_max, double eps, double step_scale, int32_t max_steps, double* out_t,
                                           uint8_t* out_status, double* out_val, double* out_grad, int32_t* out_steps,
                                           void* stream) {
    return composed_ray_cast<double>(grids, S, tf, A, origins, directions, R, mode, t_min, t_max, eps, step_scale, max_steps,
                                     RayOut<double>{out_t, out_status, out_val, out_grad, out_steps}, stream);
}
