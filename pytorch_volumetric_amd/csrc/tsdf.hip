// TSDF fusion of depth images (include/pvamd.h "TSDF integration"): K frames are averaged into a truncated signed distance volume
// in one pass, and one more pass turns the volume into the packed records of a cached voxel grid.  Replaces nothing in the
// reference: its voxel.py stops at the containers.
//
//   tsdf_integrate_kernel  one lane per voxel over the flat index, grid-stride, so the lanes of a wave run along z.  The (F, W)
//                          pair is one 8-byte load; the frame loop runs inside the lane with the pair in registers, and a voxel
//                          some frame updated leaves as one 8-byte store.  K frames cost one read and one write of the volume,
//                          not K.  Pose k is read at an address that depends on the loop counter alone (wave-uniform: scalar
//                          loads).  The depth gathers of neighbouring z lanes fall on neighbouring pixels.
//   tsdf_records_kernel    one lane per voxel: its own pair and its six neighbours' through the cache, one 16-byte store.
// No LDS, no atomics, no scratch, no allocation, no host synchronisation.
#include "common.h"
#include "exact_math.h"

namespace pvamd {

struct TsdfCamera {
    float fx, fy, cx, cy;
    float u_end, v_end;  // (float)W - 0.5f, (float)H - 0.5f
    int H, W;
};

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(Lattice L, TsdfCamera cam, const float* __restrict__ depth, int K,
                                                             const float* __restrict__ camera_from_volume, float truncation,
                                                             float max_depth, float weight, float max_weight,
                                                             f32x2* __restrict__ state, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)L.n[1] * (unsigned)L.n[2];
    const int64_t image = (int64_t)cam.H * cam.W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Voxel at = voxel_of((unsigned)i, plane, (unsigned)L.n[2]);  // n <= PVAMD_TSDF_MAX_VOXELS
        const float c0 = add_rn(L.fmin[0], mul_rn((float)at.x, L.fres[0]));
        const float c1 = add_rn(L.fmin[1], mul_rn((float)at.y, L.fres[1]));
        const float c2 = add_rn(L.fmin[2], mul_rn((float)at.z, L.fres[2]));
        const f32x2 old = state[i];
        float F = old.x, Wt = old.y;
        bool touched = false;
        for (int k = 0; k < K; ++k) {
            const float* T = camera_from_volume + 12 * (int64_t)k;
            const float pz = add_rn(add_rn(add_rn(mul_rn(T[8], c0), mul_rn(T[9], c1)), mul_rn(T[10], c2)), T[11]);
            if (!(pz > 0.0f)) continue;
            const float px = add_rn(add_rn(add_rn(mul_rn(T[0], c0), mul_rn(T[1], c1)), mul_rn(T[2], c2)), T[3]);
            const float py = add_rn(add_rn(add_rn(mul_rn(T[4], c0), mul_rn(T[5], c1)), mul_rn(T[6], c2)), T[7]);
            const float u = add_rn(mul_rn(cam.fx, div_rn(px, pz)), cam.cx);
            const float v = add_rn(mul_rn(cam.fy, div_rn(py, pz)), cam.cy);
            if (!(u >= -0.5f && u < cam.u_end && v >= -0.5f && v < cam.v_end)) continue;  // NaN fails
            const int col = min(max((int)floorf(add_rn(u, 0.5f)), 0), cam.W - 1);
            const int row = min(max((int)floorf(add_rn(v, 0.5f)), 0), cam.H - 1);
            const float d = depth[k * image + (int64_t)row * cam.W + col];  // row, col inside the image; k < K
            if (!(d > 0.0f && d < __builtin_inff() && d <= max_depth)) continue;
            const float sdf = sub_rn(d, pz);
            if (!(sdf >= -truncation)) continue;
            const float f = fminf(div_rn(sdf, truncation), 1.0f);
            const float Wn = add_rn(Wt, weight);
            F = div_rn(add_rn(mul_rn(Wt, F), mul_rn(weight, f)), Wn);
            Wt = fminf(Wn, max_weight);
            touched = true;
        }
        if (touched) {
            f32x2 out;
            out.x = F;
            out.y = Wt;
            state[i] = out;
        }
    }
}

// statement 10 at one voxel
PVAMD_DEV float tsdf_value(const f32x2* __restrict__ state, int64_t i, float truncation, float min_weight, float unknown_tsdf) {
    const f32x2 s = state[i];
    return mul_rn(truncation, s.y > min_weight ? s.x : unknown_tsdf);
}

// statement 11 along one axis: this voxel's coordinate c of n, `step` flat indices per voxel of the axis
PVAMD_DEV float tsdf_slope(const f32x2* __restrict__ state, int64_t i, int c, int n, int64_t step, float resolution,
                           float truncation, float min_weight, float unknown_tsdf) {
    const int lo = max(c - 1, 0), hi = min(c + 1, n - 1);
    const float a = tsdf_value(state, i + (hi - c) * step, truncation, min_weight, unknown_tsdf);
    const float b = tsdf_value(state, i + (lo - c) * step, truncation, min_weight, unknown_tsdf);
    return div_rn(sub_rn(a, b), mul_rn((float)(hi - lo), resolution));
}

__global__ __launch_bounds__(256) void tsdf_records_kernel(const f32x2* __restrict__ state, int nx, int ny, int nz, float resolution,
                                                           float truncation, float min_weight, float unknown_tsdf,
                                                           f32x4* __restrict__ records, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned plane = (unsigned)ny * (unsigned)nz;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Voxel at = voxel_of((unsigned)i, plane, (unsigned)nz);  // n <= PVAMD_TSDF_MAX_VOXELS
        const float val = tsdf_value(state, i, truncation, min_weight, unknown_tsdf);
        const float gx = tsdf_slope(state, i, (int)at.x, nx, (int64_t)plane, resolution, truncation, min_weight, unknown_tsdf);
        const float gy = tsdf_slope(state, i, (int)at.y, ny, (int64_t)nz, resolution, truncation, min_weight, unknown_tsdf);
        const float gz = tsdf_slope(state, i, (int)at.z, nz, 1, resolution, truncation, min_weight, unknown_tsdf);
        const float len = sqrt_rn(add_rn(add_rn(mul_rn(gx, gx), mul_rn(gy, gy)), mul_rn(gz, gz)));
        f32x4 rec = {val, 0.0f, 0.0f, 0.0f};
        if (len > 0.0f) {
            rec.y = div_rn(gx, len);
            rec.z = div_rn(gy, len);
            rec.w = div_rn(gz, len);
        }
        records[i] = rec;
    }
}

static inline bool positive_finite(float a) { return a > 0.0f && a < __builtin_inff(); }
static inline bool is_finite(float a) { return a - a == 0.0f; }

}  // namespace pvamd

using namespace pvamd;

extern "C" int pvamd_tsdf_integrate(const pvamd_grid_t* grid, const float* depth, int32_t K, int32_t H, int32_t W,
                                    const float* camera_from_volume, float fx, float fy, float cx, float cy, float truncation,
                                    float max_depth, float weight, float max_weight, float* state, void* stream) {
    if (K < 0 || H < 1 || W < 1 || (int64_t)K * H * W > PVAMD_TSDF_MAX_PIXELS) return PVAMD_E_SHAPE;
    if (!grid) return PVAMD_E_NULL;
    const int32_t* shape = grid->shape;
    if (!lattice_shape_ok(shape[0], shape[1], shape[2], PVAMD_TSDF_MIN_AXIS, PVAMD_TSDF_MAX_VOXELS)) return PVAMD_E_SHAPE;
    if (int e = check_grid(*grid, /*need_vox=*/false)) return e;
    if (!positive_finite(fx) || !positive_finite(fy) || !is_finite(cx) || !is_finite(cy)) return PVAMD_E_MODE;
    if (!positive_finite(truncation) || !positive_finite(weight)) return PVAMD_E_MODE;
    if (!(max_depth > 0.0f) || !(max_weight > 0.0f)) return PVAMD_E_MODE;  // NaN included, +inf allowed
    if (K == 0) return 0;
    if (!depth || !camera_from_volume || !state) return PVAMD_E_NULL;
    if (!aligned_to(state, 8) || !aligned_to(depth, 4) || !aligned_to(camera_from_volume, 4)) return PVAMD_E_ALIGN;
    const Lattice L = lattice_of(*grid);
    const TsdfCamera cam = {fx, fy, cx, cy, (float)W - 0.5f, (float)H - 0.5f, H, W};
    const int64_t n = (int64_t)L.n[0] * L.n[1] * L.n[2];
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, L, cam, depth, K,
                       camera_from_volume, truncation, max_depth, weight, max_weight, reinterpret_cast<f32x2*>(state), n);
    return (int)hipGetLastError();
}

extern "C" int pvamd_tsdf_records(const float* state, int32_t nx, int32_t ny, int32_t nz, float resolution, float truncation,
                                  float min_weight, float unknown_tsdf, float* records, void* stream) {
    if (!lattice_shape_ok(nx, ny, nz, PVAMD_TSDF_MIN_AXIS, PVAMD_TSDF_MAX_VOXELS)) return PVAMD_E_SHAPE;
    const int64_t n = (int64_t)nx * ny * nz;
    if (!positive_finite(resolution) || !positive_finite(truncation) || min_weight != min_weight) return PVAMD_E_MODE;
    if (unknown_tsdf != 1.0f && unknown_tsdf != -1.0f) return PVAMD_E_MODE;
    if (!state || !records) return PVAMD_E_NULL;
    if (!aligned_to(state, 8) || !aligned_to(records, 16)) return PVAMD_E_ALIGN;
    hipLaunchKernelGGL(tsdf_records_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x2*>(state), nx, ny, nz, resolution, truncation, min_weight, unknown_tsdf,
                       reinterpret_cast<f32x4*>(records), n);
    return (int)hipGetLastError();
}
