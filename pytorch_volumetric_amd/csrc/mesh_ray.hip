// Ray x triangle kernels: the first hit of every ray on a prepared mesh, under two contracts of include/pvamd.h.
//   mesh_ray_cast ("Mesh ray casting"): per (pose, ray) the smallest t with its original face id, barycentrics and face normal
//                  -- what the reference gets from open3d's RaycastingScene.cast_rays on the scene every ObjectFactory keeps
//                  (reference sdf.py:115-118), where it is an Embree BVH traversal on CPU threads.  Every triangle is tested.
//   mesh_ray_cast_culled ("Mesh ray casting, culled"): the same, where a triangle counts only if the ray also passes a stated
//                  float32 test against the bounding spheres of the triangle's tile and group, and the hit's point lies in
//                  them: opt-in, a contract of its own.
//
// Structure of both: one workgroup = one wave, a lane owns one (pose, ray) pair for the whole launch -- no LDS, no barrier, no
// atomics.  Corners and face id come from planes 3 to 5 at wave-uniform addresses: one scalar load per wave and record, nothing
// per lane.  The division of a candidate's t and the two of its uv run only when some lane of the wave passed the edge tests.
// "Smallest t, then lowest original face id" does not depend on the order the candidates arrive in.
//
// mesh_ray_cast_kernel
//   * every wave walks ALL the records of the prepared mesh, tile by tile (masked by F: the last tile is padded), so the results
//     are the plain double loop's (tests/mesh_ray_ref.c) bit for bit, whatever order pvamd_mesh_prepare was given.
//   * NO culling, although the records carry bounding spheres per tile and per group.  The contract's candidate test is the
//     float32 sequence itself, and for a ray that lies, up to rounding, in a triangle's plane all of den, U, V and T are
//     rounding noise: the double loop then reports a candidate -- with any t -- wherever the line runs in that plane.  Measured
//     on the restatement with a box rotated into general position: of the rays in the plane of a face whose LINE passes more
//     than 3 units beside the box (corners 1.74 from its centre) about 1 in 2000 is a hit, and so is 1 in 2000 of those that point
//     away from the face with every corner behind the origin (tests/test_mesh_ray_cast_gpu.py runs both).  So neither a sphere missed by
//     the line, nor one behind the origin, nor one beyond a hit the lane already holds can be skipped provably under THIS
//     contract: a cull would have to know the planes inside the sphere, and the spheres do not.
//   * gfx950, hipcc -O3 -fno-slp-vectorize (ROCm 7.2): 31 VGPRs, 46 SGPRs, 0 AGPRs, 0 bytes of scratch, 0 bytes of LDS: 8 waves per
//     SIMD by registers.  The SLP vectoriser is off for this file, as for mesh.hip and composed.hip (csrc/Makefile): left on, it
//     packs parts of the exact test into v_pk_*_f32.  Measured on the drill, three alternating runs each
//     (tools/bench_mesh_ray_cast.py, profiles/mesh_ray_cast.md): 640 x 480 rays 4.66 ms without and 5.37 ms with it, 160 x 120 rays
//     x 20 poses 5.36 and 6.22 ms.
//
// mesh_ray_cast_culled_kernel
//   * the sphere tests are part of the definition, so skipping is exact: per tile the tile's sphere (a wave-uniform address)
//     against every lane's ray and a ballot -- zero skips the tile's 24 KB; then the spheres of the tile's live groups, each
//     ANDed with the lane's tile result, and a ballot per group; the records of the surviving groups go through the plain
//     kernel's candidate sequence with `inside && lane_ok`, and a candidate's point o + t d is tested against both spheres
//     (point_ok) where some lane holds one.  A wave executes the union of its lanes' surviving groups.
//   * nothing depends on the hit a lane already holds (the contract has no such rule: it would depend on the record order), so
//     the results are the restatement's (tests/mesh_ray_cull_ref.c) bit for bit.
//   * the plain kernel's ray, candidate sequence and outputs are restated in it: sharing them as inline functions (or as one
//     templated body) changed the plain kernel's register allocation and prologue, and its code is to stay as it is.
//   * same flags: 49 VGPRs, 106 SGPRs, 0 AGPRs, 0 bytes of scratch, 0 bytes of LDS, 7 waves per SIMD by registers.  Measured
//     (profiles/mesh_ray_cast_culled.md): 640 x 480 rays at the drill 0.38 ms against 4.58 ms, 160 x 120 rays x 20 poses 0.63
//     against 5.35 ms, 640 x 480 rays at the drill split into 251,648 triangles 1.46 against 76.7 ms; the same bits in all three.
#include "common.h"
#include "grid_lookup.h"
#include "mesh_math.h"
#include "mesh_records.h"

namespace pvamd {

struct RayArgs {
    const float* normal;
    const float* rec;
    int F;
    const float* origins;
    const float* directions;
    int64_t R;
    const float* poses;  // NULL: the rays are in the object frame already
    float t_min, t_max;
    float* t_out;
    int* face_out;
    float* normal_out;  // or NULL
    float* uv_out;      // or NULL
};

constexpr int kNoFace = 0x7fffffff;

// blockIdx.x: 64 consecutive rays; pose = b0 + blockIdx.y
__global__ __launch_bounds__(64) void mesh_ray_cast_kernel(RayArgs a, int b0) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool mine = r < a.R;
    const int64_t rr = mine ? r : a.R - 1;  // the tail lanes repeat the last ray and store nothing
    const int b = b0 + (int)blockIdx.y;
    V3 o = v3(a.origins[3 * rr], a.origins[3 * rr + 1], a.origins[3 * rr + 2]);
    V3 d = v3(a.directions[3 * rr], a.directions[3 * rr + 1], a.directions[3 * rr + 2]);
    const float* M = a.poses ? a.poses + 16 * (int64_t)b : nullptr;  // wave-uniform
    if (M) {
        const V3 p = o, q = d;
        o = v3(affine_row(M[0], M[1], M[2], M[3], p.x, p.y, p.z), affine_row(M[4], M[5], M[6], M[7], p.x, p.y, p.z),
               affine_row(M[8], M[9], M[10], M[11], p.x, p.y, p.z));
        d = v3(fmaf(M[2], q.z, fmaf(M[1], q.y, mul_rn(M[0], q.x))), fmaf(M[6], q.z, fmaf(M[5], q.y, mul_rn(M[4], q.x))),
               fmaf(M[10], q.z, fmaf(M[9], q.y, mul_rn(M[8], q.x))));
    }
    float best_t = INFINITY, best_u = 0.f, best_v = 0.f;
    int best_face = kNoFace;
    const int ntiles = (a.F + kTile - 1) / kTile;
    for (int ti = 0; ti < ntiles; ++ti) {
        const int n = min(kTile, a.F - ti * kTile);  // the last tile is padded
        const f32x4* PA = tile_plane(a.rec, ti, kPlaneA);
        const f32x4* PB = tile_plane(a.rec, ti, kPlaneB);
        const f32x4* PC = tile_plane(a.rec, ti, kPlaneC);
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const f32x4 A = PA[j], B = PB[j], C3 = PC[j];
            const V3 v0 = xyz(A), v1 = xyz(B), v2 = xyz(C3);
            // ray_hits_triangle's sequence up to T (mesh_math.h; include/pvamd.h "Mesh ray casting" 2.)
            const V3 e1 = sub(v0, v1), e2 = sub(v2, v0);
            const V3 Ng = cross(e2, e1);
            const V3 C = sub(v0, o);
            const V3 Rv = cross(C, d);
            const float den = dot(Ng, d);
            const float absden = fabsf(den);
            const float sgn = den < 0.f ? -1.f : 1.f;
            const float U = mul_rn(dot(Rv, e2), sgn);
            const float V = mul_rn(dot(Rv, e1), sgn);
            const float T = mul_rn(dot(Ng, C), sgn);
            const bool inside = (den != 0.f) && (U >= 0.f) && (V >= 0.f) && (add_rn(U, V) <= absden);
            if (__ballot(inside) == 0ull) continue;
            const float t = div_rn(T, absden);
            const int face = __float_as_int(A.w);
            if (inside && (t >= a.t_min) && (t <= a.t_max) && (t < best_t || (t == best_t && face < best_face))) {
                best_t = t;
                best_face = face;
                best_u = div_rn(U, absden);
                best_v = div_rn(V, absden);
            }
        }
    }
    if (!mine) return;
    const int64_t at = (int64_t)b * a.R + r;
    const bool hit = best_face != kNoFace;
    a.t_out[at] = best_t;
    a.face_out[at] = hit ? best_face : -1;
    if (a.uv_out) {
        a.uv_out[2 * at] = best_u;
        a.uv_out[2 * at + 1] = best_v;
    }
    if (a.normal_out) {
        V3 nrm = v3(0.f, 0.f, 0.f);
        if (hit) {
            const float* fn = a.normal + 3 * (int64_t)best_face;
            nrm = v3(fn[0], fn[1], fn[2]);
            if (M) {  // back into the rays' frame: R^T n, column j of the pose's rotation dotted with n
                const V3 k = nrm;
                nrm = v3(fmaf(M[8], k.z, fmaf(M[4], k.y, mul_rn(M[0], k.x))), fmaf(M[9], k.z, fmaf(M[5], k.y, mul_rn(M[1], k.x))),
                         fmaf(M[10], k.z, fmaf(M[6], k.y, mul_rn(M[2], k.x))));
            }
        }
        // + 0: a zero component leaves as +0 whatever its sign in the mesh and whatever the pose made of it
        a.normal_out[3 * at] = add_rn(nrm.x, 0.f);
        a.normal_out[3 * at + 1] = add_rn(nrm.y, 0.f);
        a.normal_out[3 * at + 2] = add_rn(nrm.z, 0.f);
    }
}

// What a lane keeps of its ray for the sphere tests of include/pvamd.h "Mesh ray casting, culled"
struct LaneWindow {
    float dd, len;  // dot(d', d'), its correctly rounded root
    float lo, hi;   // t_min * dd, t_max * dd
};

// sphere_ok of that section, for the sphere (c, r) at s[0..3] (a wave-uniform address)
PVAMD_DEV bool sphere_ok(const float* s, V3 o, V3 d, const LaneWindow& k) {
    const V3 w = sub(v3(s[0], s[1], s[2]), o);
    const V3 q = cross(w, d);
    const float qq = dot(q, q), ww = dot(w, w), wd = dot(w, d);
    // 4e-7 |w|: q and wd evaluated in float32 are within 4 * 2^-24 |w||d| = 2.4e-7 |w||d| of w x d and w . d (the header derives it)
    const float rs = fmaf(4e-7f, sqrt_rn(ww), mul_rn(s[3], 1.00001f));
    return (qq <= mul_rn(mul_rn(rs, rs), k.dd)) && (fmaf(rs, k.len, wd) >= k.lo) && (fmaf(-rs, k.len, wd) <= k.hi);
}

// point_ok of that section: the candidate's point o + t d lies in the inflated sphere at s[0..3]
PVAMD_DEV bool point_ok(const float* s, V3 o, V3 d, float t) {
    const V3 w = sub(v3(s[0], s[1], s[2]), o);
    const V3 v = v3(fmaf(t, d.x, -w.x), fmaf(t, d.y, -w.y), fmaf(t, d.z, -w.z));
    const float rs = fmaf(4e-7f, sqrt_rn(dot(w, w)), mul_rn(s[3], 1.00001f));
    return dot(v, v) <= mul_rn(rs, rs);
}

// The culled contract: mesh_ray_cast_kernel's ray, candidate sequence and outputs, restated (sharing them with it as inline
// functions changed its code), with sphere_ok and point_ok for the record's tile and group as further conditions of a
// candidate.  tiles: mesh->tiles.
__global__ __launch_bounds__(64) void mesh_ray_cast_culled_kernel(RayArgs a, int b0, const float* __restrict__ tiles) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool mine = r < a.R;
    const int64_t rr = mine ? r : a.R - 1;  // the tail lanes repeat the last ray and store nothing
    const int b = b0 + (int)blockIdx.y;
    V3 o = v3(a.origins[3 * rr], a.origins[3 * rr + 1], a.origins[3 * rr + 2]);
    V3 d = v3(a.directions[3 * rr], a.directions[3 * rr + 1], a.directions[3 * rr + 2]);
    const float* M = a.poses ? a.poses + 16 * (int64_t)b : nullptr;  // wave-uniform
    if (M) {
        const V3 p = o, q = d;
        o = v3(affine_row(M[0], M[1], M[2], M[3], p.x, p.y, p.z), affine_row(M[4], M[5], M[6], M[7], p.x, p.y, p.z),
               affine_row(M[8], M[9], M[10], M[11], p.x, p.y, p.z));
        d = v3(fmaf(M[2], q.z, fmaf(M[1], q.y, mul_rn(M[0], q.x))), fmaf(M[6], q.z, fmaf(M[5], q.y, mul_rn(M[4], q.x))),
               fmaf(M[10], q.z, fmaf(M[9], q.y, mul_rn(M[8], q.x))));
    }
    LaneWindow k;
    k.dd = dot(d, d);
    k.len = sqrt_rn(k.dd);
    k.lo = mul_rn(a.t_min, k.dd);
    k.hi = mul_rn(a.t_max, k.dd);
    float best_t = INFINITY, best_u = 0.f, best_v = 0.f;
    int best_face = kNoFace;
    const int ntiles = (a.F + kTile - 1) / kTile;
    for (int ti = 0; ti < ntiles; ++ti) {
        // the tile's sphere against every lane's ray: no lane passes, and the tile's 24 KB are not read
        const bool tile_ok = sphere_ok(tiles + 4 * (int64_t)ti, o, d, k);
        if (__ballot(tile_ok) == 0ull) continue;
        // the spheres of its live groups (those that begin at or past F have none and are not read), all before the first
        // record so that their loads are in flight together.  Bit g: this lane / some lane passed the tile and group g.
        const int n = min(kTile, a.F - ti * kTile);  // the last tile is padded
        const int ngroups = (n + kGroup - 1) / kGroup;
        const float* gs = tiles + 4 * ((int64_t)ntiles + (int64_t)ti * kGroupsPerTile);
        unsigned passed = 0u, any = 0u;
#pragma unroll
        for (int g = 0; g < kGroupsPerTile; ++g) {
            const bool ok = tile_ok && (g < ngroups) && sphere_ok(gs + 4 * min(g, ngroups - 1), o, d, k);
            passed |= ok ? (1u << g) : 0u;
            any |= __ballot(ok) != 0ull ? (1u << g) : 0u;
        }
        const f32x4* PA = tile_plane(a.rec, ti, kPlaneA);
        const f32x4* PB = tile_plane(a.rec, ti, kPlaneB);
        const f32x4* PC = tile_plane(a.rec, ti, kPlaneC);
        for (; any; any &= any - 1u) {  // wave-uniform: the groups some lane passed
            const int g = __builtin_ctz(any);
            const bool lane_ok = (passed >> g) & 1u;
            const int end = min(n, (g + 1) * kGroup);
#pragma unroll 4
            for (int j = g * kGroup; j < end; ++j) {
                const f32x4 A = PA[j], B = PB[j], C3 = PC[j];
                const V3 v0 = xyz(A), v1 = xyz(B), v2 = xyz(C3);
                // ray_hits_triangle's sequence up to T (mesh_math.h; include/pvamd.h "Mesh ray casting" 2.)
                const V3 e1 = sub(v0, v1), e2 = sub(v2, v0);
                const V3 Ng = cross(e2, e1);
                const V3 C = sub(v0, o);
                const V3 Rv = cross(C, d);
                const float den = dot(Ng, d);
                const float absden = fabsf(den);
                const float sgn = den < 0.f ? -1.f : 1.f;
                const float U = mul_rn(dot(Rv, e2), sgn);
                const float V = mul_rn(dot(Rv, e1), sgn);
                const float T = mul_rn(dot(Ng, C), sgn);
                const bool inside = lane_ok && (den != 0.f) && (U >= 0.f) && (V >= 0.f) && (add_rn(U, V) <= absden);
                if (__ballot(inside) == 0ull) continue;
                const float t = div_rn(T, absden);
                const int face = __float_as_int(A.w);
                // point_ok only where some lane holds a candidate: the two roots run for the few records a ray is inside of
                const bool in_spheres = point_ok(tiles + 4 * (int64_t)ti, o, d, t) && point_ok(gs + 4 * g, o, d, t);
                if (inside && (t >= a.t_min) && (t <= a.t_max) && in_spheres && (t < best_t || (t == best_t && face < best_face))) {
                    best_t = t;
                    best_face = face;
                    best_u = div_rn(U, absden);
                    best_v = div_rn(V, absden);
                }
            }
        }
    }
    if (!mine) return;
    const int64_t at = (int64_t)b * a.R + r;
    const bool hit = best_face != kNoFace;
    a.t_out[at] = best_t;
    a.face_out[at] = hit ? best_face : -1;
    if (a.uv_out) {
        a.uv_out[2 * at] = best_u;
        a.uv_out[2 * at + 1] = best_v;
    }
    if (a.normal_out) {
        V3 nrm = v3(0.f, 0.f, 0.f);
        if (hit) {
            const float* fn = a.normal + 3 * (int64_t)best_face;
            nrm = v3(fn[0], fn[1], fn[2]);
            if (M) {  // back into the rays' frame: R^T n, column j of the pose's rotation dotted with n
                const V3 c = nrm;
                nrm = v3(fmaf(M[8], c.z, fmaf(M[4], c.y, mul_rn(M[0], c.x))), fmaf(M[9], c.z, fmaf(M[5], c.y, mul_rn(M[1], c.x))),
                         fmaf(M[10], c.z, fmaf(M[6], c.y, mul_rn(M[2], c.x))));
            }
        }
        // + 0: a zero component leaves as +0 whatever its sign in the mesh and whatever the pose made of it
        a.normal_out[3 * at] = add_rn(nrm.x, 0.f);
        a.normal_out[3 * at + 1] = add_rn(nrm.y, 0.f);
        a.normal_out[3 * at + 2] = add_rn(nrm.z, 0.f);
    }
}

// every output of a call that has nothing to hit (F == 0 or t_min > t_max): +inf, -1, zeros
__global__ __launch_bounds__(256) void mesh_ray_miss_kernel(int64_t n, float* __restrict__ t_out, int* __restrict__ face_out,
                                                            float* __restrict__ normal_out, float* __restrict__ uv_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        t_out[i] = INFINITY;
        face_out[i] = -1;
        if (normal_out) normal_out[3 * i] = normal_out[3 * i + 1] = normal_out[3 * i + 2] = 0.f;
        if (uv_out) uv_out[2 * i] = uv_out[2 * i + 1] = 0.f;
    }
}

constexpr int kMaxRayFaces = 1 << 26;  // the limit of the other mesh entry points (csrc/mesh.hip kMaxFaces)

}  // namespace pvamd

using namespace pvamd;

// both entry points: the checks, the miss path and the pose slabs; culled: the kernel that also reads mesh->tiles
static int mesh_ray_cast(bool culled, const pvamd_mesh_t* mesh, const float* origins, const float* directions, int64_t R,
                         const float* poses, int32_t B, float t_min, float t_max, float* t_out, int32_t* face_out, float* normal_out,
                         float* uv_out, void* stream) {
    if (R < 0 || B < 0 || (!poses && B != 1)) return PVAMD_E_SHAPE;
    if (R >= ((int64_t)1 << 31) || (int64_t)B * R >= ((int64_t)1 << 31)) return PVAMD_E_SHAPE;
    if (!mesh) return PVAMD_E_NULL;
    if (mesh->F < 0 || mesh->F > kMaxRayFaces) return PVAMD_E_SHAPE;
    if (t_min != t_min || t_max != t_max) return PVAMD_E_MODE;
    if (R == 0 || B == 0) return 0;
    if (!origins || !directions || !t_out || !face_out) return PVAMD_E_NULL;
    if (mesh->F > 0 && (!mesh->rec || (normal_out && !mesh->normal) || (culled && !mesh->tiles))) return PVAMD_E_NULL;
    if (!aligned_to(mesh->rec, 16)) return PVAMD_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (mesh->F == 0 || t_min > t_max) {
        const int64_t n = (int64_t)B * R;
        hipLaunchKernelGGL(mesh_ray_miss_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, s, n, t_out, face_out, normal_out, uv_out);
        return (int)hipGetLastError();
    }
    RayArgs a;
    a.normal = mesh->normal;
    a.rec = mesh->rec;
    a.F = mesh->F;
    a.origins = origins;
    a.directions = directions;
    a.R = R;
    a.poses = poses;
    a.t_min = t_min;
    a.t_max = t_max;
    a.t_out = t_out;
    a.face_out = face_out;
    a.normal_out = normal_out;
    a.uv_out = uv_out;
    const float* tiles = mesh->tiles;
    for_row_slabs(B, [&](int32_t first, int32_t count) {
        const dim3 grid((unsigned)((R + 63) / 64), (unsigned)count);
        if (culled) hipLaunchKernelGGL(mesh_ray_cast_culled_kernel, grid, dim3(64), 0, s, a, first, tiles);
        else hipLaunchKernelGGL(mesh_ray_cast_kernel, grid, dim3(64), 0, s, a, first);
    });
    return (int)hipGetLastError();
}

extern "C" int pvamd_mesh_ray_cast(const pvamd_mesh_t* mesh, const float* origins, const float* directions, int64_t R,
                                   const float* poses, int32_t B, float t_min, float t_max, float* t_out, int32_t* face_out,
                                   float* normal_out, float* uv_out, void* stream) {
    return mesh_ray_cast(false, mesh, origins, directions, R, poses, B, t_min, t_max, t_out, face_out, normal_out, uv_out, stream);
}

extern "C" int pvamd_mesh_ray_cast_culled(const pvamd_mesh_t* mesh, const float* origins, const float* directions, int64_t R,
                                          const float* poses, int32_t B, float t_min, float t_max, float* t_out, int32_t* face_out,
                                          float* normal_out, float* uv_out, void* stream) {
    return mesh_ray_cast(true, mesh, origins, directions, R, poses, B, t_min, t_max, t_out, face_out, normal_out, uv_out, stream);
}
