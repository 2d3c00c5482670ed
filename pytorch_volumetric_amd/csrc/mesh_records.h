// The prepared triangle records as the mesh kernels read them (written by pvamd_mesh_prepare, csrc/mesh.hip).  Shared by
// mesh.hip and mesh_ray.hip.  gfx950 only.
#pragma once
#include "common.h"
#include "mesh_math.h"

namespace pvamd {

constexpr int kRec = PVAMD_TRI_REC;      // floats per record
constexpr int kTile = PVAMD_TRI_TILE;    // records per tile: 256 * 96 B = 24 KB
constexpr int kGroup = PVAMD_TRI_GROUP;  // records per group: own bounding sphere
constexpr int kGroupsPerTile = kTile / kGroup;
static_assert(kTile == 256 && kGroup == 16 && kRec == 24, "the scan is written for 256-record tiles of six float4 planes");
// A record is six float4s; a tile stores them plane by plane ([plane][256] float4, 24 KB, whole tiles allocated), so that
// 64 lanes reading the same plane of 64 consecutive records move one contiguous KB:
//   plane 0  ctr, r       bounding sphere (ctr = centre of the in-plane bounding rectangle)
//   plane 1  u,   hu      unit vector along the longest edge, half extent of the triangle along it (about ctr)
//   plane 2  v,   hv      unit in-plane vector across it, half extent
//   plane 3  a,   face id (bits)
//   plane 4  b,   m0      m0: absolute slack of the rectangle test (plane fit + rounding of the frame)
//   plane 5  c,   0
// `tiles` buffer: [ntiles][4] tile spheres, then [ntiles][16][4] group spheres.
enum { kPlaneSphere = 0, kPlaneU = 1, kPlaneV = 2, kPlaneA = 3, kPlaneB = 4, kPlaneC = 5 };
constexpr int kTileFloats = kTile * kRec;
PVAMD_DEV const f32x4* tile_plane(const float* rec, int tile, int plane) {
    return reinterpret_cast<const f32x4*>(rec + (int64_t)tile * kTileFloats + plane * (kTile * 4));
}
PVAMD_DEV f32x4 record_plane(const float* rec, int j, int plane) { return tile_plane(rec, j / kTile, plane)[j % kTile]; }
PVAMD_DEV V3 xyz(f32x4 v) { return v3(v.x, v.y, v.z); }

}  // namespace pvamd
