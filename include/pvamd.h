/*
 * pvamd.h -- C ABI of libpvamd.so, the MI355X (gfx950) batched SDF query engine.
 *
 * The reference (UM-ARM-Lab/pytorch_volumetric @ 0.5.2) has no FFI: its boundary is the Python
 * ObjectFrameSDF protocol (sdf.py:217-246).  These entry points are what the Python classes in
 * pytorch_volumetric_amd/ bind with ctypes; each one replaces a *sequence* of stock torch ops /
 * Embree calls in the reference, cited per function below (paths relative to
 * src/pytorch_volumetric/ in the reference).
 *
 * Conventions (all entry points):
 *   - extern "C"; return 0 on success, <0 = invalid argument (PVAMD_E_*), >0 = hipError_t.
 *   - every pointer documented "device" is a device (HBM) address; "host" is ordinary memory.
 *   - fp32 buffers are dense row-major; points are AoS [P][3].
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) and the call returns without
 *     synchronising; nothing is allocated or freed; no static mutable state (re-entrant).
 *   - 4x4 transforms are row-major, column-vector convention: x' = M[:3,:3] x + M[:3,3]
 *     (chamfer.py:14, tests/test_model_to_sdf.py:277-279).
 *   - the Python binding is read from these declarations (pytorch_volumetric_amd/_header.py), and three parameter names carry
 *     meaning there: `pvamd_grid_t* grid`, `pvamd_mesh_t* mesh` and `pvamd_mesh_plan_t* plan_out` are HOST structs; a pointer
 *     under any other name (`grids`, `joints`, ...) is bound as a raw address.  One declaration per `;`, every parameter named.
 */
#ifndef PVAMD_H
#define PVAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVAMD_ABI_VERSION 16

#define PVAMD_E_NULL      (-1)  /* a required pointer is NULL            */
#define PVAMD_E_SHAPE     (-2)  /* a size/shape argument is out of range */
#define PVAMD_E_ALIGN     (-3)  /* a pointer is not 4-byte aligned       */
#define PVAMD_E_MODE      (-4)  /* unknown enum value                    */

/* sdf.py:436-438 OutOfBoundsStrategy */
#define PVAMD_OOB_LOOKUP_GT_SDF 0   /* kernel writes zeros + sets out_oob; caller queries gt_sdf on that subset */
#define PVAMD_OOB_BOUNDING_BOX  1   /* distance to the (unpadded) surface bounding box, sdf.py:555-571          */

/*
 * One cached voxel grid = the read-only state of a CachedSDF (sdf.py:441-525) plus the value-range
 * view the reference wraps around it (multidim_indexing TorchMultidimView, constructed sdf.py:521).
 *
 * HBM layout: ONE 16-byte record per voxel, vox[flat] = (val, gx, gy, gz), flat = (kx*ny + ky)*nz + kz
 * (C order: x slowest, z fastest -- voxel.py:20-25 cartesian_prod, sdf.py:504-505).  The reference keeps
 * two arrays (val [nx,ny,nz] and grad [n,3]); packing makes a query one 16-B gather.
 *
 * Index arithmetic is carried out in the dtype the reference's torch promotion would use:
 * index_f64 = 1 when the value range reached the view as float64 (numpy ranges, the README flow),
 * 0 when it reached it as float32 (python-float ranges).  Both triples are always filled in.
 *
 * `rule`: the choices of the view that NO reference test pins (multidim_indexing is an un-vendored, un-pinned
 * dependency; call sites sdf.py:521,537-540).  0 = what this library restates by default: the index is
 * round-half-to-even((p - min) / res), a point is valid when min <= p <= max (tested on the VALUE).  The bits
 * select the alternatives, so that matching the real package is a flag, not a kernel change:
 *   PVAMD_RULE_VALID_ON_INDEX   valid when 0 <= index < shape on the ROUNDED index (NaN / infinite quotients: invalid),
 *                               i.e. the range grows by half a voxel on every side
 *   PVAMD_RULE_ROUND_HALF_AWAY  index = round((p - min) / res), halves away from zero (C roundf / round)
 *   PVAMD_RULE_ROUND_FLOOR_HALF index = floor((p - min) / res + 0.5), the sum rounded in the index dtype
 *   PVAMD_RULE_RES_F64          (host side; nothing in the kernels reads it) a float32 range's resolution was evaluated
 *                               in float64 and then rounded to float32, instead of in float32 throughout
 * The query kernels' fast paths are rule-independent: their range test compares with vlo / vhi and their index
 * estimate falls back to the exact statement near every half-integer -- pvamd_grid_finalize() derives vlo / vhi for the
 * rule, and the exact statements (grid_lookup.h voxel_index_1d) follow it.
 */
#define PVAMD_RULE_VALID_ON_INDEX   1
#define PVAMD_RULE_ROUND_HALF_AWAY  2
#define PVAMD_RULE_ROUND_FLOOR_HALF 4
#define PVAMD_RULE_RES_F64          8
typedef struct pvamd_grid {
    const float* vox;        /* device, [nx*ny*nz][4]                                              */
    double       dmin[3];    /* range minimum per dim (float64 view)                               */
    double       dmax[3];    /* range maximum per dim                                              */
    double       dres[3];    /* (dmax-dmin)/(shape-1) evaluated in float64                         */
    float        fmin[3];    /* float32(range min)                                                 */
    float        fmax[3];    /* float32(range max)                                                 */
    float        fres[3];    /* (fmax-fmin)/float32(shape-1) evaluated in float32                  */
    float        bb_min[3];  /* gt_sdf.surface_bounding_box()[:,0], NO padding (sdf.py:525)        */
    float        bb_max[3];  /* ...[:,1]                                                           */
    int32_t      shape[3];   /* nx, ny, nz (each >= 2)                                             */
    int32_t      index_f64;  /* see above                                                          */
    int32_t      oob_mode;   /* PVAMD_OOB_*                                                        */
    int32_t      finalized;  /* set by pvamd_grid_finalize(); kernels refuse descriptors without it */
    /* ---- derived by pvamd_grid_finalize() from the fields above; callers do not fill these ---- */
    float        vlo[3];     /* smallest float32 p that is valid under `rule` (exact range test in fp32)       */
    float        vhi[3];     /* largest  float32 p that is valid                                             */
    float        inv32[3];   /* float32(1/res): the multiply-first index estimate, checked against a rounding */
    float        err32[3];   /* bound and redone with the exact IEEE division when it is within it            */
    /* ---- filled by the caller (before pvamd_grid_finalize) ---- */
    int32_t      rule;       /* PVAMD_RULE_* bits; 0 = the default restatement (occupies former padding)      */
    /* ---- float64 query points (the *_f64 entry points) ---- */
    double       dbb_min[3]; /* surface bounding box in float64: sdf.py:556-557 casts self.bb to the query dtype   */
    double       dbb_max[3];
    /* ---- derived by pvamd_grid_finalize() (ABI 11) ---- */
    float        range_n2;   /* the largest squared bounding-box distance fma(tz,tz,fma(ty,ty,tx*tx)) (sdf.py:559-568, float32)
                                any VALID p can have: the statements are monotone, so it is their value at the corner of
                                [vlo, vhi] farthest from the box.  n2 > range_n2 proves "out of range" with one compare.
                                +inf when the descriptor has no box (NaN bounds).                                   */
    float        reserved0;
} pvamd_grid_t;

/*
 * One triangle mesh = the read-only state of an ObjectFactory after precompute_sdf (sdf.py:97-120), prepared for the
 * kernels by pvamd_mesh_prepare().
 * normal:  device [F][3] fp32 unit face normals (sdf.py:119-120), indexed by ORIGINAL face id
 * rec:     device float[PVAMD_REC_FLOATS(F)] per-triangle records written by pvamd_mesh_prepare, in the (spatially
 *          sorted) order the caller chose, stored in whole tiles of PVAMD_TRI_TILE records (opaque layout: six float4
 *          planes per tile); each record carries its original face id
 * tiles:   device float[PVAMD_TILES_FLOATS(F)]: [T][4] bounding sphere (cx, cy, cz, r) of each run of PVAMD_TRI_TILE
 *          records (T = ceil(F/PVAMD_TRI_TILE)), followed by [T][PVAMD_TRI_TILE/PVAMD_TRI_GROUP][4] spheres of each run
 *          of PVAMD_TRI_GROUP records
 * rec_of_face: device [F] int32, position of the record of original face id f (inverse of the chosen order)
 * ray_dir: the reference passes bounding_box(padding=1.0)[:,1] as the last three floats of each ray
 *          (sdf.py:147-152); open3d reads those as the ray DIRECTION (tnear=0, tfar=inf).  Kept as float64
 *          because the reference adds its jitter in float64 before rounding to float32 (sdf.py:149-150).
 */
#define PVAMD_TRI_REC   24   /* floats per prepared triangle record */
#define PVAMD_TRI_TILE  256  /* triangles per tile / per tile sphere */
#define PVAMD_TRI_GROUP 16   /* triangles per group sphere */
#define PVAMD_REC_FLOATS(F) ((((F) + PVAMD_TRI_TILE - 1) / PVAMD_TRI_TILE) * PVAMD_TRI_TILE * PVAMD_TRI_REC)
#define PVAMD_TILES_FLOATS(F) ((((F) + PVAMD_TRI_TILE - 1) / PVAMD_TRI_TILE) * (4 + 4 * (PVAMD_TRI_TILE / PVAMD_TRI_GROUP)))
int64_t pvamd_mesh_rec_floats(int32_t F);    /* PVAMD_REC_FLOATS(F) */
int64_t pvamd_mesh_tiles_floats(int32_t F);  /* PVAMD_TILES_FLOATS(F) */
typedef struct pvamd_mesh {
    const float* normal;     /* device */
    const float* rec;        /* device */
    const float* tiles;      /* device */
    const int32_t* rec_of_face; /* device */
    int32_t      F;
    int32_t      reserved;
    double       ray_dir[3];
    uint64_t*    pair_counters; /* device, NULL (the default) or two counters the mesh kernels add to: exact closest-point tests
                                   and exact ray tests executed (measurement only: what the broad phase left to do)            */
} pvamd_mesh_t;

/* One frame of a kinematic tree (URDF link + the joint that attaches it to its parent), frames sorted parents-first. */
typedef struct pvamd_joint {
    int32_t parent;      /* index of the parent frame, -1 for the root                                       */
    int32_t jtype;       /* 0 fixed, 1 revolute / continuous, 2 prismatic                                    */
    int32_t jcol;        /* column of q that drives this joint (ignored for fixed joints)                    */
    int32_t leaf_slot;   /* s >= 0: also write this frame's world matrix to link_world_out[s*A + a]; -1: no  */
    float   axis[3];     /* unit joint axis in the joint frame                                               */
    float   reserved;
    float   origin[12];  /* rows 0..2 of the parent-link -> joint-frame transform (URDF <origin>)            */
} pvamd_joint_t;

int         pvamd_abi_version(void);
const char* pvamd_build_info(void);      /* static string: arch, compiler, build flags */
/* number of devices visible / name of device 0 -- lets a host language check the GPU without a HIP binding */
int         pvamd_device_count(void);

/* Host-side, pure: fill the derived fields of a descriptor (vlo/vhi/inv32/err32, finalized) from its primary
 * fields.  Must be called once after the primary fields are set and before the descriptor is used or uploaded.   */
int pvamd_grid_finalize(pvamd_grid_t* grid);

/* Build the packed voxel layout on device: out[i] = (val[i], grad[i][0..2]).  Replaces nothing in the
 * reference (layout choice); feeds every grid entry point.  val: device [n], grad: device [n][3], out: device [n][4]. */
int pvamd_pack_grid(const float* val, const float* grad, int64_t n, float* out, void* stream);

/* CachedSDF.__call__ (sdf.py:535-571): nearest-voxel lookup of (val, grad) with out-of-bounds handling.
 * grid: host.  points: device [P][3].  out_val: device [P].  out_grad: device [P][3].
 * out_oob: device [P] bytes or NULL; 1 where the point failed the range test (sdf.py:540-541).        */
int pvamd_cached_query(const pvamd_grid_t* grid, const float* points, int64_t P,
                       float* out_val, float* out_grad, uint8_t* out_oob, void* stream);

/* Host-side, pure: which kernel pvamd_cached_query launches for P points (one launch for any P; the choice depends on P
 * only) -- for tests that want every kernel covered and for a profile that wants to name the kernel it measured.        */
#define PVAMD_CQ_KERNEL_SCALAR     0  /* one point per lane, grid-stride                                  (P < 16,384) */
#define PVAMD_CQ_KERNEL_DIRECT_1   1  /* cached_query_direct: no LDS, 1 point per lane,  8 waves per workgroup        */
#define PVAMD_CQ_KERNEL_DIRECT_2   2  /*                              2 points per lane, 4 waves                      */
#define PVAMD_CQ_KERNEL_DIRECT_2W  3  /*                              2 points per lane, 16 waves (about 1M points)   */
#define PVAMD_CQ_KERNEL_DIRECT_4   4  /*                              4 points per lane, 4 waves                      */
#define PVAMD_CQ_KERNEL_WAVE_TILE  5  /* cached_query_wave: 256-point tiles through LDS                               */
#define PVAMD_CQ_KERNEL_STREAMING  6  /* cached_query_wave, streaming instantiation                      (P > 8M)    */
int pvamd_cached_query_kernel(int64_t P);

/* CachedSDF.outside_surface (sdf.py:593-602): OOB -> 1, else vox.val > level.  out: device [P] bytes. */
int pvamd_cached_outside(const pvamd_grid_t* grid, const float* points, int64_t P, float level,
                         uint8_t* out, void* stream);

/* The same three queries for FLOAT64 query points.  The reference returns the query dtype (sdf.py:545-547) and torch
 * promotion makes every operation on the points float64: (points - min) / resolution and the range test (sdf.py:537,
 * 540) whatever dtype the range had (dmin / dmax / dres above), the BOUNDING_BOX branch on self.bb.to(float64)
 * (sdf.py:556-571, dbb_min / dbb_max).  Cached values are float32 and are widened exactly.
 * points: device [P][3] float64.  out_val: device [P] float64.  out_grad: device [P][3] float64.                 */
int pvamd_cached_query_f64(const pvamd_grid_t* grid, const double* points, int64_t P,
                           double* out_val, double* out_grad, uint8_t* out_oob, void* stream);
int pvamd_cached_outside_f64(const pvamd_grid_t* grid, const double* points, int64_t P, double level,
                             uint8_t* out, void* stream);
int pvamd_voxel_index_f64(const pvamd_grid_t* grid, const double* points, int64_t P,
                          int64_t* out_key, int64_t* out_flat, uint8_t* out_valid, void* stream);

/* Voxel index arithmetic alone (TorchMultidimView.ensure_index_key / ravel_multi_index / get_valid_values as
 * used at sdf.py:537-540): out_key device [P][3] int64, out_flat device [P] int64, out_valid device [P] bytes.
 * Any output may be NULL.  This is the entry point the bit-exact index tests call.                     */
int pvamd_voxel_index(const pvamd_grid_t* grid, const float* points, int64_t P,
                      int64_t* out_key, int64_t* out_flat, uint8_t* out_valid, void* stream);

/* Dense voxel containers addressed by points (VoxelGrid.__getitem__ / __setitem__, voxel.py:97-103, over the value-range
 * view voxel.py:55): the same index arithmetic as above, reading or writing a caller-owned dense array in C order
 * (float32, or bytes for torch.bool grids).  grid->vox is not used.
 * gather:  out[i] = storage[flat(points[i])] where the point passes the range test, invalid_value elsewhere.
 * scatter: storage[flat(points[i])] = values[i] (or `scalar` when values is NULL) for the points that pass the range test,
 *          others are ignored.  When several points share a voxel the LAST one in input order wins, as in a sequential
 *          loop; that needs owner_scratch: device int32 [shape0*shape1*shape2] (required iff values != NULL).      */
int pvamd_voxel_gather_f32(const pvamd_grid_t* grid, const float* storage, const float* points, int64_t P,
                           float invalid_value, float* out, void* stream);
int pvamd_voxel_gather_u8(const pvamd_grid_t* grid, const uint8_t* storage, const float* points, int64_t P,
                          uint8_t invalid_value, uint8_t* out, void* stream);
int pvamd_voxel_scatter_f32(const pvamd_grid_t* grid, float* storage, const float* points, const float* values,
                            float scalar, int64_t P, int32_t* owner_scratch, void* stream);
int pvamd_voxel_scatter_u8(const pvamd_grid_t* grid, uint8_t* storage, const float* points, const uint8_t* values,
                           uint8_t scalar, int64_t P, int32_t* owner_scratch, void* stream);

/* ComposedSDF.__call__ over CachedSDF leaves (sdf.py:392-433 + 535-571 fused; also RobotSDF.__call__,
 * model_to_sdf.py:117-125): per configuration a and point p, x_s = T[s*A+a] p for every leaf s, look up leaf
 * s at x_s, rotate that gradient back with R^T, keep the first minimum over s.
 * grids: device [S] pvamd_grid_t (every oob_mode must be BOUNDING_BOX).  tf: device [S*A][4][4] obj->leaf,
 * leaf-major (model_to_sdf.py:100-113).  out_val: device [A][P].  out_grad: device [A][P][3].
 * out_leaf: device [A][P] int32 or NULL (arg-min leaf, for tests).
 * flags: 0, or PVAMD_COMPOSED_INLINE_EXACT -- a tuning hint that never changes a result: the kernels estimate a voxel
 * index in fp32 and fall back to the reference's exact division where the estimate is within its error bound (err32 of
 * pvamd_grid_finalize) of a rounding boundary.  By default flagged points are redone after the leaf loop (cheapest when
 * flags are rare and the grids are L2-resident, i.e. the kernel is instruction-bound); with the hint the exact statements
 * sit inline (cheapest for large, gather-bound grids, whose larger coordinate / resolution ratios also flag more visits).
 * The transforms must be RIGID (orthonormal 3x3, last row 0 0 0 1): the gradient is rotated back with R^T and the
 * leaf-culling bounds rely on distances being preserved.
 * Any P >= 0, any A >= 1 (the configuration is blockIdx.x: one launch for any count) and 1 <= S <= 2^30 - 2 (else
 * PVAMD_E_SHAPE; the same bound holds for the packed, bucketed and grouped entry points below); points / out_val /
 * out_grad need only their natural 4-byte alignment -- rows of an odd P (the reference README's M = 15,251) take the
 * same kernel.
 * The other bits below are for tests and tuning: they change which of three kernels serves the call, never a result;
 * pvamd_composed_query_kernel (below) tells which kernel a call takes.
 * Bits 8 and 16 of flags are retired (two tuning orders that nothing selected): ignored like any unassigned bit, and
 * not to be reused.                                                                                                  */
#define PVAMD_COMPOSED_INLINE_EXACT 1
#define PVAMD_COMPOSED_FORCE_PER_LANE 2   /* testing / tuning: take the one-point-per-lane kernel whatever the size */
#define PVAMD_COMPOSED_FORCE_WAVE_TILE 4  /* testing / tuning: take the wave-tile kernel whatever the size                 */
#define PVAMD_COMPOSED_NO_GROUPING 64   /* testing / tuning: never the chunk-grouped kernel (the round-5 kernels whatever the size) */
#define PVAMD_COMPOSED_FORCE_FUSED 128  /* testing / tuning: the chunk-grouped kernel with the in-workgroup sort whenever P >= one chunk */
#define PVAMD_COMPOSED_TILE_POINTS 256  /* points per wave tile: what the sorted / packed entry points below pad their points to */
#define PVAMD_COMPOSED_OUT_PACKED 32  /* pvamd_composed_query_grouped only: out_val takes [A][P] (val, gx, gy, gz) records (16-byte aligned), out_grad NULL */
int pvamd_composed_query(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A,
                         const float* points, int64_t P,
                         float* out_val, float* out_grad, int32_t* out_leaf, int32_t flags, void* stream);

/* Host-side, pure: which kernel pvamd_composed_query launches for A configurations of P points under `flags` (one launch
 * for any A and P; the choice depends on these three only, csrc/composed.hip composed_kind) -- for tests that want every
 * kernel covered at its default sizes and for callers that size their own path by it.  PVAMD_E_SHAPE for A < 1 or P < 0;
 * PVAMD_COMPOSED_INLINE_EXACT picks an instantiation inside the wave-tile and per-lane kernels and is not a kind. (ABI 15) */
#define PVAMD_CO_KERNEL_PER_LANE   0  /* composed_query_scalar: one point per lane, grid-stride                    */
#define PVAMD_CO_KERNEL_WAVE_TILE  1  /* composed_query_wave: 256-point tiles through LDS, per-tile leaf mask      */
#define PVAMD_CO_KERNEL_FUSED      2  /* composed_query_fused: 4096-point chunks regrouped inside the workgroup    */
int pvamd_composed_query_kernel(int32_t A, int64_t P, int32_t flags);

/* The same query for FLOAT64 points with a float64 transform stack (sdf.py:392-433 when the chain / the Transform3d is
 * float64: the transform, every leaf's index arithmetic, range test and bounding-box branch -- sdf.py:545-547 -- and the
 * gradient rotation are float64; cached records are widened exactly).  tf: device [S*A][4][4] float64.  points: device
 * [P][3] float64.  out_val: device [A][P] float64.  out_grad: device [A][P][3] float64.  8-byte alignment.            */
int pvamd_composed_query_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                             const double* points, int64_t P,
                             double* out_val, double* out_grad, int32_t* out_leaf, void* stream);

/* The glue of ComposedSDF.__call__ for leaves that are not cached grids (MeshSDF, SphereSDF, nested compositions;
 * sdf.py:392-433 around per-leaf queries), with the fused kernel's rounding so that both paths state the same numbers:
 * pvamd_transform_points: out[a][p] = tf[a] p (sdf.py:399).  tf: device [A][4][4] -- the A transforms of ONE leaf.
 *   points: device [P][3].  out: device [A][P][3].  Any P >= 0, any A >= 1.
 * pvamd_compose_merge: fold leaf s into the running first minimum (sdf.py:409,421): where leaf_val is smaller than
 *   best_val (or is NaN against a number; everywhere when first != 0) take it, with the gradient brought back to the
 *   object frame as L^T g (L = linear part of tf[a]; valid for any affine transform).  leaf_val / best_val: device [A][P].
 *   leaf_grad / best_grad: device [A][P][3].  best_leaf: device [A][P] int32 or NULL.  Any P >= 0, any A >= 1.        */
int pvamd_transform_points(const float* tf, int32_t A, const float* points, int64_t P, float* out, void* stream);
int pvamd_compose_merge(const float* tf, int32_t A, int64_t P, const float* leaf_val, const float* leaf_grad,
                        int32_t s, int32_t first, float* best_val, float* best_grad, int32_t* best_leaf, void* stream);

/* The same query when the caller has sorted the points spatially (e.g. along the Morton curve of pvamd_morton_keys):
 * coherent wave tiles let whole leaves be skipped and keep the leaf-grid region a tile touches in L2, which is what
 * decides the time once the grids are far larger than L2 (README-size link grids: 4.9 -> 1.6 ms for 200 x 262,144).
 * The kernel leaves one packed (val, gx, gy, gz) record per (configuration, sorted position) in `scratch` and a second
 * pass writes out_val / out_grad in the CALLER's point order: out[a][j] = record[a][inv[j]].  Same results, bit for
 * bit, as pvamd_composed_query on the unsorted points.
 * sorted_points: device [Pp][3], the P points in processing order followed by Pp - P copies of any of them (Pp a
 * multiple of PVAMD_COMPOSED_TILE_POINTS, 16-byte aligned).  inv: device [P] int32, position of caller point j in sorted_points.
 * scratch: device, A * Pp * 16 bytes, 16-byte aligned.  out_val: device [A][P].  out_grad: device [A][P][3].       */
int pvamd_composed_query_bucketed(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A,
                                  const float* sorted_points, const int32_t* inv, int64_t P, int64_t Pp,
                                  float* scratch, float* out_val, float* out_grad, int32_t flags, void* stream);

/* The same query with the points regrouped spatially INSIDE chunks of pvamd_group_chunk_points() consecutive points (round
 * 6; replaces nothing in the reference -- a processing order).  On scattered query points some of a wave's 64 lanes fall
 * inside a leaf's range at nearly every visit and the wave pays the look-up half for a handful of lanes; with neighbouring
 * points per wave most visits are all-outside (C4, 200 x 262,144 random points: 0.68 -> 0.5 ms).  A workgroup owns one chunk
 * and restores the caller's order through LDS, so -- unlike the globally sorted path above -- there is no second pass over
 * the outputs.  Same results, bit for bit, as pvamd_composed_query.
 * pvamd_group_points: sort every chunk of `points` (device [P][3], P >= pvamd_group_chunk_points()) once; the A
 *   configurations of a call -- and later calls on the same points -- share it.  scratch: device,
 *   pvamd_group_scratch_bytes(P) bytes, 16-byte aligned (sorted copy | bounding sphere per run of 256 | uint16 positions).
 * pvamd_composed_query_grouped: the query over that scratch.  flags: 0, or PVAMD_COMPOSED_OUT_PACKED (the records of
 *   pvamd_composed_query_packed, for any P: out_val = [A][P][4], out_grad = NULL); the INLINE_EXACT hint:
 *   PVAMD_E_MODE -- gather-bound grids gain nothing from the regrouping.  Any A >= 1, any P >= pvamd_group_chunk_points(), any 4-byte
 *   aligned outputs. */
int64_t pvamd_group_chunk_points(void);
int64_t pvamd_group_scratch_bytes(int64_t P);
int pvamd_group_points(const float* points, int64_t P, void* scratch, void* stream);
int pvamd_composed_query_grouped(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const void* scratch,
                                 int64_t P, float* out_val, float* out_grad, int32_t* out_leaf, int32_t flags, void* stream);

/* The two halves of the above, for callers that move the packed records themselves: RobotSDF.__call__
 * (model_to_sdf.py:117-125 -> sdf.py:392-433) sharded over GPUs runs on each rank's slice of the points, gathers ONE
 * buffer of records instead of val and grad, then unpacks straight into the reference's (A, P) / (A, P, 3) layout:
 * pvamd_composed_query_packed: out_rec[a][k] = (val, gx, gy, gz) of configuration a at points[k].  points: device [Pp][3],
 *   Pp a multiple of PVAMD_COMPOSED_TILE_POINTS, at most 2^24 * 4.  out_rec: device, A * Pp * 16 bytes, 16-byte aligned.  Any A.
 * pvamd_unpack_records: out_val[a][j] / out_grad[a][j] = rec[a * stride + index[j]] for j < P (index[j] may point
 *   anywhere in the buffer, e.g. into another rank's slab).  rec: device float4 records.  index: device [P] int32.   */
int pvamd_composed_query_packed(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                int64_t Pp, float* out_rec, int32_t flags, void* stream);
int pvamd_unpack_records(const float* rec, const int32_t* index, int64_t P, int64_t stride, int32_t A, float* out_val,
                         float* out_grad, void* stream);

/* Prepare a mesh for the query kernels: per-triangle records (corners, original face id, bounding sphere, and the
 * triangle's in-plane bounding rectangle: centre, two unit axes, half extents) plus one bounding sphere per run of
 * PVAMD_TRI_GROUP and of PVAMD_TRI_TILE records.  The bounds only ever SKIP work that provably cannot change a result
 * (computed in float64 for the rounded values stored, inflated by abs_margin and a relative 1e-5), so query results
 * are bit-identical to the untiled brute force whatever order the triangles are given in; input in compact runs of
 * PVAMD_TRI_GROUP / PVAMD_TRI_TILE triangles (the Python host: median-split patches of the centroids, mesh_io.patch_order;
 * half the radii of Z-order runs on a surface) is what makes the skipping effective.
 * tri: device [F][3][3] fp32 soup in the order to process.  face_id: device [F] int32 original ids, or NULL for 0..F-1.
 * abs_margin: absolute slack, >= 1e-6 * (largest |vertex coordinate| + bounding-box diagonal).
 * rec_out: device float[PVAMD_REC_FLOATS(F)] (16-byte aligned).  tiles_out: device float[PVAMD_TILES_FLOATS(F)]
 * (16-byte aligned).  F <= 2^26.
 * rec_of_face_out: device [F] int32.                                                                            */
int pvamd_mesh_prepare(const float* tri, const int32_t* face_id, int32_t F, float abs_margin, float* rec_out,
                       float* tiles_out, int32_t* rec_of_face_out, void* stream);

/* Axis-aligned bounds of the finite coordinates of a point set (the box pvamd_morton_keys wants).  points: device
 * [P][3].  box_out: device [2][3] fp32 (lo xyz, hi xyz); (+inf, -inf) for a dimension without finite values.     */
int pvamd_points_aabb(const float* points, int64_t P, float* box_out, void* stream);

/* 30-bit Z-order (Morton) key of every point inside the box [lo, hi]: the sort key for a spatially coherent
 * processing order (`order` below).  points: device [P][3].  box: device [2][3] fp32 (lo xyz, hi xyz).
 * keys_out: device [P] int32.                                                                                  */
int pvamd_morton_keys(const float* points, int64_t P, const float* box, int32_t* keys_out, void* stream);

/* A spatial processing order for a point set, in one call (bounds, cell counts, scan, scatter: seven small launches
 * instead of a general-purpose device sort): order_out[k] = index of the k-th point along a HILBERT curve (since ABI 9; a
 * Z-order curve before -- the name stayed) of 16^3 cells over the points' bounding box up to 16 k points (one launch),
 * 32^3 / 64^3 / 128^3 beyond 16 k / 64 k / 1 M: consecutive cells are face neighbours at every level, so the 64 points of
 * a wave are 25 % closer together than along the Z curve.  Points of one cell come out in an arbitrary, run-dependent
 * order -- the kernels that take an `order` return the same bits for any order.
 * order_out: device [P] int32.  inv_out: device [P] int32 or NULL, inv[order[k]] = k.  sorted_points_out: device [P][3] or
 * NULL, the points in that order.  scratch: device, pvamd_morton_order_scratch_bytes(P) bytes, 4-byte aligned (required for
 * any P, though one launch uses none).                                                                                 */
#define PVAMD_MORTON_ORDER_BITS(P) ((P) >= (1 << 20) ? 21 : ((P) >= (1 << 16) ? 18 : 15))
/* from 786,432 points on: (cell, index) pairs through a stable LSD radix sort (three 7-bit passes over 4096-pair tiles;
 * csrc/sort.hip) -- the points of a cell come out in index order.                                                    */
#ifndef PVAMD_ORDER_RADIX_SORT_FROM
#define PVAMD_ORDER_RADIX_SORT_FROM (3 << 18)  /* 786,432: counting sort 0.078 ms at 512 k, 0.166 at 1 M; radix 0.097 / 0.105 (profiles/r05_sort.txt) */
#endif
/* The larger of the two sorts' layouts (counting: bounds codes, cell counters, keys, block sums of the scan; radix: bounds
 * codes, supergroup totals, tile histograms, two key and two index arrays), so that the size does not depend on the threshold
 * a library was built with.  Host-only.                                                                                */
int64_t pvamd_morton_order_scratch_bytes(int64_t P);
int pvamd_morton_order(const float* points, int64_t P, int32_t* order_out, int32_t* inv_out, float* sorted_points_out,
                       void* scratch, void* stream);

/* Host-side, pure: which sort pvamd_morton_order runs for P points (the choice depends on P only, csrc/sort.hip order_kind),
 * and on how many leading bits of the 30-bit curve key it sorts: 12 in the one workgroup, PVAMD_MORTON_ORDER_BITS(P) beyond
 * -- for tests that want both sides of every threshold and restate neither.  PVAMD_E_SHAPE for a P that pvamd_morton_order
 * refuses. (ABI 16)                                                                                                    */
#define PVAMD_ORDER_KERNEL_SMALL     0  /* order_small_kernel: one workgroup, one launch, no scratch used             */
#define PVAMD_ORDER_KERNEL_COUNTING  1  /* the seven-launch counting sort; points of a cell in a run-dependent order  */
#define PVAMD_ORDER_KERNEL_RADIX     2  /* the LSD radix sort of (cell, index) pairs; points of a cell in index order */
int pvamd_morton_order_kernel(int64_t P);
int pvamd_morton_order_bits(int64_t P);

/* ObjectFactory._do_object_frame_closest_point (sdf.py:122-172): closest surface point, signed distance by
 * ray-hit parity, gradient, face id, optional face normal.
 * mesh: host struct with device pointers.  order: device [P] int32 permutation or NULL -- the k-th lane processes
 * point order[k] (spatially sorted processing makes the tile culling effective; outputs stay in point order).  jitter_seed: counter-based replacement for the reference's unseeded
 * np.random.randn (sdf.py:149); index_base = global index of points[0], so that a query sharded across GPUs
 * draws the jitter an unsharded one would.  out_closest: device [P][3] or NULL.  out_dist: device [P].  out_grad: device
 * [P][3].  out_face: device [P] int32 or NULL.  out_normal: device [P][3] or NULL (compute_normal=True).
 * scratch: device, PVAMD_MESH_SCRATCH_BYTES(P) bytes, 8-byte aligned, or NULL.  With it, the tiles of a 64-point group
 * are spread over several workgroups where one group's serial walk would set the time -- every group of a query of up to
 * PVAMD_MESH_SCRATCH_GROUPS groups (two launches: list, then parts + outputs), and the heavy groups of a larger one
 * (points about equidistant to much of a mesh of >= 128 tiles; three launches) -- meeting in scratch (per slot: the
 * group's points, rays, bounds, best (d^2, face) and hit counts); results are the same bits either way.  Contents on
 * return are unspecified.                                                                                          */
#define PVAMD_MESH_SCRATCH_GROUPS 8192  /* point groups (of 64) a scratch buffer has slots for: every group up to this many, ... */
/* ... then 8192 or an eighth of the groups, whichever is more (C5: 2.3 % of the groups are handed over; one that finds the
 * list full walks the mesh on its own two waves, 4x slower than the rest put together when that happens to thousands) */
#define PVAMD_MESH_SCRATCH_SLOTS(P) ((((P) + 63) / 64) < PVAMD_MESH_SCRATCH_GROUPS ? (((P) + 63) / 64) : \
                                     ((((P) + 63) / 64) / 8 > PVAMD_MESH_SCRATCH_GROUPS ? (((P) + 63) / 64) / 8 : PVAMD_MESH_SCRATCH_GROUPS))
#define PVAMD_MESH_SMALL_POINTS 16384  /* pvamd_mesh_query_unordered: at most this many points */
/* what pvamd_mesh_scratch_bytes returns (csrc/mesh.hip asserts it against the layout it carves): a header, 8 + 64 * 40 + 64
 * bytes per slot, 24 bytes per point of an unordered query */
#define PVAMD_MESH_SCRATCH_BYTES(P) (64 + PVAMD_MESH_SCRATCH_SLOTS(P) * (int64_t)(64 * 40 + 8 + 64) + 24 * PVAMD_MESH_SMALL_POINTS)
int64_t pvamd_mesh_scratch_bytes(int64_t P);
int64_t pvamd_mesh_small_points(void);  /* PVAMD_MESH_SMALL_POINTS */
int pvamd_mesh_query(const pvamd_mesh_t* mesh, const float* points, const int32_t* order, int64_t P,
                     uint64_t jitter_seed, int64_t index_base, float* out_closest, float* out_dist, float* out_grad, int32_t* out_face,
                     float* out_normal, void* scratch, void* stream);

/* Host-side, pure: the launches pvamd_mesh_query (unordered = 0), pvamd_mesh_query_unordered (unordered = 1) and
 * pvamd_cache_build (P = nx*ny*nz, unordered = 0) make for P points against a mesh of F faces, with (has_scratch != 0) or
 * without a scratch buffer -- csrc/mesh.hip mesh_query_plan, the one place that decides them; for tests that want every
 * path and every kernel instantiation covered at the sizes that reach it, and for a profile that wants to name what it
 * measured.  pvamd_chamfer_mesh_plan: the same for pvamd_chamfer_mesh (rows = B) and pvamd_chamfer_mesh_flat (rows = 1,
 * N = B * per).  Both return PVAMD_E_SHAPE for sizes the entry points refuse (and unordered with more than
 * PVAMD_MESH_SMALL_POINTS points), PVAMD_E_NULL without plan_out; a call that launches no mesh kernel (no points, no
 * rows, a chamfer against no faces) is PVAMD_MESH_PATH_NONE with every field 0. (ABI 16)                              */
#define PVAMD_MESH_PATH_NONE        0  /* nothing to do                                                                   */
#define PVAMD_MESH_PATH_LISTED      1  /* every group listed (hand_over_all / small_prep + gather), then mesh_parts_all_kernel<part_waves>,
                                          grid (groups, parts), which also writes the outputs                              */
#define PVAMD_MESH_PATH_SCAN        2  /* one launch of mesh_query_kernel / chamfer_mesh_kernel<scan_waves>                */
#define PVAMD_MESH_PATH_SCAN_HEAVY  3  /* that scan listing its heavy groups, mesh_parts_kernel over (list, parts), a finish launch */
#define PVAMD_MESH_ORDER_GIVEN      0  /* the caller's `order` (or none)                                                   */
#define PVAMD_MESH_ORDER_INSIDE     1  /* unordered: worked out by one workgroup of the first launch of the listed path    */
#define PVAMD_MESH_ORDER_SORT_CALL  2  /* unordered: a pvamd_morton_order call in front of the scan                        */
typedef struct pvamd_mesh_plan_t {
    int32_t path;        /* PVAMD_MESH_PATH_*                                                                             */
    int32_t order;       /* PVAMD_MESH_ORDER_*                                                                            */
    int32_t groups;      /* groups of 64 points: grid.x of the scan and of the listed launches (per row for a chamfer)     */
    int32_t slots;       /* PVAMD_MESH_SCRATCH_SLOTS of the point count: the groups a scratch buffer can list              */
    int32_t scan_waves;  /* waves per point group of the scan launch, 1 / 2 / 4 / 8; 0 on the listed path                  */
    int32_t parts;       /* workgroups the tiles of one listed group are spread over (grid.y of the parts launch); 0: scan */
    int32_t part_waves;  /* waves per workgroup of the parts launch, 2 or 4; 0 on the scan path                            */
} pvamd_mesh_plan_t;
int pvamd_mesh_query_plan(int64_t P, int32_t F, int32_t has_scratch, int32_t unordered, pvamd_mesh_plan_t* plan_out);
int pvamd_chamfer_mesh_plan(int64_t N, int32_t rows, int32_t F, int32_t has_scratch, pvamd_mesh_plan_t* plan_out);

/* CachedSDF construction from a mesh on the device (sdf.py:498-516: the ground-truth SDF over every voxel centre of the grid
 * voxel.py:20-25 builds, then the two arrays the reference keeps), in at most three launches for a small grid: the voxel
 * centres (cartesian product of the three coordinate arrays, x slowest) and a processing order that walks them in 4 x 4 x 4
 * bricks (inside 16^3 super-bricks) are written by one kernel -- no sort --, then pvamd_mesh_query's launches, whose last one writes the packed
 * (val, gx, gy, gz) record of voxel i = (x * ny + y) * nz + z straight into the cache.  Same bits as pvamd_mesh_query over the
 * same centres followed by pvamd_pack_grid (results do not depend on the processing order; the sign jitter is indexed by i).
 * cx / cy / cz: device [nx] / [ny] / [nz] float32.  out_packed: device [nx*ny*nz][4], 16-byte aligned.
 * points_scratch: device [nx*ny*nz][3] float32.  order_scratch: device [nx*ny*nz] int32.
 * scratch: device, PVAMD_MESH_SCRATCH_BYTES(nx*ny*nz) bytes, 8-byte aligned, or NULL.                                    */
int pvamd_cache_build(const pvamd_mesh_t* mesh, const float* cx, const float* cy, const float* cz, int32_t nx, int32_t ny,
                      int32_t nz, uint64_t jitter_seed, float* out_packed, float* points_scratch, int32_t* order_scratch,
                      void* scratch, void* stream);

/* The same query for at most PVAMD_MESH_SMALL_POINTS points that come without a processing order: the order is worked out
 * inside (into order_scratch: device [P] int32, contents on return = the order used), by one workgroup of a launch whose
 * other workgroups already do the per-point work that does not need it -- a separate pvamd_morton_order call in front of
 * pvamd_mesh_query costs a 10,000-point query a fifth of its time.  Same results, bit for bit.                       */
int pvamd_mesh_query_unordered(const pvamd_mesh_t* mesh, const float* points, int64_t P, uint64_t jitter_seed,
                               int64_t index_base, float* out_closest, float* out_dist, float* out_grad, int32_t* out_face,
                               float* out_normal, int32_t* order_scratch, void* scratch, void* stream);

/* The draw of sample_mesh_points (sdf.py:643-650: open3d's sample_points_uniformly + a random subset), counter-based so
 * that it is reproducible: sample i picks the triangle t with cdf[t-1] <= u < cdf[t] (u, r1, r2 = 53-bit uniforms from
 * splitmix64(seed, i)) and the point (1 - sqrt(r1)) a + sqrt(r1)(1 - r2) b + sqrt(r1) r2 c, in float64.
 * tri: device [F][3][3] fp32 corners (any order).  cdf: device [F] float64 inclusive cumulative area fractions
 * (non-decreasing, cdf[F-1] >= 1).  out_points: device [n][3] float64.  out_face: device [n] int32 index into tri, or
 * NULL.  out_key: device [n] int64 non-negative random keys (the n' smallest select a uniform random subset), or NULL. */
int pvamd_sample_surface(const float* tri, const double* cdf, int32_t F, int64_t n, uint64_t seed,
                         double* out_points, int32_t* out_face, int64_t* out_key, void* stream);

/* batch_chamfer_dist (chamfer.py:79-94) against a mesh: for each of B world->object transforms, transform the
 * N points, unsigned distance to the mesh, accumulate sum_n (scale*d)^2.  The caller divides by the GLOBAL N
 * (after an all-reduce when the points are sharded across GPUs).
 * W: device [B][4][4].  points: device [N][3].  order: as for pvamd_mesh_query, or NULL.
 * out_sum: device [B] float64, ZEROED by this call.  scratch: device, PVAMD_MESH_SCRATCH_BYTES(N) bytes, 8-byte aligned,
 * or NULL (as for pvamd_mesh_query: heavy point groups are spread over several workgroups; same sums up to the order of
 * the float64 additions).                                                                                     */
int pvamd_chamfer_mesh(const pvamd_mesh_t* mesh, const float* W, int32_t B, const float* points,
                       const int32_t* order, int64_t N, float scale, double* out_sum, void* scratch, void* stream);

/* The same sums when the caller has ALREADY transformed the points: points holds x[b][n] = W[b] p[n] for all B transforms
 * ([B][per][3], e.g. from pvamd_transform_points, whose rounding is the chamfer kernel's), and `order` walks all B * per
 * of them in ONE spatial order (pvamd_morton_order over the flat array).  Point i adds to out_sum[i / per].  What
 * pairwise_distance_chamfer / PlausibleDiversity want (chamfer.py:20-59,173-183: 10^4 transforms x 500 model points): with
 * few points per transform the 64 points a wave of pvamd_chamfer_mesh shares are a whole patch of the object apart and its
 * bounds cull little; in one global order they are neighbours (100 x 100 poses x 500 points on the drill: 12.3 -> 3.5 ms).
 * out_sum: device [B] float64, zeroed by this call.  scratch: PVAMD_MESH_SCRATCH_BYTES(B * per) bytes or NULL.          */
int pvamd_chamfer_mesh_flat(const pvamd_mesh_t* mesh, int32_t B, const float* points, const int32_t* order, int64_t per,
                            float scale, double* out_sum, void* scratch, void* stream);

/* Same against a cached grid (obj_sdf branch, chamfer.py:84-85).  grid: host.                            */
int pvamd_chamfer_grid(const pvamd_grid_t* grid, const float* W, int32_t B, const float* points, int64_t N,
                       float scale, double* out_sum, void* stream);

/* RobotSDF.set_joint_configuration's contraction (model_to_sdf.py:104-113): out[s*A+a] = offset_inv[s] @
 * rigid_inverse(link_world[s*A+a]).  offset_inv: device [S][4][4].  link_world: device [S*A][4][4] leaf-major.
 * out: device [S*A][4][4].  The 4x4x4 products run on the f32 MFMA (v_mfma_f32_4x4x1_16b_f32).            */
int pvamd_transform_stack(const float* offset_inv, const float* link_world, int32_t S, int32_t A,
                          float* out, void* stream);

/* Forward kinematics for A configurations (RobotSDF.set_joint_configuration, model_to_sdf.py:94-102):
 * world[f] = world[parent f] @ origin[f] @ motion(joint f, q).  joints: device [F].  q, sin_q, cos_q: device [A][M]
 * (joint values and their sine / cosine).  scratch: device [F][12][A] fp32 (all frames' matrices, rows 0..2, kept for
 * children to read).  link_world_out: device [S*A][4][4], leaf-major, the input of pvamd_transform_stack.          */
int pvamd_chain_fk(const pvamd_joint_t* joints, int32_t F, const float* q, const float* sin_q, const float* cos_q,
                   int32_t A, int32_t M, float* scratch, float* link_world_out, void* stream);

/* PlausibleDiversity's reduction of the (B, P) pairwise chamfer matrix (chamfer.py:185-195) in one pass: per row / per column
 * the minimum and where it is (first index on ties, a NaN counts as the minimum: torch.min), and means[0] = mean of the row
 * minima (plausibility), means[1] = mean of the column minima (coverage), summed in float64 in a fixed order.
 * errors: device [B][P] float32 (is_f64 = 0) or float64.  row_val / col_val: device [B] / [P] of the same dtype.
 * row_idx / col_idx: device int64.  means: device [2] float64.                                                          */
int pvamd_pairwise_min_reduce(const void* errors, int32_t is_f64, int32_t B, int32_t P, void* row_val, int64_t* row_idx,
                              void* col_val, int64_t* col_idx, double* means, void* stream);

/* The whole of RobotSDF.set_joint_configuration (model_to_sdf.py:94-113) in ONE launch, from joint values that already sit
 * on the device: sin / cos, the frame walk of pvamd_chain_fk, and stack_out[s*A+a] = offset_inv[s] @
 * rigid_inverse(world[leaf s, a]) (the f32-MFMA statement of pvamd_transform_stack) -- the obj->leaf stack that
 * pvamd_composed_query consumes.  q: device [A][M].  offset_inv: device [S][4][4].  sincos_out: device [A][M][2] (sin, cos
 * of every revolute joint value, as used: feed them to a CPU restatement to reproduce the stack bit for bit) or NULL.
 * scratch: device [F][12][A] fp32.  link_world_out: device [S*A][4][4] leaf-major or NULL.  stack_out: device [S*A][4][4].
 * At most 50 SDF-carrying links (the leaf frames of 64 configurations are staged in LDS).  Graph-capturable: no host
 * data, no allocation, one kernel.                                                                                   */
int pvamd_configure_chain(const pvamd_joint_t* joints, int32_t F, const float* q, int32_t A, int32_t M,
                          const float* offset_inv, int32_t S, float* sincos_out, float* scratch,
                          float* link_world_out, float* stack_out, void* stream);

/* ---- Backward (vector-Jacobian products) for torch autograd (ABI 13) ----
 * The gradient torch autograd would produce through the reference's expressions, GIVEN THE FORWARD'S DECISIONS (which leaf
 * won the first minimum, whether the point was in range, which voxel it fell in, which axes are active in the bounding-box
 * branch).  In range the value and gradient are a table lookup without a derivative w.r.t. the point (sdf.py:549-550);
 * outside (BOUNDING_BOX, sdf.py:556-571) with d the signed per-axis excess over the box and n = d / |d|:
 *   d val / dx = n,   d grad / dx = (I - n n^T) diag(active) / |d|   (active: the axes on which x lies outside the box).
 * Upstream gradients dval / dgrad may each be NULL (= zero); outputs are OVERWRITTEN, not accumulated.  Every sum is a
 * fixed-order reduction: two calls with the same inputs give the same bits.  Allocation-free and stream-ordered.
 *
 * pvamd_cached_query_backward: dpoints[i] = the VJP at points[i] (CachedSDF.__call__, BOUNDING_BOX grids only: PVAMD_E_MODE
 *   otherwise).  points / dpoints: device [P][3].  dval: device [P] or NULL.  dgrad: device [P][3] or NULL.              */
int pvamd_cached_query_backward(const pvamd_grid_t* grid, const float* points, int64_t P, const float* dval,
                                const float* dgrad, float* dpoints, void* stream);
int pvamd_cached_query_backward_f64(const pvamd_grid_t* grid, const double* points, int64_t P, const double* dval,
                                    const double* dgrad, double* dpoints, void* stream);

/* pvamd_composed_query_backward: ComposedSDF.__call__ over BOUNDING_BOX CachedSDF leaves (sdf.py:399,409,421-426).  Per pair
 * (a, p) with s = out_leaf[a][p] (the forward's arg-min, from pvamd_composed_query / _grouped / _f64), L, t = tf[s*A+a]:
 * x = L p + t is recomputed with the forward's fma chain, gg = L^T g.  The gradient reaches p, L and t of the winner only.
 * grids / tf / points / out_leaf: as given to the forward.  dval: device [A][P] or NULL.  dgrad: device [A][P][3] or NULL.
 * dpoints: device [P][3] or NULL (sum over configurations).  dtf: device [S*A][4][4] or NULL (sum over points; row 3 = 0).
 * scratch: device, pvamd_composed_backward_scratch_bytes(S, A, P, is_f64) bytes, 16-byte aligned (the per-workgroup slab of
 * dtf partials and, when the configurations are split over workgroups, the per-split dpoints partials).  1 <= S <= 64.  */
int64_t pvamd_composed_backward_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t is_f64);
int pvamd_composed_query_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                  int64_t P, const int32_t* out_leaf, const float* dval, const float* dgrad, float* dpoints,
                                  float* dtf, void* scratch, void* stream);
int pvamd_composed_query_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* points,
                                      int64_t P, const int32_t* out_leaf, const double* dval, const double* dgrad,
                                      double* dpoints, double* dtf, void* scratch, void* stream);

/* pvamd_chamfer_grid_backward: batch_chamfer_dist against a BOUNDING_BOX cached grid (chamfer.py:82-94) with upstream dsum[b]
 * on the per-transform SUM of (scale d)^2 (the caller folds the 1 / N of the mean into it).  Needs no saved tensors: in-range
 * pairs contribute zero and out-of-range ones depend on x = W[b] p and the box only.  W: device [B][4][4].  points: device
 * [N][3].  dsum: device [B].  dW: device [B][4][4] or NULL.  dpoints: device [N][3] or NULL.
 * scratch: pvamd_composed_backward_scratch_bytes(1, B, N, 0) bytes, 16-byte aligned.                                       */
int pvamd_chamfer_grid_backward(const pvamd_grid_t* grid, const float* W, int32_t B, const float* points, int64_t N,
                                float scale, const float* dsum, float* dW, float* dpoints, void* scratch, void* stream);

/* ---- Interpolated queries (CachedSDF / ComposedSDF with interpolation="trilinear"; opt-in, nearest-voxel stays the default) ----
 * The same descriptors (pvamd_grid_t is unchanged): the entry point chooses the mode.  T is the query dtype: float32 points use
 * fmin / fres and float32 arithmetic whatever index_f64 says, float64 points dmin / dres.  R[i][j][k] is the record
 * (val, gx, gy, gz), n_d = shape[d].
 *  1. The range decision is the nearest mode's, bit for bit (vlo / vhi under the grid's rule; voxel_key_f64 for float64).  Points
 *     that fail it take the out-of-range branch, and their val / grad are IDENTICAL to the nearest mode's (BOUNDING_BOX: the
 *     distance to the surface box; LOOKUP_GT_SDF: zeros and out_oob = 1, the caller fills in the ground truth).
 *  2. Per axis d: s = (x_d - min_d) / res_d (IEEE subtraction, then IEEE division); c = s < 0 ? 0 : (s > n_d - 1 ? n_d - 1 : s),
 *     clamped_d = (c != s) (under PVAMD_RULE_VALID_ON_INDEX valid points reach half a voxel beyond the end centres: the value
 *     is held constant there); i_d = min(floor(c), n_d - 2); f_d = c - i_d (exact).
 *  3. lerp(a, b, f) = fma(f, b - a, a).  Per channel q: e_ab = lerp(R[i+a][j+b][k][q], R[i+a][j+b][k+1][q], f_z) for (a, b) in
 *     (0,0), (0,1), (1,0), (1,1); y_a = lerp(e_a0, e_a1, f_y); out_q = lerp(y_0, y_1, f_x).
 *  4. The returned gradient is the interpolated stored gradient, not renormalised (norm <= 1 up to rounding); it is NOT
 *     d val / dx, which the backward computes exactly.
 *  5. Backward: torch autograd through these expressions given the forward's decisions (range, cell, clamped axes, winning
 *     leaf): d lerp / d f = b - a, d f_d / d x_d = 1 / res_d (upstream / res_d), 0 on a clamped axis; out of range the
 *     BOUNDING_BOX VJP of pvamd_cached_query_backward.
 *  6. Composed: the nearest kernels' leaf transform (affine_row in float32, the fma chain of pvamd_composed_query_f64 in
 *     float64), the same first-minimum comparison over leaves, the winner's gradient rotated back with the same statements.
 *
 * pvamd_cached_query_interp / _f64: as pvamd_cached_query / _f64 (same arguments, out_oob optional).
 * pvamd_composed_query_interp / _f64: as pvamd_composed_query / _f64 without flags; out_leaf (the arg-min leaf, what the backward
 *   needs) optional.  Every leaf BOUNDING_BOX, transforms rigid.
 * pvamd_cached_query_interp_backward / _f64, pvamd_composed_query_interp_backward / _f64: as pvamd_cached_query_backward /
 *   pvamd_composed_query_backward (same arguments, scratch sizes, fixed-order reductions) for the interpolated forward.       */
int pvamd_cached_query_interp(const pvamd_grid_t* grid, const float* points, int64_t P, float* out_val, float* out_grad,
                              uint8_t* out_oob, void* stream);
int pvamd_cached_query_interp_f64(const pvamd_grid_t* grid, const double* points, int64_t P, double* out_val, double* out_grad,
                                  uint8_t* out_oob, void* stream);
int pvamd_composed_query_interp(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points, int64_t P,
                                float* out_val, float* out_grad, int32_t* out_leaf, void* stream);
int pvamd_composed_query_interp_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* points,
                                    int64_t P, double* out_val, double* out_grad, int32_t* out_leaf, void* stream);
int pvamd_cached_query_interp_backward(const pvamd_grid_t* grid, const float* points, int64_t P, const float* dval,
                                       const float* dgrad, float* dpoints, void* stream);
int pvamd_cached_query_interp_backward_f64(const pvamd_grid_t* grid, const double* points, int64_t P, const double* dval,
                                           const double* dgrad, double* dpoints, void* stream);
int pvamd_composed_query_interp_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                         int64_t P, const int32_t* out_leaf, const float* dval, const float* dgrad, float* dpoints,
                                         float* dtf, void* scratch, void* stream);
int pvamd_composed_query_interp_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                             const double* points, int64_t P, const int32_t* out_leaf, const double* dval,
                                             const double* dgrad, double* dpoints, double* dtf, void* scratch, void* stream);


/* ---- Minimum over points (ComposedSDF.min_over_points / RobotSDF.min_over_points) ----
 * A composition of S leaves under A configurations (tf: device [S*A][4][4] leaf-major, rigid; every leaf BOUNDING_BOX) and P
 * points.  v_s(a, p), g_s(a, p): the value and gradient of leaf s alone at point p under transform (s, a) -- the bits of a
 * one-leaf composition ComposedSDF([sdfs[s]], slice s of the stack).  v(a, p), g(a, p): the composed answer (first minimum over
 * leaves, NaN counts as the minimum, the winner's gradient rotated back), the bits of the fused forwards.
 *  1. Order: NaN is below every number, -0.0 and +0.0 tie, ties go to the smallest point index.
 *  2. per_leaf = 0: one pair per configuration (Z = 1); out_index[a] = the smallest p minimising v(a, .); out_val[a] / out_grad[a]
 *     = v(a, p) / g(a, p) bit for bit (the composed choice of leaf at p included); out_leaf[a] = that leaf.
 *     per_leaf = 1: one pair per (a, s) (Z = S), stored [A][S]; out_index[a][s] = the smallest p minimising v_s(a, .); out_val /
 *     out_grad = v_s / g_s there; out_leaf[a][s] = s.
 *  3. mode: PVAMD_LEAF_NEAREST or PVAMD_LEAF_TRILINEAR, the leaf statements of pvamd_composed_query / _interp (float32) and
 *     pvamd_composed_query_f64 / _interp_f64 (float64).
 *  4. Bitwise reproducible whatever the launch geometry: per-chunk keys (order-preserving value bits, point index) reduced with
 *     an exact min, then the answer recomputed at the chosen point.  No device -> host synchronisation, no allocation.
 * pvamd_composed_min_over_points / _f64: out_val [A][Z], out_grad [A][Z][3], out_index [A][Z] int64, out_leaf [A][Z] int32 or
 *   NULL.  1 <= P <= 2^32 - 2.  scratch: device, PVAMD_MIN_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf) bytes, 16-byte aligned
 *   (one 16-byte key per pair and 4096-point chunk).
 * pvamd_composed_min_over_points_backward / _f64: the VJP of the pairs given the forward's out_index and out_leaf (required):
 *   torch autograd through the composed (per_leaf: one-leaf) query gathered at out_index, decisions held fixed; the per-pair
 *   statements of pvamd_composed_query_backward / _interp_backward.  dval [A][Z] / dgrad [A][Z][3] may be NULL.  dtf: device
 *   [S*A][4][4] or NULL, rows of unselected (leaf, configuration) pairs and row 3 zero.  dpoints: device [P][3] or NULL, rows
 *   no pair selected exactly zero, a row selected by several pairs summed in pair order.  S <= 64.  scratch (when dpoints is
 *   given): PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(S, A, per_leaf) bytes, 16-byte aligned.                                */
#define PVAMD_LEAF_NEAREST   0
#define PVAMD_LEAF_TRILINEAR 1
#define PVAMD_MOP_CHUNK 4096  /* points per partial key */
#define PVAMD_MIN_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf) \
    (16 * (int64_t)(A) * ((per_leaf) ? (int64_t)(S) : 1) * (((int64_t)(P) + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK))
#define PVAMD_MIN_OVER_POINTS_BACKWARD_SCRATCH_BYTES(S, A, per_leaf) (24 * (int64_t)(A) * ((per_leaf) ? (int64_t)(S) : 1))
int64_t pvamd_min_over_points_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t per_leaf);
int64_t pvamd_min_over_points_backward_scratch_bytes(int32_t S, int32_t A, int32_t per_leaf);
int pvamd_composed_min_over_points(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points, int64_t P,
                                   int32_t mode, int32_t per_leaf, float* out_val, float* out_grad, int64_t* out_index,
                                   int32_t* out_leaf, void* scratch, void* stream);
int pvamd_composed_min_over_points_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* points,
                                       int64_t P, int32_t mode, int32_t per_leaf, double* out_val, double* out_grad,
                                       int64_t* out_index, int32_t* out_leaf, void* scratch, void* stream);
int pvamd_composed_min_over_points_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                            int64_t P, int32_t mode, int32_t per_leaf, const int64_t* index, const int32_t* leaf,
                                            const float* dval, const float* dgrad, float* dpoints, float* dtf, void* scratch,
                                            void* stream);
int pvamd_composed_min_over_points_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                const double* points, int64_t P, int32_t mode, int32_t per_leaf,
                                                const int64_t* index, const int32_t* leaf, const double* dval, const double* dgrad,
                                                double* dpoints, double* dtf, void* scratch, void* stream);

/* ---- Leaf-pair distance (ComposedSDF.leaf_pair_distance / RobotSDF.self_collision_distance) ----
 * A composition of S leaves under A configurations (tf: device [S*A][4][4] leaf-major, rigid, in the query dtype; the float64
 * stack is the exact widening of the float32 one), K ordered pairs k = (s, t), s != t, and one point set per leaf, given in that
 * leaf's own frame and packed into one [npoints][3] array.  table: device int64 [K][4] = (s, t, offset of set t in the packed
 * points, P_t >= 1).
 *  1. Pair transform.  Ms = stack row (s, a), Mt = stack row (t, a).  For i, j < 3:
 *       C[i][j] = fma(Ms[i][2], Mt[j][2], fma(Ms[i][1], Mt[j][1], Ms[i][0] * Mt[j][0]))          (Rs Rt^T)
 *       C[i][3] = Ms[i][3] - fma(C[i][2], Mt[2][3], fma(C[i][1], Mt[1][3], C[i][0] * Mt[0][3]))  (ts - C_rot tt)
 *     row 3 = (0, 0, 0, 1).  C maps leaf t's frame to leaf s's frame.  Stored [K][A][4][4] (pair-major).
 *  2. out_val[a][k], out_index[a][k], out_grad[a][k] are bit for bit what pvamd_composed_min_over_points (per_leaf = 0) gives for
 *     the one-leaf composition (grids[s], stack C[k]) over the P_t points of set t: the same leaf statements, the same index
 *     rule (NaN is the minimum, -0.0 ties +0.0, the smallest index wins), the index into set t.  The gradient is leaf s's SDF
 *     gradient at the witness point rotated back by C: it is expressed in LEAF t's FRAME.
 *  3. Bitwise reproducible whatever the launch geometry; no device -> host synchronisation, no allocation, no float atomics.
 *     Extra memory: one 16-byte key per pair, configuration and 4096-point chunk when a set holds more than one chunk, else none.
 *  4. Backward: the VJP of item 2 w.r.t. the pair's transform (the single-pair statements of
 *     pvamd_composed_min_over_points_backward, decisions held fixed), then the VJP of item 1 to both stack rows, each row's
 *     gradient summed over the pairs that use it (as s or as t) in increasing k.  Points carry no gradient.  S <= 64.
 * pvamd_leaf_pair_transforms / _f64: out [K][A][4][4].  K = 0 does nothing.  A pair with a leaf out of range gives NaN rows.
 * pvamd_leaf_pair_distance / _f64: C = the pair transforms; out_val [A][K], out_grad [A][K][3], out_index [A][K] int64 (-1 and
 *   NaN for a malformed table row).  max_points = the largest P_t of the table (1 <= max_points <= 2^32 - 2).  scratch: device,
 *   PVAMD_LEAF_PAIR_SCRATCH_BYTES(K, A, max_points, sizeof(T), 0) bytes, 16-byte aligned (NULL when that is 0).
 * pvamd_leaf_pair_distance_backward / _f64: given the forward's out_index, dval [A][K] and dgrad [A][K][3] (either may be NULL),
 *   writes dtf [S*A][4][4] (every row; rows no pair uses and row 3 zero).  scratch: PVAMD_LEAF_PAIR_SCRATCH_BYTES(K, A,
 *   max_points, sizeof(T), 1) bytes, 16-byte aligned (24 values per pair and configuration: dMs and dMt).                         */
#define PVAMD_LEAF_PAIR_SCRATCH_BYTES(K, A, max_points, elem, backward)                                           \
    ((backward) ? 24 * (int64_t)(K) * (int64_t)(A) * (int64_t)(elem)                                             \
                : ((((int64_t)(max_points) + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK) > 1                          \
                       ? 16 * (int64_t)(K) * (int64_t)(A) * (((int64_t)(max_points) + PVAMD_MOP_CHUNK - 1) / PVAMD_MOP_CHUNK) \
                       : 0))
int64_t pvamd_leaf_pair_scratch_bytes(int32_t K, int32_t A, int64_t max_points, int32_t is_f64, int32_t backward);
int pvamd_leaf_pair_transforms(const float* tf, int32_t S, int32_t A, const int64_t* table, int32_t K, float* out, void* stream);
int pvamd_leaf_pair_transforms_f64(const double* tf, int32_t S, int32_t A, const int64_t* table, int32_t K, double* out,
                                   void* stream);
int pvamd_leaf_pair_distance(const pvamd_grid_t* grids, int32_t S, const float* C, int32_t A, const float* points, int64_t npoints,
                             const int64_t* table, int32_t K, int64_t max_points, int32_t mode, float* out_val, float* out_grad,
                             int64_t* out_index, void* scratch, void* stream);
int pvamd_leaf_pair_distance_f64(const pvamd_grid_t* grids, int32_t S, const double* C, int32_t A, const double* points,
                                 int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode, double* out_val,
                                 double* out_grad, int64_t* out_index, void* scratch, void* stream);
int pvamd_leaf_pair_distance_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, const float* C, int32_t A,
                                      const float* points, int64_t npoints, const int64_t* table, int32_t K, int32_t mode,
                                      const int64_t* index, const float* dval, const float* dgrad, float* dtf, void* scratch,
                                      void* stream);
int pvamd_leaf_pair_distance_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, const double* C, int32_t A,
                                          const double* points, int64_t npoints, const int64_t* table, int32_t K, int32_t mode,
                                          const int64_t* index, const double* dval, const double* dgrad, double* dtf,
                                          void* scratch, void* stream);

/* ---- Hinge penalty over points (ComposedSDF.hinge_over_points / RobotSDF.hinge_over_points) ----
 * The compositions, pairs and per-leaf values of "Minimum over points": v(a, p) the composed value (per_leaf = 0, Z = 1) or
 * v_s(a, p) the one-leaf composition's (per_leaf = 1, Z = S, pairs stored [A][S]), the bits of the fused forwards.
 *  1. margin m is given in the query dtype (a Python margin is rounded once to it, torch's rule for a scalar against a tensor).
 *  2. Each term is rounded in the query dtype as torch rounds (m - v).clamp(min=0) ** power: h = max(m - v, 0) (NaN stays
 *     NaN), then h (power 1) or h * h (power 2).
 *  3. out_val[pair] = the sum over p of the terms, in float64, in an order that depends only on (S, A, P) (per lane in point
 *     order, a wave butterfly, the four waves in order, then the 4096-point chunks in chunk order), rounded once to the query
 *     dtype: for float32 within 1 ulp of float32(fsum(terms)); for float64 an error of at most P 2^-53 sum(terms).  A NaN v
 *     makes its pair's value NaN.  Bitwise reproducible; no device -> host synchronisation, no allocation.
 *  4. out_count[pair] = the number of p with v < m (int64); a NaN is not counted.
 *  5. power: 1 or 2, else PVAMD_E_MODE.  mode: PVAMD_LEAF_NEAREST or PVAMD_LEAF_TRILINEAR.  1 <= P.
 * pvamd_composed_hinge_over_points / _f64: out_val [A][Z], out_count [A][Z] int64.  scratch: device,
 *   PVAMD_HINGE_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf) bytes, 16-byte aligned (a 16-byte (sum, count) per pair and chunk).
 * pvamd_composed_hinge_over_points_backward / _f64: the VJP given up [A][Z] (the upstream of out_val): torch autograd through
 *   ((m - v).clamp(min=0) ** power).sum(-1), decisions held fixed, bit for bit.  Per pair the composed value and winning leaf
 *   are recomputed with the forward's statements and dv = -(up (2 h)) (power 2) or -up (power 1) where m - v >= 0, else -0
 *   (clamp's mask passes v == m; a NaN v gets a zero upstream); then the per-pair statements and fixed-order sums of
 *   pvamd_composed_query_backward / _interp_backward with a value upstream only (a nearest leaf in range has no derivative).
 *   per_leaf = 1: one pass per leaf s as the one-leaf composition (its dtf rows exactly that composition's), dpoints summed
 *   over the leaves in leaf order.  No stored leaf ids, no (A, P) upstream.  dtf: device [S*A][4][4] or NULL (row 3 zero);
 *   dpoints: device [P][3] or NULL.  S <= 64.  scratch: pvamd_hinge_over_points_backward_scratch_bytes(S, A, P, per_leaf,
 *   is_f64) bytes, 16-byte aligned.  That function is the definition (the composed backward's launch plan decides the size:
 *   call it, as for pvamd_composed_backward_scratch_bytes); there is no macro.                                                 */
#define PVAMD_HINGE_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf) PVAMD_MIN_OVER_POINTS_SCRATCH_BYTES(S, A, P, per_leaf)
int64_t pvamd_hinge_over_points_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t per_leaf);
int64_t pvamd_hinge_over_points_backward_scratch_bytes(int32_t S, int32_t A, int64_t P, int32_t per_leaf, int32_t is_f64);
int pvamd_composed_hinge_over_points(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                     int64_t P, int32_t mode, int32_t per_leaf, float margin, int32_t power, float* out_val,
                                     int64_t* out_count, void* scratch, void* stream);
int pvamd_composed_hinge_over_points_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* points,
                                         int64_t P, int32_t mode, int32_t per_leaf, double margin, int32_t power, double* out_val,
                                         int64_t* out_count, void* scratch, void* stream);
int pvamd_composed_hinge_over_points_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* points,
                                              int64_t P, int32_t mode, int32_t per_leaf, float margin, int32_t power,
                                              const float* up, float* dpoints, float* dtf, void* scratch, void* stream);
int pvamd_composed_hinge_over_points_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A,
                                                  const double* points, int64_t P, int32_t mode, int32_t per_leaf, double margin,
                                                  int32_t power, const double* up, double* dpoints, double* dtf, void* scratch,
                                                  void* stream);

/* ---- Leaf-pair hinge (ComposedSDF.leaf_pair_hinge / RobotSDF.self_collision_hinge) ----
 * The compositions, pairs, point sets, table and pair transforms C of "Leaf-pair distance"; m and power as in "Hinge penalty
 * over points".
 *  1. out_val[a][k], out_count[a][k] are bit for bit what pvamd_composed_hinge_over_points (per_leaf = 0) gives for the
 *     one-leaf composition (grids[s], stack C[k]) over the P_t points of set t: each term rounded as torch rounds
 *     (m - v).clamp(min=0) ** power, the float64 sum in that call's order (per lane in point order, the wave butterfly, the
 *     four waves in order, the 4096-point chunks of set t in chunk order), rounded once; a NaN v makes the value NaN and is not
 *     counted.  A malformed table row gives NaN and 0.
 *  2. Bitwise reproducible whatever the launch geometry; no device -> host synchronisation, no allocation, no float atomics.
 *     Extra memory: one 16-byte (sum, count) per pair, configuration and 4096-point chunk when a set holds more than one chunk,
 *     else none.
 *  3. Backward: per (a, k) the VJP of item 1 w.r.t. C[k][a], the bits pvamd_composed_hinge_over_points_backward gives for the
 *     one-leaf composition's dtf (the same decisions and dv rule, the per-wave slots, the four waves in order, the 1024-point
 *     chunks in chunk order), given up [A][K]; then the VJP of "Leaf-pair distance" item 1 to both stack rows, each row summed
 *     over the pairs that use it in increasing k.  Points carry no gradient; a nearest leaf in range has no derivative.  S <= 64.
 * pvamd_leaf_pair_hinge / _f64: out_val [A][K], out_count [A][K] int64.  max_points = the largest P_t of the table
 *   (1 <= max_points <= 2^32 - 2).  scratch: device, pvamd_leaf_pair_hinge_scratch_bytes(K, A, max_points, is_f64, 0) bytes,
 *   16-byte aligned (NULL when that is 0).
 * pvamd_leaf_pair_hinge_backward / _f64: given up [A][K], writes dtf [S*A][4][4] (every row; rows no pair uses and row 3 zero).
 *   scratch: pvamd_leaf_pair_hinge_scratch_bytes(K, A, max_points, is_f64, 1) bytes, 16-byte aligned (the dC slab of
 *   12 values per pair, configuration and 1024-point chunk, then 24 values per pair and configuration: dMs and dMt).
 * pvamd_leaf_pair_hinge_scratch_bytes is the definition of both sizes: call it; there is no macro.                             */
int64_t pvamd_leaf_pair_hinge_scratch_bytes(int32_t K, int32_t A, int64_t max_points, int32_t is_f64, int32_t backward);
int pvamd_leaf_pair_hinge(const pvamd_grid_t* grids, int32_t S, const float* C, int32_t A, const float* points, int64_t npoints,
                          const int64_t* table, int32_t K, int64_t max_points, int32_t mode, float margin, int32_t power,
                          float* out_val, int64_t* out_count, void* scratch, void* stream);
int pvamd_leaf_pair_hinge_f64(const pvamd_grid_t* grids, int32_t S, const double* C, int32_t A, const double* points,
                              int64_t npoints, const int64_t* table, int32_t K, int64_t max_points, int32_t mode, double margin,
                              int32_t power, double* out_val, int64_t* out_count, void* scratch, void* stream);
int pvamd_leaf_pair_hinge_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, const float* C, int32_t A,
                                   const float* points, int64_t npoints, const int64_t* table, int32_t K, int64_t max_points,
                                   int32_t mode, float margin, int32_t power, const float* up, float* dtf, void* scratch,
                                   void* stream);
int pvamd_leaf_pair_hinge_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, const double* C, int32_t A,
                                       const double* points, int64_t npoints, const int64_t* table, int32_t K, int64_t max_points,
                                       int32_t mode, double margin, int32_t power, const double* up, double* dtf, void* scratch,
                                       void* stream);

/* ---- Chamfer normal equations (chamfer_normal_equations / refine_poses) ----
 * The Gauss-Newton normal equations of the chamfer cost sum_i (sdf(W[b] p_i))^2 of B poses against one cached grid, and the
 * Levenberg-Marquardt step built on them.  grid: 3-D, BOUNDING_BOX (else PVAMD_E_MODE), either index arithmetic (index_f64).
 *  1. Per pair (b, i): x = W[b] p_i with the bits of pvamd_transform_points (affine_row).  (v, n) = the bits of
 *     pvamd_cached_query (mode PVAMD_LEAF_NEAREST) or pvamd_cached_query_interp (PVAMD_LEAF_TRILINEAR) at x: value and returned
 *     gradient, in range or in the bounding-box branch.  The trilinear n is the interpolated stored gradient, not d val / dx:
 *     the point-to-plane linearisation is the same statement in both modes.
 *  2. The pose perturbation is a left-multiplied twist in the object frame, xi = (u, w), translation first: x' = x + w cross x
 *     + u, so j = (n, x cross n).  j is formed in float64 from the float32 x and n: each product of the cross product is exact
 *     in float64 and each component rounds once.
 *  3. out_sums[b] = (s0, s1[6], s2 upper triangle row-major [21]): s0 = sum v v, s1 = sum v j, s2 = sum j j^T, in float64, each
 *     term entering by one fused multiply-add, in an order that depends only on (B, N): per lane in point order over its points
 *     of a PVAMD_REG_CHUNK-point chunk, a wave butterfly, the four waves in order, then the chunks in chunk order.  Bitwise
 *     reproducible; no float atomics, no device -> host synchronisation, no allocation.  A NaN v or n makes that pose's sums
 *     NaN and only that pose's.
 *  4. out_counts[b] = the number of points of pose b that pass the range decision of the query (int64).
 *  5. The caller scales: cost = scale^2 s0 / N, gradient = scale^2 s1 / N (half of d cost / d xi at xi = 0 under this
 *     linearisation), hessian = scale^2 s2 / N.
 * pvamd_chamfer_normal_eq: W device [B][4][4], points device [N][3], 1 <= N, 0 <= B (B = 0 does nothing).  scratch: device,
 *   PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES(B, N) bytes, 8-byte aligned (28 sums and one count per pose and chunk).
 * pvamd_pose_lm_step: one Levenberg-Marquardt decision per pose on the device, all float64.  sums [B][28]: the raw sums just
 *   computed at Wtry.  State: Wacc, Wtry [B][3][4], sums_acc [B][28], lambda [B], accepted [B] int32 (the caller zeroes it and
 *   sets Wtry and lambda before the first call).
 *   a. Accept if first or s0(sums) < s0(sums_acc) (strict: a NaN never accepts): Wacc = Wtry, sums_acc = sums,
 *      lambda = max(lambda down, lambda_min), accepted += 1.  Otherwise lambda = min(lambda up, lambda_max).
 *   b. Solve (S2 + lambda D) xi = -S1 with the accepted sums by Cholesky without pivoting in a fixed order, D diagonal with
 *      D_k = S2_kk where that is positive and 1 elsewhere (an axis no point observes gets a zero step).  A pivot that is not
 *      positive and finite, or a non-finite xi: xi = 0 and lambda = min(lambda up, lambda_max).
 *   c. Retract: Wtry = [Exp(w) R, Exp(w) t + u] from Wacc = [R, t], Exp by Rodrigues' formula (the series below |w| < 1e-8);
 *      xi = 0 copies Wacc bit for bit.  W_next [B][4][4] = Wtry rounded to float32 with the row 0 0 0 1: what the next
 *      pvamd_chamfer_normal_eq reads.
 *   1 < up, 0 < down <= 1, 0 < lambda_min <= lambda_max < inf, first 0 or 1, else PVAMD_E_MODE.                                   */
#define PVAMD_REG_CHUNK 2048 /* points per slab row */
#define PVAMD_REG_SUMS 28    /* s0, s1[6], s2 upper triangle [21] */
#define PVAMD_CHAMFER_NORMAL_EQ_SCRATCH_BYTES(B, N) \
    (8 * (PVAMD_REG_SUMS + 1) * (int64_t)(B) * (((int64_t)(N) + PVAMD_REG_CHUNK - 1) / PVAMD_REG_CHUNK))
int64_t pvamd_chamfer_normal_eq_scratch_bytes(int32_t B, int64_t N);
int pvamd_chamfer_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points, int64_t N,
                            double* out_sums, int64_t* out_counts, void* scratch, void* stream);
int pvamd_pose_lm_step(int32_t B, const double* sums, int32_t first, double* Wacc, double* sums_acc, double* lambda,
                       int32_t* accepted, double* Wtry, float* W_next, double up, double down, double lambda_min,
                       double lambda_max, void* stream);

/* ---- Semantic normal equations (semantic_normal_equations / refine_poses with semantics, targets or huber_delta) ----
 * "Chamfer normal equations" with a kind and a target distance per point and Huber weights: the cost of a pose that must keep
 * known-free points outside the object, known-occupied points inside it and surface points on it, robust against outliers.
 * Steps 1, 2 and 5 of that section hold as they stand (x, (v, n), j, the caller's scaling; N is every point, ignored ones
 * included); the grid and mode arguments are its.  Per pair (b, i), all in float64:
 *  1. kind_i = kinds[i] (uint8; PVAMD_POINT_*; any value >= PVAMD_POINT_IGNORE is IGNORE; kinds NULL: every point is SURFACE).
 *     s_i = targets[i] (float32; targets NULL: 0).  r = (double)v - (double)s_i, rounded once.
 *  2. The pair is inactive when kind_i is IGNORE, when it is FREE and r >= 0, or when it is OCCUPIED and r <= 0.  An inactive pair
 *     adds nothing: its terms are skipped, not added as zeros, so a NaN n there reaches no sum.  A NaN r of a SURFACE, FREE or
 *     OCCUPIED point fails both comparisons: the pair is active and makes its pose's sums NaN.  Accumulators start at +0.0.
 *  3. An active pair, a = |r|, delta = huber_delta (> 0; +inf: no pair is an outlier):
 *     inlier (not a > delta): s0 = fma(r, r, s0); s1_k = fma(r, j_k, s1_k); s2_rc = fma(j_r, j_c, s2_rc) -- the statements of
 *       "Chamfer normal equations" with r for v.
 *     outlier (a > delta): w = delta / a; s0 = fma(delta, (a + a) - delta, s0); q = w r, s1_k = fma(q, j_k, s1_k); u_r = w j_r,
 *       s2_rc = fma(u_r, j_c, s2_rc).  Each named product and quotient rounds once.  This is iteratively reweighted least
 *       squares with the Huber function rho: s0 = sum rho, s1 = sum w r j, s2 = sum w j j^T (rho = r^2 inside delta).
 *  4. The order of summation is pvamd_chamfer_normal_eq's: per lane in point order over its points of a PVAMD_REG_CHUNK-point
 *     chunk, a wave butterfly, the four waves in order, the chunks in chunk order.  With kinds NULL or all 0, targets NULL or all
 *     0 and huber_delta = +inf the 28 sums are those of pvamd_chamfer_normal_eq bit for bit.
 *  5. out_counts[b][PVAMD_SEM_COUNTS] (int64): the points that pass the range decision of the query (every point, whatever its
 *     kind: out_counts of pvamd_chamfer_normal_eq); the active pairs of kind SURFACE; of kind FREE; of kind OCCUPIED; the active
 *     pairs that took the outlier branch.
 * Bitwise reproducible; no float atomics, no allocation, no device -> host synchronisation; a NaN touches its own pose only.
 * pvamd_semantic_normal_eq: the argument checks of pvamd_chamfer_normal_eq, and huber_delta NaN or <= 0 is PVAMD_E_MODE; all
 *   before any launch.  kinds device [N] or NULL, targets device [N] (4-byte aligned) or NULL.  out_sums device [B][28].
 *   scratch: device, pvamd_semantic_normal_eq_scratch_bytes(B, N) bytes, 8-byte aligned (28 sums and 5 counts per pose and
 *   chunk); the exported function is the definition of the size.  The sums feed pvamd_pose_lm_step as they are: it accepts on
 *   s0 alone.                                                                                                                    */
#define PVAMD_POINT_SURFACE  0 /* penalised on either side: r^2 */
#define PVAMD_POINT_FREE     1 /* penalised where r < 0 */
#define PVAMD_POINT_OCCUPIED 2 /* penalised where r > 0 */
#define PVAMD_POINT_IGNORE   3 /* never penalised; so is every larger value */
#define PVAMD_SEM_COUNTS 5     /* in range, active SURFACE, active FREE, active OCCUPIED, outliers */
int64_t pvamd_semantic_normal_eq_scratch_bytes(int32_t B, int64_t N);
int pvamd_semantic_normal_eq(const pvamd_grid_t* grid, int32_t mode, const float* W, int32_t B, const float* points, int64_t N,
                             const uint8_t* kinds, const float* targets, double huber_delta, double* out_sums,
                             int64_t* out_counts, void* scratch, void* stream);

/* ---- Joint-space normal equations (joint_normal_equations / refine_joint_configuration) ----
 * "Semantic normal equations" for a robot: the Gauss-Newton normal equations of scale^2 / N sum_i rho(r_i) over the joint values
 * q of A configurations of a composition of S leaves ("Minimum over points": grids device [S], stack device [S*A][4][4]
 * leaf-major, the float32 stack pvamd_configure_chain gives; every grid 3-D, BOUNDING_BOX, either index arithmetic), and the
 * Levenberg-Marquardt step built on them.  Every point is won by exactly one leaf and a link's twist Jacobian does not depend on
 * the point, so the joint-space equations factor exactly over the leaves.
 *  1. Per pair (a, i) the winning leaf s and, in its frame, x = T_s p_i with T_s = stack[s*A + a], (v, n) are those of the fused
 *     composed forwards (mop_point): the first minimum over the leaves in leaf order, a NaN counting as the minimum; n is the
 *     leaf's own returned gradient, before it is rotated back into the object frame.
 *  2. r = v - target; activity, the Huber branch and j = (n, x cross n) in float64 are the statements of "Semantic normal
 *     equations", unchanged.  The pair's 28 terms go to the sums of leaf s and to no other leaf.
 *  3. The order of summation is pvamd_semantic_normal_eq's: lane t of chunk c takes points c PVAMD_REG_CHUNK + k 256 + t in k
 *     order, a wave butterfly, the four waves in order, then the chunks in chunk order.  A point a leaf does not win is skipped for
 *     that leaf; a wave without a point of a leaf adds +0.0 for it.  So leaf_sums[a][s][28] and leaf_counts[a][s][5] are, bit for
 *     bit, what pvamd_semantic_normal_eq returns for the pose T_s and the grid of leaf s when the caller's kinds are replaced by
 *     PVAMD_POINT_IGNORE wherever s does not win -- except leaf_counts[a][s][0], which counts the in-range points s wins.
 *  4. J[a][s] (6 x M, float64, row-major) carries a joint step into a twist of leaf s's frame.  The records of leaf s's frame and
 *     its ancestors are walked root first in float64 from the float32 joint values, origins and axes (sin and cos in float64):
 *     world = world @ origin @ motion, the statements of pvamd_chain_fk.  T_s = offset_inv[s] @ rigid_inverse(world of the leaf's
 *     frame), in float64.  For a moving joint k on the way, with a = R(world_k) axis_k and o = t(world_k) in the object frame,
 *     xi_W = (u_W, w_W) = (o cross a, a) for a revolute or continuous joint and (a, 0) for a prismatic one (translation first),
 *     and with (R, t) = T_s:  J[:, k] = -(R u_W + t cross (R w_W), R w_W).  Every other column is zero.
 *  5. Assembly, float64, fused multiply-adds, leaves in order s = 0 .. S-1 from +0.0:  cost = sum_s c_s;
 *     g_k = fma(J_s[r][k], g6_s[r], g_k) for r = 0 .. 5;  H_ij (i <= j) = fma(J_s[r][i], v_r, H_ij) for r = 0 .. 5 with
 *     v_r = (H6_s J_s)[r][j] = fma(H6_s[r][c], J_s[c][j], v_r) for c = 0 .. 5 from +0.0.  Only the upper triangle is formed: the
 *     caller mirrors it, so H is exactly symmetric.  sums[a] = (cost, g[M], H upper triangle row-major [M (M + 1) / 2]).
 *     counts[a][PVAMD_SEM_COUNTS + S] (int64): the five leaf counts summed over s, then per leaf the active pairs it won.
 *  6. The caller scales by scale^2 / N, N every point, as in "Semantic normal equations".  A NaN sum of a leaf makes every
 *     entry of its configuration NaN and touches no other configuration.
 * Bitwise reproducible; no float atomics, no allocation, no device -> host synchronisation.
 * pvamd_joint_normal_eq: 1 <= S <= PVAMD_JOINT_MAX_LEAVES, 1 <= N, 0 <= A (A = 0 does nothing); mode PVAMD_LEAF_*; huber_delta NaN
 *   or <= 0 is PVAMD_E_MODE.  kinds device [N] or NULL, targets device [N] or NULL.  scratch: device,
 *   pvamd_joint_normal_eq_scratch_bytes(A, S, N) bytes, 8-byte aligned: 28 sums and 5 counts per configuration, leaf and chunk
 *   (264 A S ceil(N / PVAMD_REG_CHUNK) bytes); the exported function is the definition of the size.
 * pvamd_chain_twists: joints device [F], q device [A][M], offset_inv device [S][4][4] (the arguments of pvamd_configure_chain),
 *   0 <= M <= PVAMD_JOINT_MAX.  J device [A][S][6][M].
 * pvamd_joint_assemble: sums device [A][1 + M + M (M + 1) / 2], counts device [A][PVAMD_SEM_COUNTS + S].
 * pvamd_joint_lm_step: pvamd_pose_lm_step in joint space, one decision per configuration.  sums: the row just assembled at q_try.
 *   State: q_acc, q_try [A][M] float64, sums_acc (a row of sums each), lambda [A], accepted [A] int32 (the caller zeroes it and
 *   sets q_try and lambda before the first call).
 *   a. Accept if first or cost(sums) < cost(sums_acc) (strict: a NaN never accepts): q_acc = q_try, sums_acc = sums,
 *      lambda = max(lambda down, lambda_min), accepted += 1.  Otherwise lambda = min(lambda up, lambda_max).
 *   b. Solve (H + lambda D) dq = -g with the accepted sums by Cholesky without pivoting in pvamd_pose_lm_step's loop order, D
 *      diagonal with D_k = H_kk where that is positive and 1 elsewhere (a joint no point observes gets a zero step).  A pivot that
 *      is not positive and finite, or a non-finite dq: dq = 0 and lambda = min(lambda up, lambda_max).
 *   c. q_try = q_acc + dq in float64, then clamped into limits[k] = (lo, hi) (device [M][2] float64, or NULL: no clamp); dq = 0
 *      copies q_acc bit for bit.  q_next [A][M] = q_try rounded to float32: what the next evaluation reads.
 *   The checks of up, down, lambda_min, lambda_max and first are pvamd_pose_lm_step's.                                            */
#define PVAMD_JOINT_MAX 32        /* the most joint values M */
#define PVAMD_JOINT_MAX_LEAVES 64 /* the most leaves S */
int64_t pvamd_joint_normal_eq_scratch_bytes(int32_t A, int32_t S, int64_t N);
int pvamd_joint_normal_eq(const pvamd_grid_t* grids, int32_t S, int32_t mode, const float* stack, int32_t A, const float* points,
                          int64_t N, const uint8_t* kinds, const float* targets, double huber_delta, double* leaf_sums,
                          int64_t* leaf_counts, void* scratch, void* stream);
int pvamd_chain_twists(const pvamd_joint_t* joints, int32_t F, const float* q, int32_t A, int32_t M, const float* offset_inv,
                       int32_t S, double* J, void* stream);
int pvamd_joint_assemble(const double* leaf_sums, const int64_t* leaf_counts, const double* J, int32_t A, int32_t S, int32_t M,
                         double* sums, int64_t* counts, void* stream);
int pvamd_joint_lm_step(int32_t A, int32_t M, const double* sums, int32_t first, double* q_acc, double* sums_acc, double* lambda,
                        int32_t* accepted, double* q_try, float* q_next, const double* limits, double up, double down,
                        double lambda_min, double lambda_max, void* stream);

/* ---- Ray casting (CachedSDF.ray_cast / ComposedSDF.ray_cast / RobotSDF.ray_cast) ----
 * Sphere tracing: where the ray o + t d first meets the surface of one cached grid (3-D, BOUNDING_BOX, else PVAMD_E_MODE; either
 * index arithmetic) or of a composition ("Minimum over points": S leaves, A configurations, tf device [S*A][4][4] leaf-major,
 * rigid; the rays are given in the object frame and shared by the configurations).  sdf(p) = (v, g): the bits of
 * pvamd_cached_query / _interp / _f64 / _interp_f64 (one grid) or of the fused composed forwards (a composition) at p, chosen by
 * mode (PVAMD_LEAF_NEAREST / PVAMD_LEAF_TRILINEAR) and the element type T of the entry point.
 *  1. Scalars, all in T: t_min and t_max not NaN (t_max = +inf allowed), eps finite and >= 0, step_scale finite and > 0, else
 *     PVAMD_E_MODE; 1 <= max_steps <= 65535, else PVAMD_E_SHAPE.
 *  2. Per ray, every product and sum rounded separately in T (no fused multiply-add): what an elementwise o + t * d gives.
 *         t = t_min; steps = 0; status = MAX_STEPS; v = NaN; g = (NaN, NaN, NaN)
 *         if not (t <= t_max): status = MISS
 *         else repeat max_steps times:
 *             p_j = o_j + t * d_j   (j = 0..2)
 *             (v, g) = sdf(p); steps += 1
 *             if v != v:  status = INVALID; stop
 *             if v <= eps: status = HIT; stop
 *             tn = t + step_scale * v
 *             if not (tn <= t_max): status = MISS; stop
 *             t = tn
 *  3. Outputs per ray: out_t = the t of the last evaluated p (t_min when none was; for MAX_STEPS the t of evaluation max_steps,
 *     not the tn after it), so o + out_t d is where out_val / out_grad were read; out_status uint8 (PVAMD_RAY_*); out_val /
 *     out_grad the last (v, g); out_steps int32.
 *  4. Directions are the caller's: meant to be unit length, any other length scales the step.  A NaN in o or d ends as INVALID
 *     or MISS by the rules above; the loop is bounded by max_steps whatever the input.
 *  5. Nearest-mode values are piecewise constant (one voxel-centre sample per voxel), so a nearest grid can overshoot the
 *     surface by up to half a voxel diagonal; PVAMD_LEAF_TRILINEAR or step_scale < 1 is the remedy.
 * One lane per (configuration, ray), rays in caller order; a wave leaves the step loop when all its rays have stopped.  Raw device
 * pointers, stream-ordered, no allocation, no scratch, no device -> host synchronisation, no atomics: capturable in a graph.
 * Argument errors return before any launch.
 * pvamd_cached_ray_cast / _f64: origins, directions device [R][3]; out_t, out_val, out_steps [R], out_status [R] uint8, out_grad
 *   [R][3].  0 <= R (R = 0 does nothing).
 * pvamd_composed_ray_cast / _f64: the outputs are [A][R] ([A][R][3]): row a is the loop above under configuration a alone.
 *   1 <= S, 0 <= A, 0 <= R (A = 0 or R = 0 does nothing).                                                                          */
#define PVAMD_RAY_MISS      0  /* left [t_min, t_max] (or t_min > t_max) without a hit */
#define PVAMD_RAY_HIT       1  /* v <= eps at out_t                                    */
#define PVAMD_RAY_MAX_STEPS 2  /* max_steps evaluations without a decision             */
#define PVAMD_RAY_INVALID   3  /* the query returned NaN at out_t                      */
int pvamd_cached_ray_cast(const pvamd_grid_t* grid, int32_t mode, const float* origins, const float* directions, int64_t R,
                          float t_min, float t_max, float eps, float step_scale, int32_t max_steps, float* out_t,
                          uint8_t* out_status, float* out_val, float* out_grad, int32_t* out_steps, void* stream);
int pvamd_cached_ray_cast_f64(const pvamd_grid_t* grid, int32_t mode, const double* origins, const double* directions, int64_t R,
                              double t_min, double t_max, double eps, double step_scale, int32_t max_steps, double* out_t,
                              uint8_t* out_status, double* out_val, double* out_grad, int32_t* out_steps, void* stream);
int pvamd_composed_ray_cast(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* origins,
                            const float* directions, int64_t R, int32_t mode, float t_min, float t_max, float eps,
                            float step_scale, int32_t max_steps, float* out_t, uint8_t* out_status, float* out_val, float* out_grad,
                            int32_t* out_steps, void* stream);
int pvamd_composed_ray_cast_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* origins,
                                const double* directions, int64_t R, int32_t mode, double t_min, double t_max, double eps,
                                double step_scale, int32_t max_steps, double* out_t, uint8_t* out_status, double* out_val,
                                double* out_grad, int32_t* out_steps, void* stream);

/* ---- Ray casting: gradient of the hit distance (ray_cast(..., differentiable=True)) ----
 * The derivative of out_t of "Ray casting" w.r.t. the origins, the directions and, for a composition, the transforms, under the
 * surface-normal linearisation at the hit point -- the model "Chamfer normal equations" takes: the gradient a cache record
 * stores is the first-order model of the surface.  It is NOT the derivative of the step loop: that would need every step's
 * state and is zero at every in-range point of a nearest grid.  Decisions are held fixed: status, step count, winning leaf.
 *  1. Per (configuration a, ray i): t = out_t, x = o_i + t d_i, n = out_grad (the gradient the forward returned at x).  The model
 *     is val(x + delta) = v + n . delta, and t is the root of val(o + t d) = const.
 *  2. Every term is formed in float64 from the T inputs, every product and sum rounded separately, left to right.
 *     c = n0 d0 + n1 d1 + n2 d2.  The pair contributes only when status == PVAMD_RAY_HIT, c < 0 and c is finite; a miss, a
 *     max-steps ray, an invalid ray and a hit whose normal does not face the ray (c >= 0: a ray that starts inside and points
 *     outward) contribute exactly zero to every output.  With w = -up[a][i] / c (up: the upstream of out_t):
 *         dorigins_i    += w n
 *         ddirections_i += (w t) n
 *     A grazing hit (c -> 0-) gives a large gradient by construction; weighting it is the caller's job.
 *  3. A composition: s the winning leaf at x, M = tf[s*A + a] (rigid), gamma_r = M[r][0] n0 + M[r][1] n1 + M[r][2] n2 (the
 *     leaf-frame record gradient: the forward returned n = L^T gamma), x_j = o_j + t d_j in float64:
 *         dtf[s*A + a][r][j] += (w gamma_r) x_j   (j < 3)
 *         dtf[s*A + a][r][3] += w gamma_r
 *     Row 3 of every dtf matrix is zero and leaves that win nowhere get exactly zero rows.  (v, n, s) are recomputed at the
 *     forward's own p (o + t d rounded in T as in "Ray casting" 2) with the forward's statements: the forward's bits, so no leaf
 *     ids are stored.
 *  4. Sums: dorigins / ddirections [R][3] sum over the configurations, dtf [S*A][4][4] over the rays, in float64, in an order
 *     that depends only on (S, A, R), each rounded once to T.  dorigins / ddirections: in configuration order within a split of
 *     aper consecutive configurations, then the splits in split order, where with nchunks = ceil(R / PVAMD_RAY_BACKWARD_CHUNK)
 *     and want = min(A, ceil(2048 / nchunks)): aper = ceil(A / want).  dtf: a wave butterfly over 64 consecutive rays, the four
 *     waves of a PVAMD_RAY_BACKWARD_CHUNK-ray chunk in wave order, then the chunks in chunk order.  No float atomics: two calls
 *     give the same bits.  No device -> host synchronisation, no allocation: capturable in a graph.
 * Argument errors return before any launch.  Any of dorigins, ddirections, dtf may be NULL (not wanted).
 * pvamd_cached_ray_cast_backward / _f64: one grid; elementwise, no lookup, no scratch.  directions, grad (the forward's out_grad)
 *   [R][3]; t, status, up [R]; dorigins, ddirections [R][3].  The origins do not enter: x appears in no term.  0 <= R.
 * pvamd_composed_ray_cast_backward / _f64: t, status, up [A][R]; dtf [S*A][4][4].  1 <= S <= 64, 0 <= A, 0 <= R (A = 0 or R = 0
 *   writes zeros).  scratch: device, pvamd_ray_cast_backward_scratch_bytes(S, A, R, is_f64) bytes, 16-byte aligned: 12 float64
 *   per (chunk, leaf, configuration), then 6 float64 per (split, ray) when there is more than one split.  That function is the
 *   definition (the launch plan decides the size; the partials are float64 for either T); there is no macro.                    */
#define PVAMD_RAY_BACKWARD_CHUNK 256 /* rays per slab row */
int64_t pvamd_ray_cast_backward_scratch_bytes(int32_t S, int32_t A, int64_t R, int32_t is_f64);
int pvamd_cached_ray_cast_backward(const float* directions, int64_t R, const float* t, const uint8_t* status, const float* grad,
                                   const float* up, float* dorigins, float* ddirections, void* stream);
int pvamd_cached_ray_cast_backward_f64(const double* directions, int64_t R, const double* t, const uint8_t* status,
                                       const double* grad, const double* up, double* dorigins, double* ddirections, void* stream);
int pvamd_composed_ray_cast_backward(const pvamd_grid_t* grids, int32_t S, const float* tf, int32_t A, const float* origins,
                                     const float* directions, int64_t R, int32_t mode, const float* t, const uint8_t* status,
                                     const float* up, float* dorigins, float* ddirections, float* dtf, void* scratch, void* stream);
int pvamd_composed_ray_cast_backward_f64(const pvamd_grid_t* grids, int32_t S, const double* tf, int32_t A, const double* origins,
                                         const double* directions, int64_t R, int32_t mode, const double* t, const uint8_t* status,
                                         const double* up, double* dorigins, double* ddirections, double* dtf, void* scratch,
                                         void* stream);

/* ---- Volume lattices ----
 * The five sections below work on a 3-D lattice of nx * ny * nz voxels in C order (x slowest, z fastest): voxel (x, y, z) has the
 * flat index (x * ny + y) * nz + z, and a record is [4] float32 (val, gx, gy, gz).  No axis is longer than
 * PVAMD_LATTICE_MAX_AXIS: a coordinate takes 11 bits in the states the line passes hand on.  Each section states its own
 * shortest axis and its cap on the voxels.                                                                                     */
#define PVAMD_LATTICE_MAX_AXIS 2048

/* ---- Distance transform (SDF from voxel occupancy) ----
 * The exact Euclidean distance transform of an occupancy grid, fused with the statements that turn it into the packed (val, gx,
 * gy, gz) records of a cached voxel grid (pvamd_grid_t.vox): the producer for scenes that are observed as voxels, not given as
 * a mesh.  Replaces nothing in the reference: its VoxelGrid (voxel.py:42-103) holds the occupancy and nothing there turns it
 * into a distance field.
 *  1. occupied: device uint8 [nx][ny][nz] in C order (x slowest, z fastest, the layout of the records), non-zero = occupied.
 *     For voxel i = (x, y, z) the site class Q is: the occupied voxels when i is free; the free voxels when i is occupied and
 *     is_signed = 1; {i} itself when i is occupied and is_signed = 0.
 *  2. squared(i) = min over j in Q of |i - j|^2 in voxel units, exact in int32 (at most 3 * 2047^2 < 2^24).  site(i) = the
 *     SMALLEST flat C-order index j = (jx * ny + jy) * nz + jz that attains it: the gradient depends on this tie rule.
 *  3. With r = resolution and s = sqrtf((float)squared), each operation rounded on its own (correctly rounded sqrt and divide,
 *     no contraction), j = site(i):
 *       is_signed = 1, i free:      val = r * (s - 0.5f)         the surface lies on the voxel faces between the two classes,
 *       is_signed = 1, i occupied:  val = -(r * (s - 0.5f))      half a voxel from either centre
 *       is_signed = 0:              val = r * s                  an occupied voxel: +0.0, gradient zeros, site i
 *       gradient component k:       (float)(i_k - j_k) / s for a free voxel, (float)(j_k - i_k) / s for an occupied one
 *                                   (toward increasing val)
 *  4. Empty Q (no occupied voxel; is_signed = 1 and no free voxel): squared = PVAMD_EDT_NO_SITE, site = -1, val = +INFINITY for a
 *     free voxel and -INFINITY for an occupied one, gradient zeros.  These are ordinary results, reported without a
 *     synchronisation.
 *  5. Three line passes (z, y, x; the last fused with 3.) that keep one int32 per voxel and class in scratch; no sum ever
 *     includes the no-site sentinel.  The line minima are found by an outward scan that stops once the offset alone exceeds the
 *     best cost: the time grows with the distances in the grid, up to the line length per voxel and pass in empty space.
 * Each axis in [PVAMD_EDT_MIN_AXIS, PVAMD_LATTICE_MAX_AXIS] and nx * ny * nz <= PVAMD_EDT_MAX_VOXELS (sites is an int32), else
 * PVAMD_E_SHAPE; is_signed other than 0 / 1: PVAMD_E_MODE.
 * records: device [n][4] float32, 16-byte aligned (n = nx * ny * nz).  sites, squared: device [n] int32, or NULL (not wanted).
 * scratch: device, pvamd_distance_transform_scratch_bytes(nx, ny, nz, is_signed) bytes, 4-byte aligned; that function is the
 * definition (0 for arguments the entry point refuses) and there is no macro.  Contents on return are unspecified.
 * Stream-ordered, no allocation, no device -> host synchronisation, no atomics: capturable in a graph, and two calls give the
 * same bits.                                                                                                                    */
#define PVAMD_EDT_NO_SITE 2147483647  /* INT32_MAX: squared(i) when Q is empty */
#define PVAMD_EDT_MIN_AXIS 1
#define PVAMD_EDT_MAX_VOXELS 2147483647 /* 2^31 - 1 */
int64_t pvamd_distance_transform_scratch_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t is_signed);
int pvamd_distance_transform(const uint8_t* occupied, int32_t nx, int32_t ny, int32_t nz, float resolution, int32_t is_signed,
                             float* records, int32_t* sites, int32_t* squared, void* scratch, void* stream);

/* ---- Ray integration (occupancy from sensor rays) ----
 * One pvamd_ray_mark call classifies the voxels of a lattice by one SCAN of R rays, each from an origin o (the sensor) to an
 * endpoint e (the return), the way OctoMap's insertPointCloud does; pvamd_occupancy_update then moves a log-odds map by that
 * classification.  Replaces nothing in the reference: its voxel.py stops at the containers, whose only producer is
 * grid[points] = value.
 *  1. Marks.  After a scan on zeroed marks a voxel holds PVAMD_MARK_HIT when it is the hit voxel (3.) of at least one ray,
 *     PVAMD_MARK_FREE when it is no ray's hit voxel and the traversal (6.) of at least one ray visited it, 0 when no ray
 *     touched it.  A hit takes precedence over any number of traversals, which also makes the result independent of the order of
 *     the rays.  Marks of two calls accumulate: the traversal writes FREE only where the mark is 0, the hits overwrite.
 *  2. Lattice.  grid: a finalized descriptor (vox unused, as for the voxel scatter entry points), each axis n_k in
 *     [PVAMD_RAY_MARK_MIN_AXIS, PVAMD_LATTICE_MAX_AXIS].
 *     s_k(p) = (p_k - fmin_k) / fres_k in float32 (IEEE division); voxel i of axis k is the cell [i - 0.5, i + 0.5) in s.  The
 *     traversal always uses the float32 fields, whatever index_f64 says.  EVERYTHING below is float32 with every operation
 *     rounded on its own (no contraction, correctly rounded division and square root).
 *  3. Hit voxel.  The voxel pvamd_voxel_scatter_* writes for the point e: the flat index of pvamd_voxel_index under the grid's
 *     own rule and index_f64.  A ray has no hit voxel when e fails that range test, when the ray is ignored (4.) or cut (5.).
 *  4. Ignored rays.  A ray with a non-finite coordinate in o or e marks nothing.
 *  5. Range limit.  With v = e - o: len = sqrtf((v_x * v_x + v_y * v_y) + v_z * v_z).  When len > max_range the ray is cut: it
 *     has no hit voxel and is traversed up to t_end = max_range / len.  Otherwise t_end = 1.  max_range = +INFINITY: no limit.
 *  6. Traversal.  a = s(o), b = s(e), d = b - a.  Nothing is visited unless every d_k is finite.
 *     a. Clip to the box, starting from t0 = 0, t1 = t_end.  An axis with d_k == 0: nothing is visited unless
 *        -0.5 <= a_k < n_k - 0.5.  Any other axis: u = (-0.5 - a_k) / d_k, w = (n_k - 0.5 - a_k) / d_k,
 *        t0 = fmaxf(t0, fminf(u, w)), t1 = fminf(t1, fmaxf(u, w)).  Nothing is visited unless t0 <= t1.
 *     b. Start cell: c_k = (int)fminf(fmaxf(floorf((a_k + t0 * d_k) + 0.5f), 0), n_k - 1).
 *     c. step_k = sign(d_k) (0 for d_k == 0).  tmax_k = (((float)c_k + 0.5f * step_k) - a_k) / d_k, +INFINITY when d_k == 0:
 *        where the ray leaves cell c along axis k.  It is recomputed from the cell after every step, never accumulated.
 *     d. At most n_x + n_y + n_z times: visit c; take the axis k with the smallest tmax_k, the lowest axis on a tie; stop unless
 *        tmax_k < t1; c_k += step_k; stop when that leaves the grid; recompute tmax_k.
 *     The walk moves by one cell along one axis and never turns back, so it repeats no cell.  It ends in the hit voxel of a
 *     generic ray that ends inside the grid; where an endpoint or a crossing sits on a cell boundary it may end in a cell next
 *     to it, which then carries FREE beside the HIT.
 *  7. Launches: the traversal (one lane per ray; plain byte stores, every writer storing the same value), then the hits in a
 *     launch of their own, so that the precedence rests on stream order alone and nothing is handed between workgroups inside a
 *     kernel.  No atomics.
 *  8. Update, one pass over the voxels, fused with clearing the marks: HIT: L = fminf(fmaxf(L + l_hit, l_min), l_max); FREE: the
 *     same with l_miss; 0: L keeps its bits.  observed |= (mark != 0) where observed is given.  Every mark is 0 on return.
 * Argument errors return before any launch: PVAMD_E_SHAPE for R < 0, n < 0 or an axis outside those limits; PVAMD_E_NULL;
 * PVAMD_E_MODE for a max_range that is NaN or <= 0, a shared_origin other than 0 / 1, a NaN among l_hit, l_miss, l_min, l_max or
 * l_min > l_max; PVAMD_E_ALIGN for log_odds not 16-byte, marks (of the update) or observed not 4-byte aligned.
 * origins: device [1][3] when shared_origin = 1 (one eye for a whole image), else [R][3].  endpoints: device [R][3].
 * marks: device uint8 [n_x * n_y * n_z] in C order, zero on entry where the caller wants a fresh scan.
 * log_odds: device float32 [n].  observed: device uint8 [n] (0 / 1) or NULL.
 * Stream-ordered, no allocation, no device -> host synchronisation: capturable in a graph, and two calls give the same bits. */
#define PVAMD_MARK_FREE 1
#define PVAMD_MARK_HIT  2
#define PVAMD_RAY_MARK_MIN_AXIS 2
int pvamd_ray_mark(const pvamd_grid_t* grid, const float* origins, int32_t shared_origin, const float* endpoints, int64_t R,
                   float max_range, uint8_t* marks, void* stream);
int pvamd_occupancy_update(uint8_t* marks, int64_t n, float l_hit, float l_miss, float l_min, float l_max, float* log_odds,
                           uint8_t* observed, void* stream);

/* ---- TSDF integration (truncated signed distance volumes from depth images) ----
 * pvamd_tsdf_integrate averages K depth images into a truncated signed distance volume, the integration step of Curless & Levoy
 * and KinectFusion, in ONE pass over the volume: a voxel's state is read once, taken through the K frames in order in registers
 * and written once.  pvamd_tsdf_records turns the state into the packed (val, gx, gy, gz) records of a cached voxel grid
 * (pvamd_grid_t.vox).  Replaces nothing in the reference: its voxel.py stops at the containers.
 * EVERYTHING below is float32 with every operation rounded on its own (no contraction, correctly rounded division and square
 * root).
 *  1. State.  state: device [n][2] float32, (F, W) per voxel in C order (x slowest, z fastest): the running average of the
 *     truncated signed distance in units of the truncation, F in [-1, 1], and its weight.  A fresh volume is all +0.0.  The state
 *     of a voxel is read once before the first frame and written once after the last, and only if some frame updated the voxel:
 *     an untouched voxel keeps its bits, -0.0 included.  One call over K frames gives, bit for bit, what K calls of one frame
 *     each give in that order.
 *  2. Lattice.  grid: a finalized descriptor (vox unused), each axis n_j in [PVAMD_TSDF_MIN_AXIS, PVAMD_LATTICE_MAX_AXIS].  The
 *     centre of voxel i = (x, y, z) is
 *     c_j = fmin_j + (float)i_j * fres_j: always the descriptor's float32 fields, as in "Ray integration" 2.
 *  Per voxel, for frame k = 0 .. K-1 in order, with T = camera_from_volume[k] (the camera looks along +z, x right, y down):
 *  3. p_r = ((T[r][0] * c_x + T[r][1] * c_y) + T[r][2] * c_z) + T[r][3] for r = 0, 1, 2.  The frame is skipped unless p_z > 0.
 *  4. u = fx * (p_x / p_z) + cx, v = fy * (p_y / p_z) + cy.  Pixel (row, col) covers [col - 0.5, col + 0.5) in u.  Skipped unless
 *     -0.5 <= u < (float)W - 0.5 and -0.5 <= v < (float)H - 0.5: tested in float before any conversion, and NaN fails it.
 *  5. col = (int)floorf(u + 0.5f), row = (int)floorf(v + 0.5f), each clamped into [0, W - 1] / [0, H - 1] after the conversion
 *     (the rounded sum can reach W).
 *  6. d = depth[(k * H + row) * W + col]: z-depth along the optical axis, not range.  Skipped unless d > 0, d is finite and
 *     d <= max_depth (zero, negative, NaN and infinite depths mean "no return"; max_depth = +INFINITY: no limit).
 *  7. sdf = d - p_z.  Skipped unless sdf >= -truncation: a voxel further than the band behind the surface is unobserved.
 *  8. f = fminf(sdf / truncation, 1.0f): free space in front of a surface is evidence too.
 *  9. With (Fo, Wo) the voxel's state: Wn = Wo + weight, F = ((Wo * Fo) + (weight * f)) / Wn, W = fminf(Wn, max_weight).
 *  Records, per voxel i (pvamd_tsdf_records):
 * 10. Known iff W > min_weight.  t = known ? F : unknown_tsdf (+1: unknown space is free, -1: occupied), val = truncation * t.
 * 11. Per axis j: lo = max(i_j - 1, 0), hi = min(i_j + 1, n_j - 1), g_j = (val(hi) - val(lo)) / ((float)(hi - lo) * resolution),
 *     val of the neighbours by the same substitution (one-sided at the border).
 * 12. len = sqrtf((g_x * g_x + g_y * g_y) + g_z * g_z).  The record is (val, g_x / len, g_y / len, g_z / len) when len > 0, else
 *     (val, 0, 0, 0).  The gradients have unit length, as the mesh and distance-transform records have: consumers use them as
 *     the surface normal.  Saturated regions, |t| = 1 all round, get zero gradients.  The field is TRUNCATED: |val| never exceeds
 *     the truncation, which suits sphere tracing, hinge margins up to the truncation and registration, and is wrong for anyone
 *     who reads far-field distances ("Redistancing" below completes it).
 * Argument errors return before any launch: PVAMD_E_SHAPE for K < 0, H or W < 1, K * H * W > PVAMD_TSDF_MAX_PIXELS, an axis
 * outside those limits or more than PVAMD_TSDF_MAX_VOXELS voxels; PVAMD_E_NULL; PVAMD_E_MODE for non-finite intrinsics, fx or
 * fy <= 0, a truncation, weight or resolution that is non-finite or <= 0, a max_weight or max_depth that is NaN or <= 0
 * (+INFINITY is allowed), a NaN min_weight, an unknown_tsdf other than +1 / -1; PVAMD_E_ALIGN for state not 8-byte, records not
 * 16-byte aligned.  K = 0 returns 0 without a launch.
 * depth: device [K][H][W] float32.  camera_from_volume: device [K][3][4] float32, the rigid inverse of the camera's pose in the
 * volume's frame.  records: device [n][4] float32.
 * One launch each.  Stream-ordered, no allocation, no device -> host synchronisation, no atomics: capturable in a graph, and two
 * calls give the same bits.                                                                                                    */
#define PVAMD_TSDF_MIN_AXIS 2
#define PVAMD_TSDF_MAX_VOXELS 2147483647 /* 2^31 - 1 */
#define PVAMD_TSDF_MAX_PIXELS 2147483647 /* 2^31 - 1 */
int pvamd_tsdf_integrate(const pvamd_grid_t* grid, const float* depth, int32_t K, int32_t H, int32_t W,
                         const float* camera_from_volume, float fx, float fy, float cx, float cy, float truncation,
                         float max_depth, float weight, float max_weight, float* state, void* stream);
int pvamd_tsdf_records(const float* state, int32_t nx, int32_t ny, int32_t nz, float resolution, float truncation,
                       float min_weight, float unknown_tsdf, float* records, void* stream);

/* ---- Redistancing (full Euclidean distance fields from sampled signed fields) ----
 * pvamd_redistance measures, from every voxel, the Euclidean distance to the zero set of a signed field sampled on the lattice,
 * the zero set taken at sub-voxel precision where the samples change sign along the lattice edges: "ESDF from TSDF".  With
 * band = truncation it completes the records of pvamd_tsdf_records: the band round the surface is kept bit for bit, everything
 * else becomes a distance with a unit gradient.  Replaces nothing in the reference.
 * EVERYTHING below is float32 with every operation rounded on its own (no contraction, no fma, correctly rounded division and
 * square root).  Coordinates are in voxels until statement 7.
 *  1. Input.  records_in: device [n][4] float32 packed (val, gx, gy, gz) in C order (x slowest, z fastest), n = nx * ny * nz.
 *     V_i is the val of voxel i.  Only kept voxels (6.) read the gradients.
 *  2. Crossings.  For axis k and a voxel a with a_k < n_k - 1, b = a + e_k: the lattice edge (a, b) carries a crossing iff V_a and
 *     V_b are both finite and (V_a < 0) != (V_b < 0).  It lies at a_k + f along k, f = V_a / (V_a - V_b) in [0, 1], and at a's
 *     integers on the other two axes.  Its family is k.  A NaN or infinite sample gives its edges no crossing.
 *  3. Cost of a crossing of family k to voxel i.  t = (float)(i_k - a_k) - f.  With p2 > p3 the remaining axes, highest index
 *     first (x: (z, y); y: (z, x); z: (y, x)) and d_j = i_j - a_j exact in int:
 *         c1 = t * t,  c2 = c1 + (float)(d_p2 * d_p2),  c3 = c2 + (float)(d_p3 * d_p3).
 *     Rounding is monotone, so nested line minima give the minimum of c3 over all crossings, and a candidate at offset d along
 *     the line of a pass costs at least (float)(d * d).
 *  4. Site.  Defined by the nesting.  Pass 1, along k: per voxel, the crossing on the voxel's own line with the smallest c1, the
 *     smaller a_k on a tie.  Pass 2, along p2: among the pass-1 results of the voxels of the line, the smallest c2, the smaller
 *     coordinate along p2 on a tie.  Pass 3, along p3, likewise with c3.  Across the families the smallest c3 wins, the lowest k
 *     on a tie.  sites[i] = ((a_x * ny + a_y) * nz + a_z) * 4 + k, squared[i] = c3.
 *  5. Range.  Rv = max_distance / resolution, R2 = Rv * Rv; max_distance = +INFINITY: no limit.  A candidate whose cost exceeds
 *     R2 at any stage may be dropped: it cannot change a result that 5. does not overwrite.  A voxel without a site, or whose
 *     c3 > R2, gets sites = -1, squared = +INFINITY, val = max_distance (-max_distance when V_i < 0) and a zero gradient.
 *  6. Kept voxels.  fabsf(V_i) < band: the output record is the input record bit for bit, sites = PVAMD_REDIST_KEPT, squared =
 *     +INFINITY.  band = 0 keeps nothing; a NaN V_i is never kept and counts as not negative.
 *  7. Every other voxel, len = sqrtf(c3): val = resolution * len, negated when V_i < 0.  Gradient: t / len on the site's axis,
 *     (float)d_j / len on the other two, all three negated when V_i < 0, zeros when c3 == 0.
 *  8. Three line passes per family, each an outward scan that stops once (float)(d * d) exceeds min(best, R2): in space without
 *     crossings a scan runs to both ends of its line, and max_distance is what bounds that.  The time grows with the distances
 *     in the grid, as the distance transform's does.
 * Argument errors return before any launch, tested in this order: PVAMD_E_SHAPE for an axis outside
 * [PVAMD_REDIST_MIN_AXIS, PVAMD_LATTICE_MAX_AXIS] or n > PVAMD_REDIST_MAX_VOXELS (sites = flat * 4 + k is an int32);
 * PVAMD_E_MODE for a resolution that is non-finite or <= 0, a band that is NaN or < 0, a max_distance that is NaN or <= 0;
 * PVAMD_E_NULL (sites and squared may be NULL: not wanted); PVAMD_E_ALIGN for records not 16-byte, scratch, sites or squared not
 * 4-byte aligned.
 * records_in is never written and must not overlap records_out: device [n][4] float32.  sites: device [n] int32.  squared: device
 * [n] float32.  scratch: device, pvamd_redistance_scratch_bytes(nx, ny, nz) bytes, 4-byte aligned; that function is the
 * definition (0 for shapes the entry point refuses) and there is no macro.  Contents on return are unspecified.
 * Stream-ordered, no allocation, no device -> host synchronisation, no atomics: capturable in a graph, and two calls give the
 * same bits.                                                                                                                    */
#define PVAMD_REDIST_KEPT (-2) /* sites[i] of a voxel inside the band */
#define PVAMD_REDIST_MIN_AXIS 2
#define PVAMD_REDIST_MAX_VOXELS 536870912 /* 2^29 */
int64_t pvamd_redistance_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int pvamd_redistance(const float* records_in, int32_t nx, int32_t ny, int32_t nz, float resolution, float band, float max_distance,
                     float* records_out, int32_t* sites, float* squared, void* scratch, void* stream);

/* ---- Surface extraction (triangle meshes from sampled signed fields) ----
 * pvamd_surface_count and pvamd_surface_emit turn the level set of a field sampled on the lattice into an indexed triangle mesh by
 * naive surface nets (dual contouring without a QEF): one vertex per lattice cell the surface passes through, placed at the mean
 * of the crossings on the cell's edges, and one quad (two triangles) per lattice edge that carries a crossing.  No case table.
 * count sizes the result and prepares scratch; emit writes it.  Replaces nothing in the reference.
 * EVERYTHING below is float32 with every operation rounded on its own (no contraction, no fma, correctly rounded division and
 * square root).
 *  1. Samples.  records: device [n][4] float32 packed (val, gx, gy, gz) in C order, V_i the val of voxel i; W_i = V_i - level.
 *     A sample is usable iff W_i is finite and (valid == NULL or valid[i] != 0); it is negative iff W_i < 0.
 *  2. Crossings.  For axis k and a voxel a with a_k < n_k - 1, b = a + e_k: the lattice edge (a, b) carries a crossing iff both
 *     ends are usable and (W_a < 0) != (W_b < 0).  It lies at f = W_a / (W_a - W_b) along k.  With level = 0 and valid = NULL
 *     these are exactly the crossings of "Redistancing" 2.
 *  3. Cells.  Cell c, c_j <= n_j - 2 on every axis, has the corners c + {0, 1}^3.  It is active iff all eight corners are usable
 *     and they are not all negative and not all non-negative.  A cell with an unusable corner emits nothing: no surface between
 *     seen and unseen space.
 *  4. Vertex of an active cell.  The twelve edges in this order: the four along x by (dy, dz) = (0,0), (0,1), (1,0), (1,1), then
 *     the four along y by (dx, dz), then the four along z by (dx, dy), in the same order.  Starting from S = (0, 0, 0) and m = 0,
 *     each edge that carries a crossing adds its offset inside the cell to S, component by component -- f on the edge's own
 *     axis, the edge's 0 / 1 on the other two -- and 1 to m.  p_j = (float)c_j + S_j / (float)m in voxels, and the vertex is
 *     P_j = fmin_j + p_j * fres_j with the lattice of "TSDF integration" 2. (the descriptor's float32 fields): a whole p gives
 *     the voxel's centre bit for bit.
 *  5. Normal (normals != NULL).  In the same edge order, from N = (0, 0, 0): N_j = N_j + (g_a,j + f * (g_b,j - g_a,j)) with g the
 *     gradients of the records at the edge's ends.  len = sqrtf((N_x * N_x + N_y * N_y) + N_z * N_z); the row is N / len when
 *     len > 0 and finite, else zeros.
 *  6. Vertex ids.  The active cells, numbered in flat C order of c.  Every active cell has a vertex, also one that no face names
 *     (on the lattice's border, next to unusable samples).
 *  7. Faces.  A crossing of family k at a emits one quad iff the four cells round its edge exist and are active: with (p, q) the
 *     other axes in cyclic order (x: (y, z); y: (z, x); z: (x, y)), C0 = a - e_p - e_q, C1 = a - e_q, C2 = a, C3 = a - e_p.  Its
 *     vertices are (v0, v1, v2, v3) = ids of (C0, C1, C2, C3) when W_a < 0 and of (C0, C3, C2, C1) otherwise, so that the face
 *     normals point to the non-negative side; its triangles are (v0, v1, v2) and (v0, v2, v3), in consecutive rows.  Quads are
 *     ordered by flat(a) * 3 + k.  counts = (number of vertices, number of triangles).
 *  8. Capacities.  emit writes the vertex (and normal) rows < max_vertices and the face rows < max_faces and not a byte beyond
 *     them: complete with capacities >= counts, the exact prefix with smaller ones (faces may then name vertices that were not
 *     written).  A fixed budget makes count + emit capturable in a graph.  scratch as count left it serves any number of emit
 *     calls while records, valid, level and the shape are unchanged; emit does not write it.
 *  9. Topology, documented and not promised: a closed field away from the border gives a closed, consistently oriented mesh
 *     wherever every cell's sign pattern is unambiguous; ambiguous patterns can give an edge four triangles, and an f of
 *     exactly 0 or 1 can make two vertices of a quad coincide (a degenerate triangle).
 * grid: a finalized descriptor used as the lattice only (vox unused); each axis in [PVAMD_SURFACE_MIN_AXIS,
 * PVAMD_LATTICE_MAX_AXIS] and n <= PVAMD_SURFACE_MAX_VOXELS: vertex ids and quad counts (<= 3 n) then fit an int32, and the
 * triangle counts are int64.  Argument errors return before any launch, tested in this order: PVAMD_E_NULL for grid;
 * PVAMD_E_SHAPE for those limits or a negative capacity; PVAMD_E_MODE for a descriptor that is not finalized and for a NaN or
 * infinite level; PVAMD_E_NULL (valid and normals may be NULL; vertices / faces only with a capacity of zero); PVAMD_E_ALIGN for
 * records not 16-byte, counts not 8-byte, scratch, vertices, normals or faces not 4-byte aligned.
 * records and valid (device [n] uint8) are never written.  counts: device [2] int64.  vertices, normals: device
 * [max_vertices][3] float32.  faces: device [max_faces][3] int32.  scratch: device, pvamd_surface_scratch_bytes(nx, ny, nz) bytes,
 * 4-byte aligned; that function is the definition (0 for shapes the entry points refuse) and there is no macro.  The ids come
 * from an exclusive scan over blocks of PVAMD_SURFACE_CHUNK consecutive voxels, whose sums one workgroup scans
 * PVAMD_SURFACE_SCAN_WIDTH at a time; in-wave ranks are popcounts of lower lanes.
 * Stream-ordered, no allocation, no device -> host synchronisation, no atomics: capturable in a graph, and two calls give the
 * same bits.                                                                                                                    */
#define PVAMD_SURFACE_MIN_AXIS 2
#define PVAMD_SURFACE_MAX_VOXELS 536870912 /* 2^29 */
#define PVAMD_SURFACE_CHUNK 256
#define PVAMD_SURFACE_SCAN_WIDTH 1024
int64_t pvamd_surface_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int pvamd_surface_count(const pvamd_grid_t* grid, const float* records, const uint8_t* valid, float level, void* scratch,
                        int64_t* counts, void* stream);
int pvamd_surface_emit(const pvamd_grid_t* grid, const float* records, const uint8_t* valid, float level, const void* scratch,
                       int64_t max_vertices, int64_t max_faces, float* vertices, float* normals, int32_t* faces, void* stream);

/* ---- Mesh ray casting (the first hit of rays on a triangle mesh) ----
 * pvamd_mesh_ray_cast finds, for each of B poses and R rays o + t d, the triangle of a prepared mesh the ray meets first: what
 * the reference's users get from cast_rays on the open3d RaycastingScene every ObjectFactory keeps (sdf.py:115-118).  Exact: the
 * result is that of the plain loop over all F triangles, not of a march that stops within a tolerance.  An additive entry point:
 * the ABI version is unchanged.
 * EVERYTHING below is float32 with every operation rounded on its own: no contraction; fmaf(a, b, c) is one fused, once-rounded
 * a * b + c exactly where it is written, as in the mesh query's sequences (csrc/mesh_math.h); correctly rounded division.
 * dot(a, b) = fmaf(a_z, b_z, fmaf(a_y, b_y, a_x * b_x)); cross(a, b) = (fmaf(a_y, b_z, -(a_z * b_y)), fmaf(a_z, b_x, -(a_x * b_z)),
 * fmaf(a_x, b_y, -(a_y * b_x))).
 *  1. The ray in the object frame.  poses == NULL: o' = o, d' = d.  With pose b, M = poses[b] row-major, world_to_object:
 *     o'_i = fmaf(M[4i+2], o_z, fmaf(M[4i+1], o_y, M[4i] * o_x)) + M[4i+3]  -- affine_row, the statement of pvamd_chamfer_mesh and
 *     the composed queries -- and d'_i = fmaf(M[4i+2], d_z, fmaf(M[4i+1], d_y, M[4i] * d_x)): the same chain without the translation.
 *     The last row of M is not read.
 *  2. Candidates.  For a triangle (v0, v1, v2) = the corners (a, b, c) of a face, as float32: e1 = v0 - v1, e2 = v2 - v0,
 *     Ng = cross(e2, e1), C = v0 - o', Rv = cross(C, d'), den = dot(Ng, d'), absden = |den|, sgn = -1 if den < 0 else 1,
 *     U = dot(Rv, e2) * sgn, V = dot(Rv, e1) * sgn, T = dot(Ng, C) * sgn -- ray_hits_triangle's sequence of the mesh query's
 *     parity rays -- and t = T / absden.  The triangle is a candidate iff den != 0, U >= 0, V >= 0, U + V <= absden, t >= t_min and
 *     t <= t_max.  A NaN fails its comparison (den != 0 alone holds for a NaN den; U >= 0 then fails): a ray with a NaN or
 *     infinite coordinate, or a zero direction, has no candidate.  Edges and corners are inclusive, both faces of a triangle count.
 *  3. Result.  Of the candidates, the one with the smallest t; among equal t (-0 equals +0) the one with the smallest ORIGINAL
 *     face id -- the lexicographic rule of the closest-point query, whatever order the triangles are stored or visited in.
 *     t_out = its t, face_out = its id, uv_out = (U / absden, V / absden), two more divisions: the hit is
 *     (1 - u - v) a + u b + v c -- u weights corner b, v corner c -- up to rounding.  normal_out = mesh->normal[face], the
 *     stored unit face normal, NOT flipped towards the ray; with a pose it is taken back into the rays' frame by the transpose
 *     of M's 3 x 3 block, n_j = fmaf(M[8+j], n_z, fmaf(M[4+j], n_y, M[j] * n_x)).  Either way each component is written as n_j + 0, so
 *     that a zero leaves as +0 and the identity pose gives the bits of poses == NULL.  No candidate: t_out = +inf, face_out = -1,
 *     normal_out and uv_out zeros.
 *  4. t is the parameter of o + t d for the caller's d, of any length; a pose is affine, so t is the same number in both
 *     frames.  The normal taken back by the transpose is the normal in the rays' frame for RIGID poses only (orthonormal block);
 *     nothing checks rigidity.
 * mesh: host struct (pvamd_mesh_prepare's buffers; of them rec and normal are read, and F).  origins, directions: device [R][3].
 * poses: NULL (B must be 1) or device [B][16].  t_out: device [B][R] float32; face_out: device [B][R] int32; normal_out: device
 * [B][R][3] or NULL; uv_out: device [B][R][2] or NULL: the rays are shared by the poses.
 * Argument errors return before any launch: PVAMD_E_SHAPE for R < 0, B < 0, poses == NULL with B != 1, B * R >= 2^31 or F outside
 * [0, 2^26]; PVAMD_E_NULL; PVAMD_E_MODE for a NaN t_min or t_max; PVAMD_E_ALIGN for records not 16-byte aligned.
 * R == 0 or B == 0: nothing is launched or written.  F == 0 or t_min > t_max: every ray misses.
 * One lane per (pose, ray), rays in caller order; every wave tests its rays against all F records (wave-uniform loads).  Nothing
 * is culled, although the records carry bounding spheres: for a ray that lies, up to rounding, in a triangle's plane, den, U, V
 * and T of 2. are all rounding noise and the triangle can be a candidate, with any t, wherever in that plane the line runs -- also
 * wholly behind the origin or far beside the line.  The statements above are the definition, so no sphere may be skipped.
 * Stream-ordered, no allocation, no device -> host synchronisation, no atomics: capturable in a graph, and two calls give the
 * same bits.  mesh->pair_counters is not used.                                                                                  */
int pvamd_mesh_ray_cast(const pvamd_mesh_t* mesh, const float* origins, const float* directions, int64_t R, const float* poses,
                        int32_t B, float t_min, float t_max, float* t_out, int32_t* face_out, float* normal_out, float* uv_out,
                        void* stream);

/* ---- Mesh ray casting, culled (the same call with the bounding spheres of the prepared mesh as part of the definition) ----
 * pvamd_mesh_ray_cast_culled has the signature of pvamd_mesh_ray_cast and a second, opt-in contract, stated as strictly as the
 * first: a triangle is a candidate only if, in addition, the ray (sphere_ok) and the candidate's own point o' + t d'
 * (point_ok) pass the float32 tests below against the two bounding spheres pvamd_mesh_prepare wrote for the triangle's record
 * -- that of its tile (PVAMD_TRI_TILE records) and that of its group (PVAMD_TRI_GROUP records).  It exists because the plain contract cannot be culled (the end of "Mesh ray casting"), and costs
 * rays x triangles.  An additive entry point: the ABI version is unchanged.
 * The rules of "Mesh ray casting" hold: float32, every operation rounded on its own, fmaf exactly where it is written, the same
 * dot and cross; sqrt is correctly rounded.  Steps 1, 3 and 4 apply unchanged.  Step 2 gains two conditions: with j =
 * rec_of_face[f] the position of the triangle's record and T = ceil(F / PVAMD_TRI_TILE), the ray passes sphere_ok, and the t of
 * step 2 passes point_ok, for the tile sphere tiles[4 (j / PVAMD_TRI_TILE) ...] AND for the group sphere
 * tiles[4 T + 4 (j / PVAMD_TRI_GROUP) ...].  Both spheres are required: that the group's sphere lies inside the tile's is not
 * provable in float32, so neither test stands for the other.
 *   per ray, after the pose:   dd = dot(d', d');   len = sqrt(dd)
 *   per sphere (c, r):         w = c - o';   q = cross(w, d');   qq = dot(q, q);   ww = dot(w, w);   wd = dot(w, d')
 *                              rs = fmaf(4e-7f, sqrt(ww), r * 1.00001f)
 *   sphere_ok  :=  qq <= (rs * rs) * dd                  the line meets the inflated sphere
 *              and fmaf( rs, len, wd) >= t_min * dd      the sphere is not wholly before t_min
 *              and fmaf(-rs, len, wd) <= t_max * dd      the sphere is not wholly beyond t_max
 *   point_ok   :=  dot(v, v) <= rs * rs,  v_i = fmaf(t, d'_i, -w_i)     the point o' + t d' lies in the inflated sphere
 * sphere_ok does not know t, so whole tiles and groups can be skipped by it; point_ok is what ties the t of a candidate to its
 * spheres.  Without it a ray in a triangle's rounded plane whose line does pass the sphere keeps its noise candidate, with
 * any t: of 30,000 such rays at a rotated box one kept a hit 3.88 from the centre of a sphere of radius 2.6.
 * A NaN fails its comparison and inf * 0 is NaN: a ray with a NaN or infinite coordinate, or a zero direction, has no candidate, as in the plain
 * mode (a zero direction under a finite window passes the spheres and fails den != 0).
 * The slack.  4e-7 |w| covers the float32 evaluation of q and wd for a line that meets the stored sphere in real arithmetic
 * (|w x d'| <= r |d'|): w carries a relative error of 2^-24 per component (the sphere moved by at most 2^-24 |w|); each
 * component of q adds the rounding of one product and of the fmaf, together at most 2^-24 (|w||d'| + |q|) as a vector; wd adds
 * three roundings of terms bounded by |w||d'|.  To first order |q - w x d'| and |wd - w . d'| are both at most
 * 4 * 2^-24 |w||d'| = 2.4e-7 |w||d'| < 4e-7 |w||d'| (tests/test_mesh_ray_cull.py measures it).  The factor 1.00001 covers what is
 * relative to r: the roundings of qq, ww, dd, len, rs and the products of the comparison, under 16 * 2^-24 = 1e-6 together.  This
 * holds while nothing under- or overflows.  v of point_ok carries the error of w and one rounding, 2^-24 (|w| + |v|), inside
 * the same slack.  All of this bounds the evaluation of the tests, not t: the t of a candidate is the float32 t of step 2, whose
 * own error is not covered -- a triangle met at a grazing angle at the very rim of its sphere may be inside by its corners and
 * outside by its t.
 * No candidate is dropped because of a hit already held: "the sphere begins beyond the best t so far" would depend on the order
 * of the records, and is not part of this contract.
 * Consequences.  Every culled result is a candidate of the plain loop, and its point lies in the inflated spheres of its
 * triangle.  The two modes differ only where the plain winner is a candidate that fails sphere_ok or point_ok of its own
 * triangle: in practice the rays of "Mesh ray casting" that lie, up to rounding, in a triangle's plane, whose t is noise.  Which tile and group a triangle
 * sits in follows the order given to pvamd_mesh_prepare, so the results on such rays may depend on that order; the plain mode's
 * never do.  Groups that begin at or past F have no sphere and are never read as a test.
 * mesh: as for pvamd_mesh_ray_cast, and `tiles` is read as well.  All other arguments, the outputs, the error codes, R == 0 or
 * B == 0 and the miss path for F == 0 or t_min > t_max are those of pvamd_mesh_ray_cast; in addition PVAMD_E_NULL for F > 0 without
 * `tiles`.
 * One lane per (pose, ray), rays in caller order.  A wave skips a tile, and in a tile a group, whose sphere none of its 64 rays
 * passes, so it executes the exact tests of the union of its rays' surviving groups: rays that are neighbours in space should
 * be neighbours in the call.  Stream-ordered, no allocation, no device -> host synchronisation, no atomics: capturable in a
 * graph, and two calls give the same bits.  mesh->pair_counters is not used.                                                  */
int pvamd_mesh_ray_cast_culled(const pvamd_mesh_t* mesh, const float* origins, const float* directions, int64_t R,
                               const float* poses, int32_t B, float t_min, float t_max, float* t_out, int32_t* face_out,
                               float* normal_out, float* uv_out, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* PVAMD_H */
