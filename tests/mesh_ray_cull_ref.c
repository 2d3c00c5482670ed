/* Restatement of include/pvamd.h "Mesh ray casting, culled" for its tests -- TEST INFRASTRUCTURE.  The plain loop of
 * mesh_ray_ref.c -- every pose, every ray, every triangle of the float32 soup in ORIGINAL face order -- with the section's
 * sphere_ok and point_ok as further conditions of a candidate, for the sphere of the tile and the sphere of the group the
 * triangle's record sits in, found through rec_of_face and the `tiles` array, both documented in pvamd_mesh_t.  Nothing of
 * the opaque record layout is read.  Compiled with -ffp-contract=off, so that a product and a sum are fused exactly where fmaf is written.  Shares no code
 * with csrc/. */
#include <math.h>
#include <stdint.h>

#define TILE 256 /* PVAMD_TRI_TILE */
#define GROUP 16 /* PVAMD_TRI_GROUP */

static float dot3(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

static void cross3(const float a[3], const float b[3], float out[3]) {
    out[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
    out[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
    out[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}

/* sphere: (cx, cy, cz, r); o, d: the ray in the object frame; dd = dot(d, d), len = sqrt(dd) */
static int sphere_ok(const float* sphere, const float o[3], const float d[3], float dd, float len, float t_min, float t_max) {
    float w[3], q[3];
    for (int i = 0; i < 3; ++i) w[i] = sphere[i] - o[i];
    cross3(w, d, q);
    const float qq = dot3(q, q), ww = dot3(w, w), wd = dot3(w, d);
    const float rs = fmaf(4e-7f, sqrtf(ww), sphere[3] * 1.00001f);
    return qq <= (rs * rs) * dd && fmaf(rs, len, wd) >= t_min * dd && fmaf(-rs, len, wd) <= t_max * dd;
}

/* point_ok of the section: the candidate's point o + t d lies in the inflated sphere */
static int point_ok(const float* sphere, const float o[3], const float d[3], float t) {
    float w[3], v[3];
    for (int i = 0; i < 3; ++i) w[i] = sphere[i] - o[i];
    for (int i = 0; i < 3; ++i) v[i] = fmaf(t, d[i], -w[i]);
    const float rs = fmaf(4e-7f, sqrtf(dot3(w, w)), sphere[3] * 1.00001f);
    return dot3(v, v) <= rs * rs;
}

/* tri: [F][3][3] corners; normal: [F][3]; rec_of_face: [F]; tiles: [T][4] then [T][16][4], T = ceil(F / 256); origins,
 * directions: [R][3]; poses: NULL or [B][16]; outputs as the entry point's, normal_out / uv_out may be NULL; tests_out: [B][R]
 * exact triangle tests made for the ray (the triangles whose two spheres it passes), or NULL */
void mesh_ray_cull_ref(const float* tri, const float* normal, int32_t F, const int32_t* rec_of_face, const float* tiles,
                       const float* origins, const float* directions, int64_t R, const float* poses, int32_t B, float t_min,
                       float t_max, float* t_out, int32_t* face_out, float* normal_out, float* uv_out, int32_t* tests_out) {
    const int64_t T = ((int64_t)F + TILE - 1) / TILE;
    for (int32_t b = 0; b < B; ++b) {
        const float* M = poses ? poses + 16 * (int64_t)b : 0;
        for (int64_t r = 0; r < R; ++r) {
            float o[3], d[3];
            for (int i = 0; i < 3; ++i) {
                o[i] = origins[3 * r + i];
                d[i] = directions[3 * r + i];
            }
            if (M) {
                float po[3], pd[3];
                for (int i = 0; i < 3; ++i) {
                    const float* row = M + 4 * i;
                    po[i] = fmaf(row[2], o[2], fmaf(row[1], o[1], row[0] * o[0])) + row[3];
                    pd[i] = fmaf(row[2], d[2], fmaf(row[1], d[1], row[0] * d[0]));
                }
                for (int i = 0; i < 3; ++i) {
                    o[i] = po[i];
                    d[i] = pd[i];
                }
            }
            const float dd = dot3(d, d);
            const float len = sqrtf(dd);
            int found = 0;
            int32_t face = -1, tests = 0;
            float t_best = INFINITY, u_best = 0.f, v_best = 0.f;
            for (int32_t f = 0; f < F; ++f) {
                const int32_t j = rec_of_face[f];
                const float* tile = tiles + 4 * (int64_t)(j / TILE);
                const float* group = tiles + 4 * T + 4 * (int64_t)(j / GROUP);
                if (!sphere_ok(tile, o, d, dd, len, t_min, t_max)) continue;
                if (!sphere_ok(group, o, d, dd, len, t_min, t_max)) continue;
                ++tests;
                const float *v0 = tri + 9 * (int64_t)f, *v1 = v0 + 3, *v2 = v0 + 6;
                float e1[3], e2[3], Ng[3], C[3], Rv[3];
                for (int i = 0; i < 3; ++i) {
                    e1[i] = v0[i] - v1[i];
                    e2[i] = v2[i] - v0[i];
                    C[i] = v0[i] - o[i];
                }
                cross3(e2, e1, Ng);
                cross3(C, d, Rv);
                const float den = dot3(Ng, d);
                const float absden = fabsf(den);
                const float sgn = den < 0.f ? -1.f : 1.f;
                const float U = dot3(Rv, e2) * sgn;
                const float V = dot3(Rv, e1) * sgn;
                const float Tn = dot3(Ng, C) * sgn;
                if (!(den != 0.f && U >= 0.f && V >= 0.f && U + V <= absden)) continue;
                const float t = Tn / absden;
                if (!(t >= t_min && t <= t_max)) continue;
                if (!(point_ok(tile, o, d, t) && point_ok(group, o, d, t))) continue;
                /* faces come in ascending id: a later one wins only with a strictly smaller t */
                if (!found || t < t_best) {
                    found = 1;
                    face = f;
                    t_best = t;
                    u_best = U / absden;
                    v_best = V / absden;
                }
            }
            const int64_t at = (int64_t)b * R + r;
            t_out[at] = found ? t_best : INFINITY;
            face_out[at] = face;
            if (tests_out) tests_out[at] = tests;
            if (uv_out) {
                uv_out[2 * at] = u_best;
                uv_out[2 * at + 1] = v_best;
            }
            if (normal_out) {
                float n[3] = {0.f, 0.f, 0.f};
                if (found) {
                    const float* k = normal + 3 * (int64_t)face;
                    for (int j = 0; j < 3; ++j) n[j] = M ? fmaf(M[8 + j], k[2], fmaf(M[4 + j], k[1], M[j] * k[0])) : k[j];
                }
                for (int j = 0; j < 3; ++j) normal_out[3 * at + j] = n[j] + 0.f;
            }
        }
    }
}
