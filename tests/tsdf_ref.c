/* Restatement of include/pvamd.h "TSDF integration" in plain C for the tests -- TEST INFRASTRUCTURE.  Statement numbers are the
 * header's.  Compiled by tests/tsdf_ref.py with -O2 -ffp-contract=off: every float operation below is rounded on its own. */
#include <math.h>
#include <stdint.h>

typedef struct {
    float fmin[3], fres[3];
    int32_t shape[3];
} lattice_t;

/* branch counters of the projection statements, for tests that must know which branches their inputs reach */
enum { HIT_BEHIND, HIT_U_LOW_EDGE, HIT_U_HIGH_EDGE, HIT_U_HALF, HIT_COL_CLAMPED, HIT_NO_RETURN, HIT_TOO_FAR, HIT_BAND_EDGE,
       HIT_BEHIND_BAND, HIT_SATURATED_EDGE, HIT_UPDATED, HIT_OUTSIDE, HIT_COUNT };

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

void tsdf_integrate_ref(const lattice_t* L, const float* depth, int32_t K, int32_t H, int32_t W, const float* camera_from_volume,
                        float fx, float fy, float cx, float cy, float truncation, float max_depth, float weight, float max_weight,
                        float* state, int64_t* hits) {
    const int nx = L->shape[0], ny = L->shape[1], nz = L->shape[2];
    const float u_end = (float)W - 0.5f, v_end = (float)H - 0.5f;
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y)
            for (int z = 0; z < nz; ++z) {
                const int64_t i = ((int64_t)x * ny + y) * nz + z;
                /* 2. */
                const float c0 = L->fmin[0] + (float)x * L->fres[0];
                const float c1 = L->fmin[1] + (float)y * L->fres[1];
                const float c2 = L->fmin[2] + (float)z * L->fres[2];
                float F = state[2 * i], Wt = state[2 * i + 1]; /* 1.: read once */
                int touched = 0;
                for (int k = 0; k < K; ++k) {
                    const float* T = camera_from_volume + 12 * (int64_t)k;
                    /* 3. */
                    const float px = ((T[0] * c0 + T[1] * c1) + T[2] * c2) + T[3];
                    const float py = ((T[4] * c0 + T[5] * c1) + T[6] * c2) + T[7];
                    const float pz = ((T[8] * c0 + T[9] * c1) + T[10] * c2) + T[11];
                    if (!(pz > 0.0f)) { hits[HIT_BEHIND]++; continue; }
                    /* 4. */
                    const float u = fx * (px / pz) + cx;
                    const float v = fy * (py / pz) + cy;
                    if (!(u >= -0.5f && u < u_end && v >= -0.5f && v < v_end)) {
                        hits[HIT_OUTSIDE]++;
                        if (u == u_end) hits[HIT_U_HIGH_EDGE]++;
                        continue;
                    }
                    if (u == -0.5f) hits[HIT_U_LOW_EDGE]++;
                    if (u - floorf(u) == 0.5f && u > 0.0f) hits[HIT_U_HALF]++;
                    /* 5. */
                    const int col_raw = (int)floorf(u + 0.5f), row_raw = (int)floorf(v + 0.5f);
                    const int col = clampi(col_raw, 0, W - 1), row = clampi(row_raw, 0, H - 1);
                    if (col != col_raw || row != row_raw) hits[HIT_COL_CLAMPED]++;
                    /* 6. */
                    const float d = depth[((int64_t)k * H + row) * W + col];
                    if (!(d > 0.0f && d < INFINITY)) { hits[HIT_NO_RETURN]++; continue; }
                    if (!(d <= max_depth)) { hits[HIT_TOO_FAR]++; continue; }
                    /* 7. */
                    const float sdf = d - pz;
                    if (!(sdf >= -truncation)) { hits[HIT_BEHIND_BAND]++; continue; }
                    if (sdf == -truncation) hits[HIT_BAND_EDGE]++;
                    if (sdf == truncation) hits[HIT_SATURATED_EDGE]++;
                    /* 8. */
                    const float f = fminf(sdf / truncation, 1.0f);
                    /* 9. */
                    const float Wn = Wt + weight;
                    F = ((Wt * F) + (weight * f)) / Wn;
                    Wt = fminf(Wn, max_weight);
                    touched = 1;
                    hits[HIT_UPDATED]++;
                }
                if (touched) { /* 1.: written once, and only then */
                    state[2 * i] = F;
                    state[2 * i + 1] = Wt;
                }
            }
}

/* 10. */
static float value_at(const float* state, int64_t i, float truncation, float min_weight, float unknown_tsdf) {
    const float t = state[2 * i + 1] > min_weight ? state[2 * i] : unknown_tsdf;
    return truncation * t;
}

/* 11. along one axis */
static float slope(const float* state, int64_t i, int c, int n, int64_t step, float resolution, float truncation, float min_weight,
                   float unknown_tsdf) {
    const int lo = c - 1 > 0 ? c - 1 : 0, hi = c + 1 < n - 1 ? c + 1 : n - 1;
    const float a = value_at(state, i + (hi - c) * step, truncation, min_weight, unknown_tsdf);
    const float b = value_at(state, i + (lo - c) * step, truncation, min_weight, unknown_tsdf);
    return (a - b) / ((float)(hi - lo) * resolution);
}

void tsdf_records_ref(const float* state, int32_t nx, int32_t ny, int32_t nz, float resolution, float truncation, float min_weight,
                      float unknown_tsdf, float* records) {
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y)
            for (int z = 0; z < nz; ++z) {
                const int64_t i = ((int64_t)x * ny + y) * nz + z;
                const float val = value_at(state, i, truncation, min_weight, unknown_tsdf);
                const float gx = slope(state, i, x, nx, (int64_t)ny * nz, resolution, truncation, min_weight, unknown_tsdf);
                const float gy = slope(state, i, y, ny, nz, resolution, truncation, min_weight, unknown_tsdf);
                const float gz = slope(state, i, z, nz, 1, resolution, truncation, min_weight, unknown_tsdf);
                /* 12. */
                const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
                float* r = records + 4 * i;
                r[0] = val;
                if (len > 0.0f) {
                    r[1] = gx / len;
                    r[2] = gy / len;
                    r[3] = gz / len;
                } else {
                    r[1] = r[2] = r[3] = 0.0f;
                }
            }
}
