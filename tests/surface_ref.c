/* Restatement of include/pvamd.h "Surface extraction" in plain C for the tests -- TEST INFRASTRUCTURE.  Statement numbers are the
 * header's.  Compiled by tests/surface_ref.py with -O2 -ffp-contract=off: every float operation below is rounded on its own.
 * One function does both jobs: it always reports the counts, and writes the rows below the capacities it is given. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* 1. */
static float sample(const float* records, float level, int64_t i) { return records[4 * i] - level; }

static int usable(const float* records, const uint8_t* valid, float level, int64_t i) {
    return isfinite(sample(records, level, i)) && (!valid || valid[i] != 0);
}

/* 2. for the edge from voxel a along an axis whose flat step is `step` */
static int crossing(const float* records, const uint8_t* valid, float level, int64_t a, int64_t step, float* f) {
    if (!usable(records, valid, level, a) || !usable(records, valid, level, a + step)) return 0;
    const float wa = sample(records, level, a), wb = sample(records, level, a + step);
    if ((wa < 0.0f) == (wb < 0.0f)) return 0;
    *f = wa / (wa - wb);
    return 1;
}

/* 3. for the cell whose lowest corner is voxel c = (x, y, z) */
static int active(const float* records, const uint8_t* valid, float level, const int n[3], const int64_t step[3], int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x > n[0] - 2 || y > n[1] - 2 || z > n[2] - 2) return 0;
    int negative = 0;
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy)
            for (int dz = 0; dz < 2; ++dz) {
                const int64_t i = (x + dx) * step[0] + (y + dy) * step[1] + (z + dz) * step[2];
                if (!usable(records, valid, level, i)) return 0;
                negative += sample(records, level, i) < 0.0f;
            }
    return negative > 0 && negative < 8;
}

/* counts[0..1] = (vertices, triangles); ids: [n] int32 scratch of the caller's, the vertex id of every cell (by the flat index of
 * its lowest corner), -1 without one.  fmin, fres: the lattice.  normals may be NULL. */
void surface_ref(const float* records, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, const float* fmin, const float* fres,
                 float level, int64_t max_vertices, int64_t max_faces, float* vertices, float* normals, int32_t* faces, int32_t* ids,
                 int64_t* counts) {
    const int n[3] = {nx, ny, nz};
    const int64_t step[3] = {(int64_t)ny * nz, nz, 1};
    int64_t nv = 0, nf = 0;
    int c[3];
    /* 4. - 6. */
    for (c[0] = 0; c[0] < nx; ++c[0])
        for (c[1] = 0; c[1] < ny; ++c[1])
            for (c[2] = 0; c[2] < nz; ++c[2]) {
                const int64_t flat = c[0] * step[0] + c[1] * step[1] + c[2] * step[2];
                ids[flat] = -1;
                if (!active(records, valid, level, n, step, c[0], c[1], c[2])) continue;
                const int64_t id = nv++;
                ids[flat] = (int32_t)id;
                if (id >= max_vertices) continue;
                float S[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f};
                int m = 0;
                for (int k = 0; k < 3; ++k) {
                    const int o0 = k == 0 ? 1 : 0, o1 = k == 2 ? 1 : 2; /* the other two axes, ascending */
                    for (int d0 = 0; d0 < 2; ++d0)
                        for (int d1 = 0; d1 < 2; ++d1) {
                            const int64_t a = flat + d0 * step[o0] + d1 * step[o1];
                            float f;
                            if (!crossing(records, valid, level, a, step[k], &f)) continue;
                            float offset[3];
                            offset[k] = f;
                            offset[o0] = (float)d0;
                            offset[o1] = (float)d1;
                            for (int j = 0; j < 3; ++j) S[j] = S[j] + offset[j];
                            ++m;
                            const float* ga = records + 4 * a + 1;
                            const float* gb = records + 4 * (a + step[k]) + 1;
                            for (int j = 0; j < 3; ++j) N[j] = N[j] + (ga[j] + f * (gb[j] - ga[j]));
                        }
                }
                for (int j = 0; j < 3; ++j) {
                    const float p = (float)c[j] + S[j] / (float)m;
                    vertices[3 * id + j] = fmin[j] + p * fres[j];
                }
                if (normals) {
                    const float len = sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
                    const int ok = len > 0.0f && isfinite(len);
                    for (int j = 0; j < 3; ++j) normals[3 * id + j] = ok ? N[j] / len : 0.0f;
                }
            }
    /* 7. */
    int a[3];
    for (a[0] = 0; a[0] < nx; ++a[0])
        for (a[1] = 0; a[1] < ny; ++a[1])
            for (a[2] = 0; a[2] < nz; ++a[2])
                for (int k = 0; k < 3; ++k) {
                    if (a[k] > n[k] - 2) continue;
                    const int64_t flat = a[0] * step[0] + a[1] * step[1] + a[2] * step[2];
                    float f;
                    if (!crossing(records, valid, level, flat, step[k], &f)) continue;
                    const int p = (k + 1) % 3, q = (k + 2) % 3;
                    int cell[4][3];
                    for (int v = 0; v < 4; ++v)
                        for (int j = 0; j < 3; ++j) cell[v][j] = a[j];
                    cell[0][p] -= 1, cell[0][q] -= 1; /* C0 = a - e_p - e_q */
                    cell[1][q] -= 1;                  /* C1 = a - e_q */
                    cell[3][p] -= 1;                  /* C3 = a - e_p; C2 = a */
                    int32_t v[4];
                    int all = 1;
                    for (int w = 0; w < 4; ++w) {
                        all = all && active(records, valid, level, n, step, cell[w][0], cell[w][1], cell[w][2]);
                        if (all) v[w] = ids[cell[w][0] * step[0] + cell[w][1] * step[1] + cell[w][2] * step[2]];
                    }
                    if (!all) continue;
                    if (!(sample(records, level, flat) < 0.0f)) {
                        const int32_t t = v[1];
                        v[1] = v[3];
                        v[3] = t;
                    }
                    const int32_t rows[2][3] = {{v[0], v[1], v[2]}, {v[0], v[2], v[3]}};
                    for (int r = 0; r < 2; ++r, ++nf)
                        if (nf < max_faces)
                            for (int j = 0; j < 3; ++j) faces[3 * nf + j] = rows[r][j];
                }
    counts[0] = nv;
    counts[1] = nf;
}
