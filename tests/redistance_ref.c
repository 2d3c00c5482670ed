/* Restatement of include/pvamd.h "Redistancing" in plain C for the tests -- TEST INFRASTRUCTURE.  Statement numbers are the
 * header's.  Compiled by tests/redistance_ref.py with -O2 -ffp-contract=off: every float operation below is rounded on its own.
 * Two forms: the nested separable one, which is the definition (sites included), with whole-line minima and no early exit; and a
 * brute-force minimum of c3 over every crossing of the lattice. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* 3.: the remaining axes of family k, highest index first */
static const int P2[3] = {2, 2, 1}, P3[3] = {1, 0, 0};

/* 2. */
static int crossing(float va, float vb, float* f) {
    if (!isfinite(va) || !isfinite(vb) || (va < 0.0f) == (vb < 0.0f)) return 0;
    *f = va / (va - vb);
    return 1;
}

static float value(const float* records, int64_t i) { return records[4 * i]; }

/* 3. for the crossing on the edge of family k whose lower voxel is a, seen from voxel i */
static float cost3(const float* records, const int64_t step[3], const int i[3], const int a[3], int k, float* t_out) {
    const int64_t flat = a[0] * step[0] + a[1] * step[1] + a[2] * step[2];
    float f = 0.0f;
    crossing(value(records, flat), value(records, flat + step[k]), &f);
    const int p2 = P2[k], p3 = P3[k];
    const float t = (float)(i[k] - a[k]) - f;
    const float c1 = t * t;
    const float c2 = c1 + (float)((i[p2] - a[p2]) * (i[p2] - a[p2]));
    if (t_out) *t_out = t;
    return c2 + (float)((i[p3] - a[p3]) * (i[p3] - a[p3]));
}

/* 4. for one family: cost[i] = c3 of the family's site for voxel i, site[3 * i ..] its lower voxel; site[3 * i] = -1: none */
static void family(const float* records, const int n[3], const int64_t step[3], int k, float* cost, int* site) {
    const int64_t total = (int64_t)n[0] * n[1] * n[2];
    const int p2 = P2[k], p3 = P3[k];
    float* c1 = malloc(sizeof(float) * total);
    float* c2 = malloc(sizeof(float) * total);
    int* a1 = malloc(sizeof(int) * total);     /* a_k after pass 1, -1: the line has no crossing */
    int* a2 = malloc(sizeof(int) * 2 * total); /* (a_k, a_p2) after pass 2 */
    int v[3];
    /* pass 1 */
    for (v[0] = 0; v[0] < n[0]; ++v[0])
        for (v[1] = 0; v[1] < n[1]; ++v[1])
            for (v[2] = 0; v[2] < n[2]; ++v[2]) {
                const int64_t i = v[0] * step[0] + v[1] * step[1] + v[2] * step[2];
                const int64_t line = i - v[k] * step[k];
                c1[i] = INFINITY;
                a1[i] = -1;
                for (int a = 0; a < n[k] - 1; ++a) { /* ascending: a strict < keeps the smaller a_k */
                    float f;
                    if (!crossing(value(records, line + a * step[k]), value(records, line + (a + 1) * step[k]), &f)) continue;
                    const float t = (float)(v[k] - a) - f;
                    const float c = t * t;
                    if (a1[i] < 0 || c < c1[i]) { c1[i] = c; a1[i] = a; }
                }
            }
    /* pass 2 */
    for (v[0] = 0; v[0] < n[0]; ++v[0])
        for (v[1] = 0; v[1] < n[1]; ++v[1])
            for (v[2] = 0; v[2] < n[2]; ++v[2]) {
                const int64_t i = v[0] * step[0] + v[1] * step[1] + v[2] * step[2];
                const int64_t line = i - v[p2] * step[p2];
                c2[i] = INFINITY;
                a2[2 * i] = -1;
                for (int j = 0; j < n[p2]; ++j) {
                    const int64_t w = line + j * step[p2];
                    if (a1[w] < 0) continue;
                    const float c = c1[w] + (float)((v[p2] - j) * (v[p2] - j));
                    if (a2[2 * i] < 0 || c < c2[i]) { c2[i] = c; a2[2 * i] = a1[w]; a2[2 * i + 1] = j; }
                }
            }
    /* pass 3 */
    for (v[0] = 0; v[0] < n[0]; ++v[0])
        for (v[1] = 0; v[1] < n[1]; ++v[1])
            for (v[2] = 0; v[2] < n[2]; ++v[2]) {
                const int64_t i = v[0] * step[0] + v[1] * step[1] + v[2] * step[2];
                const int64_t line = i - v[p3] * step[p3];
                cost[i] = INFINITY;
                site[3 * i] = -1;
                for (int j = 0; j < n[p3]; ++j) {
                    const int64_t w = line + j * step[p3];
                    if (a2[2 * w] < 0) continue;
                    const float c = c2[w] + (float)((v[p3] - j) * (v[p3] - j));
                    if (site[3 * i] < 0 || c < cost[i]) {
                        cost[i] = c;
                        site[3 * i + k] = a2[2 * w];
                        site[3 * i + p2] = a2[2 * w + 1];
                        site[3 * i + p3] = j;
                    }
                }
            }
    free(c1);
    free(c2);
    free(a1);
    free(a2);
}

/* the whole contract: records_out [n][4], sites [n], squared [n].  Returns at how many voxels the nested cost is not, bit for bit,
 * statement 3. evaluated at the site the nesting chose: zero. */
int64_t redistance_ref(const float* records, int32_t nx, int32_t ny, int32_t nz, float resolution, float band, float max_distance,
                    float* records_out, int32_t* sites, float* squared) {
    const int n[3] = {nx, ny, nz};
    const int64_t step[3] = {(int64_t)ny * nz, nz, 1};
    const int64_t total = (int64_t)nx * ny * nz;
    float* cost[3];
    int* site[3];
    for (int k = 0; k < 3; ++k) {
        cost[k] = malloc(sizeof(float) * total);
        site[k] = malloc(sizeof(int) * 3 * total);
        family(records, n, step, k, cost[k], site[k]);
    }
    /* 5. */
    const float Rv = max_distance / resolution;
    const float R2 = Rv * Rv;
    int64_t differ = 0;
    int v[3];
    for (v[0] = 0; v[0] < nx; ++v[0])
        for (v[1] = 0; v[1] < ny; ++v[1])
            for (v[2] = 0; v[2] < nz; ++v[2]) {
                const int64_t i = v[0] * step[0] + v[1] * step[1] + v[2] * step[2];
                const float V = value(records, i);
                float* out = records_out + 4 * i;
                if (fabsf(V) < band) { /* 6. */
                    for (int c = 0; c < 4; ++c) out[c] = records[4 * i + c];
                    sites[i] = -2;
                    squared[i] = INFINITY;
                    continue;
                }
                int k = -1;
                for (int c = 0; c < 3; ++c) /* 4.: the lowest k on a tie */
                    if (site[c][3 * i] >= 0 && (k < 0 || cost[c][i] < cost[k][i])) k = c;
                const int negative = V < 0.0f;
                if (k < 0 || cost[k][i] > R2) { /* 5. */
                    sites[i] = -1;
                    squared[i] = INFINITY;
                    out[0] = negative ? -max_distance : max_distance;
                    out[1] = out[2] = out[3] = 0.0f;
                    continue;
                }
                const int* a = site[k] + 3 * i;
                float t;
                const float c3 = cost3(records, step, v, a, k, &t);
                if (c3 != cost[k][i]) ++differ; /* the nesting adds the terms in the order of 3. */
                sites[i] = (int32_t)((a[0] * step[0] + a[1] * step[1] + a[2] * step[2]) * 4 + k);
                squared[i] = c3;
                /* 7. */
                const float len = sqrtf(c3);
                const float val = resolution * len;
                out[0] = negative ? -val : val;
                for (int j = 0; j < 3; ++j) {
                    float g = 0.0f;
                    if (c3 != 0.0f) {
                        g = (j == k ? t : (float)(v[j] - a[j])) / len;
                        if (negative) g = -g;
                    }
                    out[1 + j] = g;
                }
            }
    for (int k = 0; k < 3; ++k) {
        free(cost[k]);
        free(site[k]);
    }
    return differ;
}

/* min over every crossing of the lattice of c3, +INFINITY without one: O(n * crossings) */
void redistance_brute(const float* records, int32_t nx, int32_t ny, int32_t nz, float* squared) {
    const int n[3] = {nx, ny, nz};
    const int64_t step[3] = {(int64_t)ny * nz, nz, 1};
    int v[3], a[3];
    for (v[0] = 0; v[0] < nx; ++v[0])
        for (v[1] = 0; v[1] < ny; ++v[1])
            for (v[2] = 0; v[2] < nz; ++v[2]) {
                float best = INFINITY;
                for (int k = 0; k < 3; ++k)
                    for (a[0] = 0; a[0] < n[0] - (k == 0); ++a[0])
                        for (a[1] = 0; a[1] < n[1] - (k == 1); ++a[1])
                            for (a[2] = 0; a[2] < n[2] - (k == 2); ++a[2]) {
                                const int64_t flat = a[0] * step[0] + a[1] * step[1] + a[2] * step[2];
                                float f;
                                if (!crossing(value(records, flat), value(records, flat + step[k]), &f)) continue;
                                const float c = cost3(records, step, v, a, k, 0);
                                if (c < best) best = c;
                            }
                squared[v[0] * step[0] + v[1] * step[1] + v[2] * step[2]] = best;
            }
}

/* c3 of the crossing that sites[i] names, from voxel i; +INFINITY where sites[i] < 0 or the edge carries no crossing */
void redistance_site_costs(const float* records, int32_t nx, int32_t ny, int32_t nz, const int32_t* sites, float* out) {
    const int64_t step[3] = {(int64_t)ny * nz, nz, 1};
    int v[3];
    for (v[0] = 0; v[0] < nx; ++v[0])
        for (v[1] = 0; v[1] < ny; ++v[1])
            for (v[2] = 0; v[2] < nz; ++v[2]) {
                const int64_t i = v[0] * step[0] + v[1] * step[1] + v[2] * step[2];
                out[i] = INFINITY;
                if (sites[i] < 0) continue;
                const int k = sites[i] & 3;
                const int64_t flat = sites[i] >> 2;
                const int a[3] = {(int)(flat / step[0]), (int)(flat % step[0] / step[1]), (int)(flat % step[1])};
                float f;
                if (k > 2 || a[k] >= (k == 0 ? nx : (k == 1 ? ny : nz)) - 1) continue;
                if (!crossing(value(records, flat), value(records, flat + step[k]), &f)) continue;
                out[i] = cost3(records, step, v, a, k, 0);
            }
}
