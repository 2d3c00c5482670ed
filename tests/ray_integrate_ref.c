/* Restatement of include/pvamd.h "Ray integration" -- TEST INFRASTRUCTURE, compiled on the fly with -O2 -ffp-contract=off
 * (tests/ray_integrate_ref.py).  One ray after the other, one operation per statement, in the order the header numbers them. */
#include <math.h>
#include <stdint.h>

#define MARK_FREE 1
#define MARK_HIT 2
#define RULE_VALID_ON_INDEX 1
#define RULE_ROUND_HALF_AWAY 2
#define RULE_ROUND_FLOOR_HALF 4

typedef struct {
    double dmin[3], dmax[3], dres[3];
    float fmin[3], fmax[3], fres[3];
    int32_t shape[3];
    int32_t index_f64, rule;
} lattice_t;

static int finite_ray(const float* o, const float* e) {
    for (int k = 0; k < 3; ++k)
        if (!isfinite(o[k]) || !isfinite(e[k])) return 0;
    return 1;
}

/* statement 5 */
static float ray_length(const float* o, const float* e) {
    const float vx = e[0] - o[0], vy = e[1] - o[1], vz = e[2] - o[2];
    const float xx = vx * vx, yy = vy * vy, zz = vz * vz;
    const float xy = xx + yy;
    return sqrtf(xy + zz);
}

/* statement 3: the index statements of the voxel containers; 1 and *flat when e passes the range test */
static int hit_voxel(const lattice_t* g, const float* e, int64_t* flat) {
    int valid = 1;
    int64_t f = 0;
    for (int k = 0; k < 3; ++k) {
        double kq;
        if (g->index_f64) {
            const double q = ((double)e[k] - g->dmin[k]) / g->dres[k];
            kq = (g->rule & RULE_ROUND_HALF_AWAY) ? round(q) : (g->rule & RULE_ROUND_FLOOR_HALF) ? floor(q + 0.5) : rint(q);
        } else {
            const float num = e[k] - g->fmin[k];
            const float q = num / g->fres[k];
            float r;
            if (g->rule & RULE_ROUND_HALF_AWAY) r = roundf(q);
            else if (g->rule & RULE_ROUND_FLOOR_HALF) { const float h = q + 0.5f; r = floorf(h); }
            else r = rintf(q);
            kq = (double)r;
        }
        if (g->rule & RULE_VALID_ON_INDEX) valid &= (kq >= 0.0) && (kq <= (double)(g->shape[k] - 1));
        else if (g->index_f64) valid &= (g->dmin[k] <= (double)e[k]) && ((double)e[k] <= g->dmax[k]);
        else valid &= (g->fmin[k] <= e[k]) && (e[k] <= g->fmax[k]);
        if (!valid) return 0;
        f = f * g->shape[k] + (int64_t)kq;
    }
    *flat = f;
    return 1;
}

static float exit_of(int c, int step, float a, float d) {
    if (step == 0) return INFINITY;
    const float half = 0.5f * (float)step;
    const float face = (float)c + half;
    const float num = face - a;
    return num / d;
}

/* statement 6 for one ray: the cells of its walk, in order, as flat indices into cells[] (room for nx + ny + nz); returns how many */
int32_t ray_walk_ref(const lattice_t* g, const float* o, const float* e, float max_range, int64_t* cells) {
    if (!finite_ray(o, e)) return 0;
    const float len = ray_length(o, e);
    float t0 = 0.0f, t1 = len > max_range ? max_range / len : 1.0f;
    float a[3], d[3];
    for (int k = 0; k < 3; ++k) {
        const float on = o[k] - g->fmin[k], en = e[k] - g->fmin[k];
        a[k] = on / g->fres[k];
        const float b = en / g->fres[k];
        d[k] = b - a[k];
    }
    for (int k = 0; k < 3; ++k)
        if (!isfinite(d[k])) return 0;
    for (int k = 0; k < 3; ++k) {
        const float top = (float)g->shape[k] - 0.5f;
        if (d[k] == 0.0f) {
            if (!(-0.5f <= a[k] && a[k] < top)) return 0;
        } else {
            const float un = -0.5f - a[k], wn = top - a[k];
            const float u = un / d[k], w = wn / d[k];
            t0 = fmaxf(t0, fminf(u, w));
            t1 = fminf(t1, fmaxf(u, w));
        }
    }
    if (!(t0 <= t1)) return 0;
    int c[3], step[3];
    float tmax[3];
    for (int k = 0; k < 3; ++k) {
        const float along = t0 * d[k];
        const float at = a[k] + along;
        const float shifted = at + 0.5f;
        c[k] = (int)fminf(fmaxf(floorf(shifted), 0.0f), (float)(g->shape[k] - 1));
        step[k] = d[k] > 0.0f ? 1 : (d[k] < 0.0f ? -1 : 0);
        tmax[k] = exit_of(c[k], step[k], a[k], d[k]);
    }
    const int budget = g->shape[0] + g->shape[1] + g->shape[2];
    int32_t count = 0;
    for (int visit = 0; visit < budget; ++visit) {
        cells[count++] = ((int64_t)c[0] * g->shape[1] + c[1]) * g->shape[2] + c[2];
        int k = 0;
        if (tmax[1] < tmax[k]) k = 1;
        if (tmax[2] < tmax[k]) k = 2;
        if (!(tmax[k] < t1)) break;
        c[k] += step[k];
        if (c[k] < 0 || c[k] >= g->shape[k]) break;
        tmax[k] = exit_of(c[k], step[k], a[k], d[k]);
    }
    return count;
}

/* statements 1 and 3 to 7 for one scan: origins [1][3] when shared, else [R][3]; marks accumulate as the header says */
void ray_mark_ref(const lattice_t* g, const float* origins, int32_t shared, const float* endpoints, int64_t R, float max_range,
                  uint8_t* marks, int64_t* cells) {
    for (int64_t i = 0; i < R; ++i) {
        const int32_t count = ray_walk_ref(g, shared ? origins : origins + 3 * i, endpoints + 3 * i, max_range, cells);
        for (int32_t j = 0; j < count; ++j)
            if (marks[cells[j]] == 0) marks[cells[j]] = MARK_FREE;
    }
    for (int64_t i = 0; i < R; ++i) {
        const float* o = shared ? origins : origins + 3 * i;
        const float* e = endpoints + 3 * i;
        int64_t flat;
        if (!finite_ray(o, e) || ray_length(o, e) > max_range) continue;
        if (hit_voxel(g, e, &flat)) marks[flat] = MARK_HIT;
    }
}

/* statement 8 */
void occupancy_update_ref(uint8_t* marks, int64_t n, float l_hit, float l_miss, float l_min, float l_max, float* log_odds,
                          uint8_t* observed) {
    for (int64_t i = 0; i < n; ++i) {
        if (marks[i] == 0) continue;
        const float moved = log_odds[i] + (marks[i] == MARK_HIT ? l_hit : l_miss);
        log_odds[i] = fminf(fmaxf(moved, l_min), l_max);
        observed[i] = 1;
        marks[i] = 0;
    }
}
