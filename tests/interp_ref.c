/* CPU restatement of the trilinear arithmetic contract (include/pvamd.h "Interpolated queries", items 2-5) for in-range
 * points -- TEST INFRASTRUCTURE.  Compiled by the tests with gcc -O2 -ffp-contract=off -shared -fPIC ... -lm, so every
 * operation rounds as written; fmaf / fma are explicit.  The range decision (item 1) is the nearest mode's and is taken from
 * the nearest kernel's out_oob by the tests: points with valid[p] == 0 are left untouched here.
 *
 * rec: [n][4] float (val, gx, gy, gz), C order over shape[3].  mn / res: the query dtype's (fmin / fres for float32 points,
 * dmin / dres for float64).  Forward: val[P], grad[P][3].  VJP: dpts[P][3] for upstream dval[P] and dgrad[P][3].
 * interp_cell_* / interp_blend_*: the forward split in two -- its cell decisions (index triple, fractions, clamped flags) and
 * its lerp sequence for given decisions -- for the decision-conditioned VJP (oracle/conditioned_vjp.py, trilinear mode). */
#include <math.h>
#include <stdint.h>

#define CELL(T, FLOOR, SUB, DIV)                                                                  \
    for (int d = 0; d < 3; ++d) {                                                                 \
        const T s = DIV(SUB(x[d], mn[d]), res[d]);                                                \
        const T top = (T)(shape[d] - 1);                                                          \
        const T c = s < (T)0 ? (T)0 : (s > top ? top : s);                                       \
        cl[d] = c != s;                                                                           \
        int k = (int)FLOOR(c);                                                                    \
        if (k > shape[d] - 2) k = shape[d] - 2;                                                   \
        if (k < 0) k = 0;                                                                         \
        i[d] = k;                                                                                 \
        f[d] = SUB(c, (T)k);                                                                      \
    }

static float subf_(float a, float b) { return a - b; }
static float divf_(float a, float b) { return a / b; }
static double sub_(double a, double b) { return a - b; }
static double div_(double a, double b) { return a / b; }

static void corners(const float* rec, const int32_t shape[3], const int i[3], const float* r[8]) {
    const int64_t sy = shape[2], sx = (int64_t)shape[1] * shape[2];
    const int64_t base = ((int64_t)i[0] * shape[1] + i[1]) * shape[2] + i[2];
    const int64_t off[8] = {0, 1, sy, sy + 1, sx, sx + 1, sx + sy, sx + sy + 1};
    for (int c = 0; c < 8; ++c) r[c] = rec + 4 * (base + off[c]);
}

static float lerpf_(float a, float b, float f) { return fmaf(f, b - a, a); }
static double lerp_(double a, double b, double f) { return fma(f, b - a, a); }

void interp_forward_f32(const float* rec, const int32_t* shape, const float* mn, const float* res, const float* pts, int64_t P,
                        const uint8_t* valid, float* val, float* grad) {
    for (int64_t p = 0; p < P; ++p) {
        if (!valid[p]) continue;
        const float* x = pts + 3 * p;
        int i[3], cl[3];
        float f[3];
        CELL(float, floorf, subf_, divf_)
        (void)cl;
        const float* r[8];
        corners(rec, shape, i, r);
        float o[4];
        for (int q = 0; q < 4; ++q) {
            float e[4];
            for (int ab = 0; ab < 4; ++ab) e[ab] = lerpf_(r[2 * ab][q], r[2 * ab + 1][q], f[2]);
            o[q] = lerpf_(lerpf_(e[0], e[1], f[1]), lerpf_(e[2], e[3], f[1]), f[0]);
        }
        val[p] = o[0];
        for (int d = 0; d < 3; ++d) grad[3 * p + d] = o[1 + d];
    }
}

void interp_forward_f64(const float* rec, const int32_t* shape, const double* mn, const double* res, const double* pts, int64_t P,
                        const uint8_t* valid, double* val, double* grad) {
    for (int64_t p = 0; p < P; ++p) {
        if (!valid[p]) continue;
        const double* x = pts + 3 * p;
        int i[3], cl[3];
        double f[3];
        CELL(double, floor, sub_, div_)
        (void)cl;
        const float* r[8];
        corners(rec, shape, i, r);
        double o[4];
        for (int q = 0; q < 4; ++q) {
            double e[4];
            for (int ab = 0; ab < 4; ++ab) e[ab] = lerp_((double)r[2 * ab][q], (double)r[2 * ab + 1][q], f[2]);
            o[q] = lerp_(lerp_(e[0], e[1], f[1]), lerp_(e[2], e[3], f[1]), f[0]);
        }
        val[p] = o[0];
        for (int d = 0; d < 3; ++d) grad[3 * p + d] = o[1 + d];
    }
}

/* The cell decisions alone, by the forward's own CELL statements: per point the corner index triple idx[P][3], the fractions
 * frac[P][3] in the query dtype and clamped[P][3] (0 / 1).  Every point is evaluated (the range decision is the caller's). */
void interp_cell_f32(const int32_t* shape, const float* mn, const float* res, const float* pts, int64_t P, int32_t* idx,
                     float* frac, uint8_t* clamped) {
    for (int64_t p = 0; p < P; ++p) {
        const float* x = pts + 3 * p;
        int i[3], cl[3];
        float f[3];
        CELL(float, floorf, subf_, divf_)
        for (int d = 0; d < 3; ++d) {
            idx[3 * p + d] = i[d];
            frac[3 * p + d] = f[d];
            clamped[3 * p + d] = (uint8_t)cl[d];
        }
    }
}

void interp_cell_f64(const int32_t* shape, const double* mn, const double* res, const double* pts, int64_t P, int32_t* idx,
                     double* frac, uint8_t* clamped) {
    for (int64_t p = 0; p < P; ++p) {
        const double* x = pts + 3 * p;
        int i[3], cl[3];
        double f[3];
        CELL(double, floor, sub_, div_)
        for (int d = 0; d < 3; ++d) {
            idx[3 * p + d] = i[d];
            frac[3 * p + d] = f[d];
            clamped[3 * p + d] = (uint8_t)cl[d];
        }
    }
}

/* The forward's blend of the eight corner records for GIVEN cell decisions (idx, frac as interp_cell_* returns them): the lerp
 * sequence of interp_forward_*, so that cell + blend is the forward bit for bit. */
void interp_blend_f32(const float* rec, const int32_t* shape, const int32_t* idx, const float* frac, int64_t P, float* val,
                      float* grad) {
    for (int64_t p = 0; p < P; ++p) {
        const int i[3] = {idx[3 * p], idx[3 * p + 1], idx[3 * p + 2]};
        const float* f = frac + 3 * p;
        const float* r[8];
        corners(rec, shape, i, r);
        float o[4];
        for (int q = 0; q < 4; ++q) {
            float e[4];
            for (int ab = 0; ab < 4; ++ab) e[ab] = lerpf_(r[2 * ab][q], r[2 * ab + 1][q], f[2]);
            o[q] = lerpf_(lerpf_(e[0], e[1], f[1]), lerpf_(e[2], e[3], f[1]), f[0]);
        }
        val[p] = o[0];
        for (int d = 0; d < 3; ++d) grad[3 * p + d] = o[1 + d];
    }
}

void interp_blend_f64(const float* rec, const int32_t* shape, const int32_t* idx, const double* frac, int64_t P, double* val,
                      double* grad) {
    for (int64_t p = 0; p < P; ++p) {
        const int i[3] = {idx[3 * p], idx[3 * p + 1], idx[3 * p + 2]};
        const double* f = frac + 3 * p;
        const float* r[8];
        corners(rec, shape, i, r);
        double o[4];
        for (int q = 0; q < 4; ++q) {
            double e[4];
            for (int ab = 0; ab < 4; ++ab) e[ab] = lerp_((double)r[2 * ab][q], (double)r[2 * ab + 1][q], f[2]);
            o[q] = lerp_(lerp_(e[0], e[1], f[1]), lerp_(e[2], e[3], f[1]), f[0]);
        }
        val[p] = o[0];
        for (int d = 0; d < 3; ++d) grad[3 * p + d] = o[1 + d];
    }
}

/* per-point VJP in float64 (item 5): dx_d = sum_q u_q d out_q / d f_d / res_d, 0 on a clamped axis.  pts / mn / res in float64
 * (float32 queries pass their points, fmin and fres widened: the decisions are then the float32 ones for stable points) */
void interp_vjp_f64(const float* rec, const int32_t* shape, const double* mn, const double* res, const double* pts, int64_t P,
                    const uint8_t* valid, const double* dval, const double* dgrad, double* dpts) {
    for (int64_t p = 0; p < P; ++p) {
        if (!valid[p]) continue;
        const double* x = pts + 3 * p;
        int i[3], cl[3];
        double f[3];
        CELL(double, floor, sub_, div_)
        const float* r[8];
        corners(rec, shape, i, r);
        double df[3] = {0, 0, 0};
        for (int q = 0; q < 4; ++q) {
            const double u = q == 0 ? dval[p] : dgrad[3 * p + q - 1];
            double e[4], de[4];
            for (int ab = 0; ab < 4; ++ab) {
                const double a = r[2 * ab][q], b = r[2 * ab + 1][q];
                e[ab] = lerp_(a, b, f[2]);
                de[ab] = b - a;
            }
            const double y0 = lerp_(e[0], e[1], f[1]), y1 = lerp_(e[2], e[3], f[1]);
            df[0] += u * (y1 - y0);
            df[1] += u * ((1 - f[0]) * (e[1] - e[0]) + f[0] * (e[3] - e[2]));
            df[2] += u * ((1 - f[0]) * ((1 - f[1]) * de[0] + f[1] * de[1]) + f[0] * ((1 - f[1]) * de[2] + f[1] * de[3]));
        }
        for (int d = 0; d < 3; ++d) dpts[3 * p + d] = cl[d] ? 0.0 : df[d] / res[d];
    }
}

/* ComposedSDF over trilinear BOUNDING_BOX leaves (item 6), float32 points, rule 0 or any rule through vlo / vhi: per leaf s the
 * kernels' transform statement x = ((m0 px + m1 py) + m2 pz) + m3 as fmaf, the range test vlo <= x <= vhi, in range the
 * interpolation, outside the bounding-box statements; first minimum (NaN counts as the minimum, +inf initial value with a NaN
 * gradient at leaf 0); the winner's gradient rotated back with fmaf(M8, gz, fmaf(M4, gy, M0 gx)).
 * recs[s]: leaf s's records; shapes / mns / ress / vlos / vhis / bbs: [S][3] ([S][6] for bbs: min xyz, max xyz); tf [S*A][16]. */
void composed_forward_f32(int32_t S, const float* const* recs, const int32_t* shapes, const float* mns, const float* ress,
                          const float* vlos, const float* vhis, const float* bbs, const float* tf, int32_t A, const float* pts,
                          int64_t P, float* val, float* grad, int32_t* leaf) {
    for (int a = 0; a < A; ++a)
        for (int64_t p = 0; p < P; ++p) {
            const float px = pts[3 * p], py = pts[3 * p + 1], pz = pts[3 * p + 2];
            float bv = INFINITY, bg[3] = {NAN, NAN, NAN};
            int bs = 0;
            for (int s = 0; s < S; ++s) {
                const float* M = tf + 16 * ((int64_t)s * A + a);
                float x[3];
                for (int r = 0; r < 3; ++r) x[r] = fmaf(M[4 * r + 2], pz, fmaf(M[4 * r + 1], py, M[4 * r] * px)) + M[4 * r + 3];
                int in = 1;
                for (int d = 0; d < 3; ++d) in &= (vlos[3 * s + d] <= x[d]) & (x[d] <= vhis[3 * s + d]);
                float o[4];
                if (in) {
                    uint8_t one = 1;
                    interp_forward_f32(recs[s], shapes + 3 * s, mns + 3 * s, ress + 3 * s, x, 1, &one, o, o + 1);
                } else {
                    float t[3];
                    for (int d = 0; d < 3; ++d) {
                        float lo = bbs[6 * s + d] - x[d];
                        const int la = lo > 0.f;
                        lo = la ? lo : 0.f;
                        float hi = x[d] - bbs[6 * s + 3 + d];
                        hi = hi > 0.f ? hi : 0.f;
                        const float sm = lo + hi;
                        t[d] = la ? -sm : sm;
                    }
                    const float n = sqrtf(fmaf(t[2], t[2], fmaf(t[1], t[1], t[0] * t[0])));
                    o[0] = n;
                    for (int d = 0; d < 3; ++d) o[1 + d] = t[d] / n;
                }
                const int take = !(o[0] >= bv) && (bv == bv);
                if (take) {
                    bv = o[0];
                    bg[0] = o[1]; bg[1] = o[2]; bg[2] = o[3];
                    bs = s;
                }
            }
            const float* M = tf + 16 * ((int64_t)bs * A + a);
            const int64_t o = (int64_t)a * P + p;
            val[o] = bv;
            for (int j = 0; j < 3; ++j) grad[3 * o + j] = fmaf(M[8 + j], bg[2], fmaf(M[4 + j], bg[1], M[j] * bg[0]));
            leaf[o] = bs;
        }
}

/* The same composition in float64 (float64 points and stack, default index rule): per leaf s x = ((m0 px + m1 py) + m2 pz) + m3 as
 * fma, the nearest mode's float64 range test dmin <= x <= dmax, in range the interpolation, outside the bounding-box statements
 * in float64; the first minimum from the first leaf on (NaN counts as the minimum); the winner's gradient rotated back with
 * fma(M8, gz, fma(M4, gy, M0 gx)).  mns / ress / dmins / dmaxs / bbs: the descriptors' dmin / dres / dmin / dmax / dbb_min,
 * dbb_max, in the layouts of composed_forward_f32. */
void composed_forward_f64(int32_t S, const float* const* recs, const int32_t* shapes, const double* mns, const double* ress,
                          const double* dmins, const double* dmaxs, const double* bbs, const double* tf, int32_t A,
                          const double* pts, int64_t P, double* val, double* grad, int32_t* leaf) {
    for (int a = 0; a < A; ++a)
        for (int64_t p = 0; p < P; ++p) {
            const double* q = pts + 3 * p;
            double bv = 0.0, bg[3] = {0.0, 0.0, 0.0};
            int bs = -1;
            for (int s = 0; s < S; ++s) {
                const double* M = tf + 16 * ((int64_t)s * A + a);
                double x[3];
                for (int r = 0; r < 3; ++r) x[r] = fma(M[4 * r + 2], q[2], fma(M[4 * r + 1], q[1], M[4 * r] * q[0])) + M[4 * r + 3];
                int in = 1;
                for (int d = 0; d < 3; ++d) in &= (dmins[3 * s + d] <= x[d]) & (x[d] <= dmaxs[3 * s + d]);
                double o[4];
                if (in) {
                    uint8_t one = 1;
                    interp_forward_f64(recs[s], shapes + 3 * s, mns + 3 * s, ress + 3 * s, x, 1, &one, o, o + 1);
                } else {
                    double t[3];
                    for (int d = 0; d < 3; ++d) {
                        double lo = bbs[6 * s + d] - x[d];
                        const int la = lo > 0.0;
                        lo = la ? lo : 0.0;
                        double hi = x[d] - bbs[6 * s + 3 + d];
                        hi = hi > 0.0 ? hi : 0.0;
                        const double sm = lo + hi;
                        t[d] = la ? -sm : sm;
                    }
                    const double n = sqrt(fma(t[2], t[2], fma(t[1], t[1], t[0] * t[0])));
                    o[0] = n;
                    for (int d = 0; d < 3; ++d) o[1 + d] = t[d] / n;
                }
                if (bs < 0 || o[0] < bv || (o[0] != o[0] && bv == bv)) {
                    bv = o[0];
                    bg[0] = o[1]; bg[1] = o[2]; bg[2] = o[3];
                    bs = s;
                }
            }
            const double* M = tf + 16 * ((int64_t)bs * A + a);
            const int64_t o = (int64_t)a * P + p;
            val[o] = bv;
            for (int j = 0; j < 3; ++j) grad[3 * o + j] = fma(M[8 + j], bg[2], fma(M[4 + j], bg[1], M[j] * bg[0]));
            leaf[o] = bs;
        }
}
