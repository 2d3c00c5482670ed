// Trilinear interpolation of the packed (val, gx, gy, gz) records: the per-leaf statements shared by the interpolated
// forward kernels (lane_query.hip, min_over_points.hip) and their backward (backward.hip); and leaf_f64, the float64 leaf of
// both modes.  The arithmetic contract is include/pvamd.h's
// "Interpolated queries"; tests/interp_ref.c states the same sequence on the CPU.
//   per axis d:  s = (x_d - min_d) / res_d                   IEEE subtraction, then IEEE division, in the query dtype
//                c = s < 0 ? 0 : (s > n_d - 1 ? n_d - 1 : s)  clamped_d = (c != s)
//                i_d = min(floor(c), n_d - 2),  f_d = c - i_d (exact)
//   lerp(a, b, f) = fma(f, b - a, a); z-lerps first (corners (0,0), (0,1), (1,0), (1,1) in (x, y)), then y, then x.
// The range decision is the nearest mode's (in_range / voxel_key_f64, grid_lookup.h): these run for in-range points only.
#pragma once
#include "grid_lookup.h"

namespace pvamd {

template <typename T> struct InterpCell {
    int base;      // flat index of corner (i, j, k)
    T f[3];        // fractions
    bool cl[3];    // the coordinate was clamped: no derivative along that axis
};

template <typename T> PVAMD_DEV T interp_lerp(T a, T b, T f);
template <> PVAMD_DEV float interp_lerp<float>(float a, float b, float f) { return fmaf(f, sub_rn(b, a), a); }
template <> PVAMD_DEV double interp_lerp<double>(double a, double b, double f) { return __builtin_fma(f, b - a, a); }

template <typename T>
PVAMD_DEV void interp_cell(const pvamd_grid_t& g, const T x[3], InterpCell<T>& c) {
    int i[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        T s;
        if constexpr (sizeof(T) == 8) s = (x[d] - g.dmin[d]) / g.dres[d];
        else s = div_rn(sub_rn(x[d], g.fmin[d]), g.fres[d]);
        const T top = (T)(g.shape[d] - 1);
        const T cc = s < T(0) ? T(0) : (s > top ? top : s);
        c.cl[d] = cc != s;
        T fl;
        if constexpr (sizeof(T) == 8) fl = __builtin_floor(cc);
        else fl = __builtin_floorf(cc);
        int k = (int)fl;
        k = k < g.shape[d] - 2 ? k : g.shape[d] - 2;
        k = k > 0 ? k : 0;  // a no-op for finite in-range points; keeps the gathers in bounds regardless
        i[d] = k;
        if constexpr (sizeof(T) == 8) c.f[d] = cc - (T)k;
        else c.f[d] = sub_rn(cc, (float)k);
    }
    c.base = (i[0] * g.shape[1] + i[1]) * g.shape[2] + i[2];
}

// The eight corner records, all loads issued before the first use: r[2 * (2a + b) + e] = R[i+a, j+b, k+e].  In C order the
// pair (k, k+1) is 32 contiguous bytes, so a point reads four 32-byte segments.
PVAMD_DEV void interp_gather(const pvamd_grid_t& g, int base, float4 r[8]) {
    const int sy = g.shape[2], sx = g.shape[1] * g.shape[2];
    r[0] = load_record(g.vox, base);
    r[1] = load_record(g.vox, base + 1);
    r[2] = load_record(g.vox, base + sy);
    r[3] = load_record(g.vox, base + sy + 1);
    r[4] = load_record(g.vox, base + sx);
    r[5] = load_record(g.vox, base + sx + 1);
    r[6] = load_record(g.vox, base + sx + sy);
    r[7] = load_record(g.vox, base + sx + sy + 1);
}

PVAMD_DEV float rec_ch(const float4& r, int q) { return q == 0 ? r.x : (q == 1 ? r.y : (q == 2 ? r.z : r.w)); }

// out[q] for the four channels (val, gx, gy, gz)
template <typename T>
PVAMD_DEV void interp_combine(const float4 r[8], const T f[3], T out[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        T e[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) e[ab] = interp_lerp<T>((T)rec_ch(r[2 * ab], q), (T)rec_ch(r[2 * ab + 1], q), f[2]);
        const T y0 = interp_lerp<T>(e[0], e[1], f[1]);
        const T y1 = interp_lerp<T>(e[2], e[3], f[1]);
        out[q] = interp_lerp<T>(y0, y1, f[0]);
    }
}

// VJP of interp_combine w.r.t. the fractions: df[d] = sum_q u[q] d out_q / d f_d (d lerp / d f = b - a, d lerp / d a = 1 - f,
// d lerp / d b = f), for the upstream u[q] of the four channels.
template <typename T>
PVAMD_DEV void interp_fraction_vjp(const float4 r[8], const T f[3], const T u[4], bool has_g, T df[3]) {
    df[0] = df[1] = df[2] = T(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q > 0 && !has_g) break;
        T e[4], de[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const T a = (T)rec_ch(r[2 * ab], q), b = (T)rec_ch(r[2 * ab + 1], q);
            e[ab] = interp_lerp<T>(a, b, f[2]);
            de[ab] = b - a;
        }
        const T y0 = interp_lerp<T>(e[0], e[1], f[1]);
        const T y1 = interp_lerp<T>(e[2], e[3], f[1]);
        const T wx0 = T(1) - f[0], wy0 = T(1) - f[1];
        // d out / d f_x = y1 - y0;  d out / d y0 = 1 - f_x, d out / d y1 = f_x
        const T dfx = y1 - y0;
        const T dfy = wx0 * (e[1] - e[0]) + f[0] * (e[3] - e[2]);
        const T dfz = wx0 * (wy0 * de[0] + f[1] * de[1]) + f[0] * (wy0 * de[2] + f[1] * de[3]);
        df[0] += u[q] * dfx;
        df[1] += u[q] * dfy;
        df[2] += u[q] * dfz;
    }
}

// (val, gx, gy, gz) of one float64 point in a leaf's frame; returns the range test
template <bool INTERP>
PVAMD_DEV bool leaf_f64(const pvamd_grid_t& g, const double x[3], double o[4]) {
    long long key[3];
    const bool valid = voxel_key_f64(g, x, key);
    o[0] = o[1] = o[2] = o[3] = 0.0;
    if (valid) {
        if constexpr (INTERP) {
            InterpCell<double> c;
            interp_cell<double>(g, x, c);
            float4 r[8];
            interp_gather(g, c.base, r);
            interp_combine<double>(r, c.f, o);
        } else {
            const float4 r = load_record(g.vox, clamped_flat(g, key));
            o[0] = (double)r.x; o[1] = (double)r.y; o[2] = (double)r.z; o[3] = (double)r.w;
        }
    } else if (g.oob_mode == PVAMD_OOB_BOUNDING_BOX) {
        double t[3];
        o[0] = LeafOps<double>::box(g, x, t);
        o[1] = t[0] / o[0]; o[2] = t[1] / o[0]; o[3] = t[2] / o[0];
    }
    return valid;
}

}  // namespace pvamd
