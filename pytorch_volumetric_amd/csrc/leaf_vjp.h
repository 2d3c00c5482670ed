// The per-leaf VJPs shared by the backward kernels (backward.hip, min_over_points.hip): given a leaf-frame point x and the
// upstream (dv, dg) of the leaf's (val, grad), the point's VJP dx -- the bounding-box branch (sdf.py:559-571) and the
// interpolated leaf in range (interp.h).  The nearest leaf in range is a table lookup: no derivative w.r.t. x.
#pragma once
#include "grid_lookup.h"
#include "interp.h"

namespace pvamd {

// dx of the bounding-box branch at a point x outside the range: dv n + (I - n n^T) dg / |d| on the active axes.
// Returns |d| (the value) for callers that need it.
template <typename T>
PVAMD_DEV T box_backward(const pvamd_grid_t& g, const T x[3], T dv, const T dg[3], bool has_g, T n[3], T dx[3]) {
    T t[3];
    const T nrm = LeafOps<T>::box(g, x, t);
#pragma unroll
    for (int d = 0; d < 3; ++d) n[d] = LeafOps<T>::div(t[d], nrm);
    T dot = 0;
    if (has_g) dot = n[0] * dg[0] + n[1] * dg[1] + n[2] * dg[2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        T v = dv * n[d];
        if (has_g) v += LeafOps<T>::div(dg[d] - n[d] * dot, nrm);
        dx[d] = (t[d] != T(0)) ? v : T(0);
    }
    return nrm;
}

// The interpolated leaf (interpolation="trilinear", interp.h) in range: the interpolated record and the VJP of its four channels
// w.r.t. x through the fractions -- d f_d / d x_d = 1 / res_d (torch's div backward: upstream / res_d), 0 on a clamped axis.
// gr = the interpolated gradient (what the forward rotated back), dx = the point's VJP.
template <typename T> struct InterpOps {
    static PVAMD_DEV T res(const pvamd_grid_t& g, int d) {
        if constexpr (sizeof(T) == 8) return g.dres[d];
        else return g.fres[d];
    }
    static PVAMD_DEV void leaf(const pvamd_grid_t& g, const T x[3], T dv, const T dg[3], bool has_g, T gr[3], T dx[3]) {
        InterpCell<T> c;
        interp_cell<T>(g, x, c);
        float4 r[8];
        interp_gather(g, c.base, r);
        T o[4];
        interp_combine<T>(r, c.f, o);
        gr[0] = o[1]; gr[1] = o[2]; gr[2] = o[3];
        const T u[4] = {dv, dg[0], dg[1], dg[2]};
        T df[3];
        interp_fraction_vjp<T>(r, c.f, u, has_g, df);
#pragma unroll
        for (int d = 0; d < 3; ++d) dx[d] = c.cl[d] ? T(0) : LeafOps<T>::div(df[d], res(g, d));
    }
};

}  // namespace pvamd
