// The composed answer at one point, with the fused forwards' own leaf statements: shared by the reductions over points
// (min_over_points.hip, hinge_over_points.hip) and the hinge backward (backward.hip), which recompute the value and the winning
// leaf per pair instead of storing them.  float32 nearest = cached_lookup (the cached kernels' fast index with the exact
// fallback, the bounding-box branch), float32 trilinear = composed_interp_kernel's leaf, float64 = leaf_f64.
#pragma once
#include "grid_lookup.h"
#include "interp.h"
#include "leaf_vjp.h"

namespace pvamd {

// The exact first-minimum reduction of the reductions over points (min_over_points.hip, leaf_pair.hip)
constexpr uint32_t kNoIndex = 0xffffffffu;

// order-preserving key of a value: NaN -> 0 (below every number), -0 -> +0, then the usual sign-magnitude flip
PVAMD_DEV uint64_t mop_key(float v) {
    if (v != v) return 0;
    uint32_t u = (uint32_t)__float_as_int(v == 0.f ? 0.f : v);
    return (u >> 31) ? (uint64_t)(~u) : (uint64_t)(u | 0x80000000u);
}
PVAMD_DEV uint64_t mop_key(double v) {
    if (v != v) return 0;
    uint64_t u = (uint64_t)__double_as_longlong(v == 0.0 ? 0.0 : v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

struct MopKey {
    uint64_t key;  // mop_key of the value; ~0 when the slot saw no point
    uint32_t idx;  // point index; kNoIndex when the slot saw no point
    uint32_t pad;
};

PVAMD_DEV bool mop_less(uint64_t k0, uint32_t i0, uint64_t k1, uint32_t i1) { return k0 < k1 || (k0 == k1 && i0 < i1); }

// the minimum (key, idx) over the wave, in every lane
PVAMD_DEV void mop_wave_min(uint64_t& k, uint32_t& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((unsigned)(k & 0xffffffffu), off, 64);
        const uint32_t hi = __shfl_xor((unsigned)(k >> 32), off, 64);
        const uint32_t oi = __shfl_xor((unsigned)i, off, 64);
        const uint64_t ok = ((uint64_t)hi << 32) | lo;
        if (mop_less(ok, oi, k, i)) { k = ok; i = oi; }
    }
}

// The hinge's fixed-order float64 sum (hinge_over_points.hip, leaf_pair.hip): per lane in point order over kHopK points of a
// PVAMD_MOP_CHUNK chunk, a wave butterfly, the four waves in order, then the chunks in chunk order
constexpr int kHopBlock = 256;
constexpr int kHopK = PVAMD_MOP_CHUNK / kHopBlock;  // points per lane per chunk
static_assert(kHopK * kHopBlock == PVAMD_MOP_CHUNK, "whole lanes per chunk");

struct HopPart {
    double sum;     // the chunk's terms, in float64
    int64_t count;  // the chunk's points with v < m
};

template <typename T>
PVAMD_DEV T hop_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;  // a butterfly: every lane holds the same bits
}

// The composed backward's workgroup (backward.hip composed_backward_kernel, leaf_pair.hip lph_backward_kernel)
constexpr int kBwdBlock = 256;                     // four waves
constexpr int kBwdK = 4;                           // points per lane
constexpr int kBwdChunk = kBwdBlock * kBwdK;       // points per workgroup
constexpr int kBwdTargetBlocks = 2048;             // configurations are split over workgroups until about this many exist

// host: where the next part of a scratch buffer starts
static inline int64_t round256(int64_t n) { return ((n + 255) / 256) * 256; }

// (val, gx, gy, gz) of one leaf at the leaf-frame point x
template <typename T, bool INTERP> struct MopLeaf;

template <> struct MopLeaf<float, false> {
    static PVAMD_DEV void eval(const pvamd_grid_t& g, const float x[3], float o[4]) {
        bool valid;
        const float4 r = cached_lookup<false>(g, x[0], x[1], x[2], valid);
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
    }
};

template <> struct MopLeaf<float, true> {
    static PVAMD_DEV void eval(const pvamd_grid_t& g, const float x[3], float o[4]) {
        if (in_range(g, x[0], x[1], x[2])) {
            InterpCell<float> c;
            interp_cell<float>(g, x, c);
            float4 r[8];
            interp_gather(g, c.base, r);
            interp_combine<float>(r, c.f, o);
        } else {
            const float4 b = bounding_box_sdf(g, x[0], x[1], x[2]);
            o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
        }
    }
};

template <bool INTERP> struct MopLeaf<double, INTERP> {
    static PVAMD_DEV void eval(const pvamd_grid_t& g, const double x[3], double o[4]) { leaf_f64<INTERP>(g, x, o); }
};

// The composed answer over leaves [s0, s1) at object-frame point p under configuration a: the first minimum (NaN counts as the
// minimum) and the winner's gradient rotated back -- composed_interp_kernel's statements in float32, composed_query_f64_kernel's
// in float64.  bs = the winning leaf.
template <typename T, bool INTERP>
PVAMD_DEV void mop_point(const pvamd_grid_t* __restrict__ grids, int s0, int s1, const T* __restrict__ tf, int A, int a,
                         const T p[3], T& bv, T bg[3], int& bs) {
    if constexpr (sizeof(T) == 4) {
        bv = __builtin_inff();
        T lg[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        bs = s0;
        for (int s = s0; s < s1; ++s) {
            const T* M = tf + 16 * ((int64_t)s * A + a);  // wave-uniform: scalar loads
            T x[3], o[4];
            LeafOps<T>::xform(M, p, x);
            MopLeaf<T, INTERP>::eval(grids[s], x, o);
            const bool take = !(o[0] >= bv) & (bv == bv);
            bv = take ? o[0] : bv;
            lg[0] = take ? o[1] : lg[0];
            lg[1] = take ? o[2] : lg[1];
            lg[2] = take ? o[3] : lg[2];
            bs = take ? s : bs;
        }
        const T* M = tf + 16 * ((int64_t)bs * A + a);
        bg[0] = fmaf(M[8], lg[2], fmaf(M[4], lg[1], mul_rn(M[0], lg[0])));
        bg[1] = fmaf(M[9], lg[2], fmaf(M[5], lg[1], mul_rn(M[1], lg[0])));
        bg[2] = fmaf(M[10], lg[2], fmaf(M[6], lg[1], mul_rn(M[2], lg[0])));
    } else {
        bv = 0.0;
        bg[0] = bg[1] = bg[2] = 0.0;
        bs = -1;
        for (int s = s0; s < s1; ++s) {
            const T* M = tf + 16 * ((int64_t)s * A + a);
            T x[3], o[4];
            LeafOps<T>::xform(M, p, x);
            MopLeaf<T, INTERP>::eval(grids[s], x, o);
            if ((bs < 0) || (o[0] < bv) || (o[0] != o[0] && bv == bv)) {
                bv = o[0];
                bs = s;
#pragma unroll
                for (int j = 0; j < 3; ++j) bg[j] = __builtin_fma(M[8 + j], o[3], __builtin_fma(M[4 + j], o[2], M[j] * o[1]));
            }
        }
    }
}

}  // namespace pvamd
