// The fixed-order sum of the transform stack's gradient, stated once for the backward kernels that form it (backward.hip
// composed_backward_kernel, leaf_pair.hip lph_backward_kernel; ray_cast_backward.hip composed_ray_cast_backward_kernel keeps a
// copy of steps 1 and 2 that must equal them, and shares step 3 and the plan).  A lane holds the twelve partials c[12] of one (configuration, point or ray) pair and its winning leaf
// s (-1: none).  They are added
//   1. over the wave: one butterfly per leaf that wins somewhere in the wave, into that wave's LDS slot (tf_wave_reduce);
//   2. over the four waves, in wave order, into one slab row per leaf, every row written (tf_block_store);
//   3. over the workgroups' slab rows, in chunk order (tf_chunk_sum; reduce_tf_kernel rounds once to the output's type).
// No float atomics, so two calls give the same bits; and the three kernels give each other's bits where their pairs are the
// same (tests/test_leaf_pair_hinge_gpu.py holds lph_backward_kernel to the one-leaf hinge backward).
// The host half is the plan that splits the configurations over workgroups and places the slab in the scratch buffer.
#pragma once
#include "common.h"
#include "composed_point.h"

namespace pvamd {

constexpr int kTfWaves = kBwdBlock / 64;  // every kernel here runs four waves per workgroup
constexpr int kTfMaxLeaves = 64;          // the per-wave LDS slots and the presence mask hold up to 64 leaves

// Step 1, called once per pair of the lane (wave-uniform).  part[wave][leaf][12] and present[wave] are the caller's LDS (CAP
// leaves, a Mask of at least CAP bits), present[wave] cleared by lane 0 before a configuration's first call.  The slot rule:
// assign on first sight of a leaf in this wave, then add.  CAP == 1 (the one-leaf kernel): the caller passes s in {-1, 0} only,
// so one pass takes every winner; that is the only special case here.
template <typename Acc, typename Mask, int CAP>
PVAMD_DEV void tf_wave_reduce(int s, const Acc (&c)[12], Acc (&part)[kTfWaves][CAP][12], Mask (&present)[kTfWaves], int wave, int lane) {
    static_assert(CAP >= 1 && CAP <= kTfMaxLeaves && (int)sizeof(Mask) * 8 >= CAP, "one bit of the presence mask per slot");
    uint64_t todo = __builtin_amdgcn_ballot_w64(s >= 0);
    while (todo) {  // wave-uniform: one butterfly per leaf that wins somewhere in the wave
        const int first = __builtin_ctzll(todo);
        const int sl = CAP == 1 ? 0 : __builtin_amdgcn_readlane(s, first);  // one slot: s is 0 wherever it is no -1,
        const bool mine = s == sl;
        todo = CAP == 1 ? 0 : todo & ~__builtin_amdgcn_ballot_w64(mine);    // and this pass takes every winner
        const bool seen = (present[wave] >> sl) & Mask(1);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const Acc v = hop_wave_sum<Acc>(mine ? c[j] : Acc(0));
            if (lane == 0) part[wave][sl][j] = seen ? part[wave][sl][j] + v : v;
        }
        if (lane == 0) present[wave] |= Mask(1) << sl;
        PVAMD_WAVE_SYNC();
    }
}

// Step 2, once per configuration (workgroup-uniform): leaf s's twelve sums go to row0 + s * leaf_stride; zeros for a leaf that
// won nowhere in the workgroup, so the slab needs no clearing.  The slots are free again when it returns.
template <typename Acc, typename Mask, int CAP>
PVAMD_DEV void tf_block_store(int S, const Acc (&part)[kTfWaves][CAP][12], const Mask (&present)[kTfWaves], Acc* __restrict__ row0,
                              int64_t leaf_stride) {
    static_assert(CAP >= 1 && CAP <= kTfMaxLeaves && (int)sizeof(Mask) * 8 >= CAP, "one bit of the presence mask per slot");
    __syncthreads();
    for (int e = threadIdx.x; e < S * 12; e += kTfWaves * 64) {
        const int s = e / 12, j = e - 12 * (e / 12);
        Acc v = Acc(0);
#pragma unroll
        for (int w = 0; w < kTfWaves; ++w)
            if ((present[w] >> s) & Mask(1)) v += part[w][s][j];
        row0[(int64_t)s * leaf_stride + j] = v;
    }
    __syncthreads();
}

// Step 3: first[0] + first[stride] + ... in chunk order
template <typename Acc>
PVAMD_DEV Acc tf_chunk_sum(const Acc* __restrict__ first, int64_t nchunks, int64_t stride) {
    Acc v = Acc(0);
    for (int64_t ch = 0; ch < nchunks; ++ch) v += first[ch * stride];
    return v;
}

// dtf[sa][r][c] = T(sum over chunks, in chunk order, of slab[chunk][sa][4r + c]) (row 3: zeros)
template <typename Acc, typename T>
__global__ __launch_bounds__(256) void reduce_tf_kernel(const Acc* __restrict__ slab, int64_t nchunks, int64_t SA, T* __restrict__ dtf) {
    const int64_t n = SA * 16;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t sa = e >> 4;
        const int rc = (int)(e & 15);
        dtf[e] = (T)(rc < 12 ? tf_chunk_sum<Acc>(slab + sa * 12 + rc, nchunks, SA * 12) : Acc(0));
    }
}

template <typename Acc, typename T>
static inline void launch_reduce_tf(const Acc* slab, int64_t nchunks, int64_t SA, T* dtf, hipStream_t st) {
    hipLaunchKernelGGL((reduce_tf_kernel<Acc, T>), dim3(stream_grid(SA * 16, 256)), dim3(256), 0, st, slab, nchunks, SA, dtf);
}

// host: the configurations are split over workgroups until about kBwdTargetBlocks exist.  `rows` workgroups exist without a
// split (the point or ray chunks, times the pairs in leaf_pair.hip); each then takes `aper` configurations, `nsplit` per row.
struct TfSplit {
    int aper, nsplit;
};

static inline TfSplit tf_split_plan(int64_t rows, int A) {
    int64_t want = (kBwdTargetBlocks + rows - 1) / rows;
    if (want > A) want = A;
    if (want < 1) want = 1;
    TfSplit p;
    p.aper = (int)((A + want - 1) / want);
    p.nsplit = (A + p.aper - 1) / p.aper;
    return p;
}

// host: bytes of a slab of `rows` rows of twelve sums, up to where the next part of the scratch buffer starts
static inline int64_t tf_slab_bytes(int64_t rows, size_t elem) { return round256(rows * 12 * (int64_t)elem); }

}  // namespace pvamd
