// Host-only check that composed_kind (csrc/composed.hip) and config_rows (csrc/common.h) give what the expressions they
// replaced gave: those expressions stand below as pvamd_composed_query, pvamd_composed_query_grouped and composed_f64 had
// them, and are compared over a grid of (A, P, flags).  Needs no GPU: main() makes no HIP call (the kernels of composed.hip are
// compiled along because the file is included whole, and are never launched).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 [-Xarch_host -fsanitize=address,undefined] tools/composed_kind_check.cpp -o check && ./check
// Prints the number of tuples and of differences; exit status 1 if any differ.  (profiles/composed_dispatch.md)
#include <cstdio>
#include <set>
#include <vector>

#include "../pytorch_volumetric_amd/csrc/composed.hip"

// 0 per-lane, 1 wave-tile, 2 fused: the order the entry point tested them in
static int kind_before(int32_t A, int64_t P, int32_t flags) {
    const int64_t ntiles = (P + kTilePoints - 1) / kTilePoints;
    {
        const int64_t nchunks = (P + kFusedChunk - 1) / kFusedChunk;
        const bool plain_flags = !(flags & (PVAMD_COMPOSED_INLINE_EXACT | PVAMD_COMPOSED_FORCE_PER_LANE |
                                            PVAMD_COMPOSED_FORCE_WAVE_TILE | PVAMD_COMPOSED_NO_GROUPING));
        const bool fused = P >= kFusedChunk &&
                           ((plain_flags && nchunks * (int64_t)A >= kFusedMinBlocks) || (flags & PVAMD_COMPOSED_FORCE_FUSED));
        if (fused) return 2;
    }
    const bool wave_tiles = P >= kTilePoints && ((A >= 2 && ntiles * (int64_t)A >= kWaveTileMinTiles && !(flags & PVAMD_COMPOSED_FORCE_PER_LANE)) || (flags & PVAMD_COMPOSED_FORCE_WAVE_TILE));
    return wave_tiles ? 1 : 0;
}

// gridDim.y as the direct and the grouped entry points computed it
static unsigned rows_before(int32_t A, int64_t need) {
    int64_t cap = ((int64_t)65536 + A - 1) / A;
    if (cap > 65535) cap = 65535;  // gridDim.y
    return (unsigned)(need < cap ? need : (cap < 1 ? 1 : cap));
}

// ... and as the float64 lane query did
static unsigned rows_before_f64(int32_t A, int64_t P) {
    int64_t gy = (P + 255) / 256;
    int64_t cap = ((int64_t)65536 + A - 1) / A;
    if (cap > 65535) cap = 65535;
    if (gy > cap) gy = cap;
    return (unsigned)(gy < 1 ? 1 : gy);
}

int main() {
    const int32_t As[] = {1, 2, 7, 8, 200, 2185, 65535, 70000};
    const int32_t bits[] = {PVAMD_COMPOSED_INLINE_EXACT, PVAMD_COMPOSED_FORCE_PER_LANE, PVAMD_COMPOSED_FORCE_WAVE_TILE,
                            PVAMD_COMPOSED_NO_GROUPING, PVAMD_COMPOSED_FORCE_FUSED};
    std::set<int64_t> Ps;
    auto around = [&](int64_t p) {
        for (int64_t d = -2; d <= 2; ++d)
            if (p + d >= 0) Ps.insert(p + d);
    };
    around(0); around(kTilePoints); around(kFusedChunk); around(kGroupChunk);
    for (int32_t A : As) {
        // the first point count of the tile / chunk count at which the product with A reaches its threshold, and of its neighbours
        const int64_t tiles = (kWaveTileMinTiles + A - 1) / A, chunks = (kFusedMinBlocks + A - 1) / A;
        for (int64_t d = -1; d <= 1; ++d) {
            around((tiles + d) * kTilePoints); around((tiles + d - 1) * kTilePoints + 1);
            around((chunks + d) * kFusedChunk); around((chunks + d - 1) * kFusedChunk + 1);
        }
    }
    for (int64_t k = 1; k <= 300; ++k) Ps.insert(k * 97);            // below and around one chunk
    for (int64_t k = 1; k <= 100; ++k) Ps.insert(k * 41'943 + 191);  // ragged sizes up to 4M
    for (int sh = 23; sh <= 40; ++sh) around((int64_t)1 << sh);
    long long tuples = 0, kind_diffs = 0, row_diffs = 0;
    for (int32_t A : As)
        for (int64_t P : Ps) {
            for (int m = 0; m < 32; ++m) {
                int32_t flags = 0;
                for (int b = 0; b < 5; ++b)
                    if (m >> b & 1) flags |= bits[b];
                ++tuples;
                if ((int)composed_kind(A, P, flags) != kind_before(A, P, flags)) {
                    if (kind_diffs++ < 10) printf("kind differs: A %d P %lld flags %d\n", A, (long long)P, flags);
                }
                if (pvamd_composed_query_kernel(A, P, flags) != kind_before(A, P, flags)) ++kind_diffs;
            }
            if (P < 1) continue;  // every launch site returns before its grid for P = 0
            const int64_t needs[] = {(P + kFusedChunk - 1) / kFusedChunk, ((P + kTilePoints - 1) / kTilePoints + kWavesPerBlock - 1) / kWavesPerBlock,
                                     (P + 255) / 256, (P + kGroupChunk - 1) / kGroupChunk};
            for (int64_t need : needs)
                if (config_rows(A, need) != rows_before(A, need)) ++row_diffs;
            if (config_rows(A, (P + 255) / 256) != rows_before_f64(A, P)) ++row_diffs;
        }
    printf("%lld (A, P, flags) tuples over %zu point counts: %lld kind differences, %lld grid-row differences\n", tuples, Ps.size(),
           kind_diffs, row_diffs);
    return kind_diffs || row_diffs ? 1 : 0;
}
