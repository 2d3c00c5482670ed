// Host-only check that mesh_query_plan / chamfer_mesh_plan (csrc/mesh.hip) and order_kind (csrc/sort.hip) give what the
// expressions they replaced gave: those expressions stand below as mesh_query_impl, launch_chamfer_mesh, launch_heavy_parts and
// pvamd_morton_order had them, and are compared over a grid of sizes.  Needs no GPU: main() makes no HIP call (the kernels of
// the two files are compiled along because the files are included whole, and are never launched).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 [-Xarch_host -fsanitize=address,undefined] tools/mesh_plan_check.cpp -o check && ./check
// Prints the number of tuples and of differences; exit status 1 if any differ.  (profiles/mesh_plan.md)
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "../pytorch_volumetric_amd/csrc/mesh.hip"
#include "../pytorch_volumetric_amd/csrc/sort.hip"

// ---- the parent's expressions, verbatim ----
static int pick_slices_before(int64_t groups, int mesh_tiles, bool hand_over) {
    int s = 2;
    while (s < 8 && (int64_t)s * groups < 16384) s <<= 1;
    if (mesh_tiles > 128 && !hand_over) s = 8;
    if (s > 8) s = 8;
    while (s > 1 && s > mesh_tiles) s >>= 1;
    return s;
}

struct Before {
    int64_t groups;
    int cap;                          // PVAMD_MESH_SCRATCH_SLOTS
    bool two_launches, heavy;
    bool sort_in_prep, sort_call;     // how an unordered query got its order
    int slices, parts, aw, heavy_parts;
};

// mesh_query_impl between its argument checks and its launches (ho_cap = ho.cap: the slots of a scratch that is there)
static Before query_before(int64_t P, int F, bool has_scratch, bool sort_into) {
    Before b = {};
    const int64_t groups = (P + 63) / 64;
    const int ntiles = (F + 256 - 1) / 256;
    const int cap = (int)PVAMD_MESH_SCRATCH_SLOTS(P);
    const int ho_cap = has_scratch ? cap : 0;
    const int slices = pick_slices_before(groups, ntiles, ho_cap > 0 && ntiles >= 128);
    const int half_tiles = groups <= 64 ? 2 : (groups <= 256 ? 3 : (groups < 2048 ? 6 : (int)(groups / 256)));
    int parts = (2 * ntiles + half_tiles - 1) / half_tiles;
    if (parts > 65535) parts = 65535;
    const int aw = (int64_t)groups * parts * 4 > 100000 ? 2 : 4;
    const bool few = parts >= 4;
    const bool two_launches = ho_cap > 0 && groups <= ho_cap && few;
    const bool heavy = ho_cap > 0 && ntiles >= 128;
    b.groups = groups; b.cap = cap; b.two_launches = two_launches; b.heavy = heavy;
    b.sort_in_prep = sort_into && two_launches; b.sort_call = sort_into && !two_launches;
    b.slices = slices; b.parts = parts; b.aw = aw;
    b.heavy_parts = 32 < ntiles ? 32 : ntiles;  // launch_heavy_parts
    return b;
}

// launch_chamfer_mesh: ny = B, or 1 for the flat call
static Before chamfer_before(int64_t N, int64_t ny, int F, bool has_scratch) {
    Before b = {};
    const int64_t groups = (N + 63) / 64;
    const int ntiles = (F + 256 - 1) / 256;
    const int cap = (int)PVAMD_MESH_SCRATCH_SLOTS(N);
    const int ho_cap = (ntiles >= 128 ? has_scratch : false) ? cap : 0;
    b.groups = groups; b.cap = cap;
    b.slices = pick_slices_before(groups * (int64_t)ny, ntiles, ho_cap > 0);
    b.heavy = ho_cap > 0;
    b.heavy_parts = 32 < ntiles ? 32 : ntiles;
    return b;
}

static bool same_query(const Before& b, const pvamd_mesh_plan_t& p, bool unordered) {
    if (p.groups != b.groups || p.slots != b.cap) return false;
    if (b.two_launches)
        return p.path == PVAMD_MESH_PATH_LISTED && p.parts == b.parts && p.part_waves == b.aw && p.scan_waves == 0 &&
               p.order == (b.sort_in_prep ? PVAMD_MESH_ORDER_INSIDE : PVAMD_MESH_ORDER_GIVEN) && !b.sort_call;
    if (p.order != (b.sort_call ? PVAMD_MESH_ORDER_SORT_CALL : PVAMD_MESH_ORDER_GIVEN) || b.sort_in_prep || (unordered != b.sort_call)) return false;
    if (p.scan_waves != b.slices) return false;
    if (b.heavy) return p.path == PVAMD_MESH_PATH_SCAN_HEAVY && p.parts == b.heavy_parts && p.part_waves == 4;
    return p.path == PVAMD_MESH_PATH_SCAN && p.parts == 0 && p.part_waves == 0;
}

// pvamd_morton_order's three branches: 0 one workgroup, 1 counting, 2 radix; the key bits each sorts on; grid.x of its first launch
struct SortBefore { int kind, bits; int64_t first_grid; };
static SortBefore sort_before(int64_t P) {
    if (P <= 16384) return {0, 12, 1};  // order_small_kernel, dim3(1), dim3(1024): 16^3 cells
    if (P >= PVAMD_ORDER_RADIX_SORT_FROM) {
        const int64_t tiles = (P + 4096 - 1) / 4096;
        int G = 1;
        while ((int64_t)G * G < tiles) ++G;
        const int nsg = (int)((tiles + G - 1) / G);
        const int zero_words = 3 * nsg * 128;
        return {2, PVAMD_MORTON_ORDER_BITS(P), (zero_words + 255) / 256};
    }
    const int bits = PVAMD_MORTON_ORDER_BITS(P), cells = 1 << bits;
    return {1, bits, (cells + 255) / 256};
}
static int64_t first_grid_now(int64_t P) {  // from the layouts pvamd_morton_order carves with
    switch (order_kind(P)) {
        case OrderKind::kSmall: return 1;
        case OrderKind::kRadix: { const RadixLayout l = radix_layout(P); return ((int)(l.table - l.sgtotal) + 255) / 256; }
        default: return ((1 << PVAMD_MORTON_ORDER_BITS(P)) + 255) / 256;
    }
}

int main() {
    static_assert(kOrderSmallPoints == 16384 && kOrderSmallThreads == 1024, "the one-workgroup sort's capacity moved: so must sort_before");
    const int tiles[] = {0, 1, 2, 11, 12, 62, 127, 128, 129, 140, 262144};
    std::vector<int> Fs;
    for (int t : tiles) {
        Fs.push_back(t * 256);
        if (t > 0) Fs.push_back((t - 1) * 256 + 1);  // the same number of tiles, the last one holding one record
    }
    const int64_t top_groups = (int64_t)1 << 20;  // 2^26 points
    long long tuples = 0, diffs = 0, changes = 0;
    std::set<std::tuple<int, int, int, int, int>> plans;
    auto report = [&](const char* what, int64_t P, int64_t rows, int F, int sc, int un) {
        if (diffs++ < 10) printf("%s differs: P %lld rows %lld F %d scratch %d unordered %d\n", what, (long long)P, (long long)rows, F, sc, un);
    };
    // every group count up to 2^20 (so: both sides of every change of every field), each at its first, a ragged and its last point count
    for (int F : Fs)
        for (int sc = 0; sc < 2; ++sc)
            for (int un = 0; un < 2; ++un) {
                pvamd_mesh_plan_t last = {};
                for (int64_t g = 1; g <= top_groups; ++g) {
                    const int64_t Ps[] = {64 * g - 63, 64 * g - 37, 64 * g};
                    for (int64_t P : Ps) {
                        if (un && P > PVAMD_MESH_SMALL_POINTS) continue;
                        ++tuples;
                        pvamd_mesh_plan_t now = {};
                        if (pvamd_mesh_query_plan(P, F, sc, un, &now) != 0 || !same_query(query_before(P, F, sc, un), now, un)) report("query", P, 1, F, sc, un);
                        if (now.path != last.path || now.order != last.order || now.scan_waves != last.scan_waves || now.parts != last.parts || now.part_waves != last.part_waves) ++changes;
                        last = now;
                        plans.insert({now.path, now.order, now.scan_waves, now.parts > 0, now.part_waves});
                    }
                }
            }
    const int64_t rows_of[] = {1, 2, 10000, 70000};
    for (int F : Fs)
        for (int sc = 0; sc < 2; ++sc)
            for (int64_t rows : rows_of)
                for (int64_t g = 1; g <= top_groups; g += (g < 8200 ? 1 : 7)) {
                    const int64_t Ns[] = {64 * g - 63, 64 * g - 37, 64 * g};
                    for (int64_t N : Ns) {
                        ++tuples;
                        pvamd_mesh_plan_t now = {};
                        const int rc = pvamd_chamfer_mesh_plan(N, (int32_t)rows, F, sc, &now);
                        if (F == 0) {  // the entry point zeroes the sums and returns
                            if (rc != 0 || now.path != PVAMD_MESH_PATH_NONE) report("chamfer", N, rows, F, sc, 0);
                            continue;
                        }
                        const Before b = chamfer_before(N, rows, F, sc);
                        const bool same = rc == 0 && now.groups == b.groups && now.slots == b.cap && now.scan_waves == b.slices &&
                                          now.order == PVAMD_MESH_ORDER_GIVEN &&
                                          (b.heavy ? now.path == PVAMD_MESH_PATH_SCAN_HEAVY && now.parts == b.heavy_parts && now.part_waves == 4
                                                   : now.path == PVAMD_MESH_PATH_SCAN && now.parts == 0 && now.part_waves == 0);
                        if (!same) report("chamfer", N, rows, F, sc, 0);
                    }
                }
    // the sort: every point count up to 2^21 + 2, then both sides of powers of two and of the thresholds up to 2^31 - 1
    std::set<int64_t> Ps;
    for (int64_t P = 0; P <= (1 << 21) + 2; ++P) Ps.insert(P);
    for (int sh = 21; sh <= 31; ++sh)
        for (int64_t d = -2; d <= 2; ++d)
            if (((int64_t)1 << sh) + d <= 0x7fffffffLL) Ps.insert(((int64_t)1 << sh) + d);
    long long sort_tuples = 0, sort_diffs = 0;
    for (int64_t P : Ps) {
        ++sort_tuples;
        const SortBefore b = sort_before(P);
        if (pvamd_morton_order_kernel(P) != b.kind || (int)order_kind(P) != b.kind || pvamd_morton_order_bits(P) != b.bits ||
            (P > 0 && first_grid_now(P) != b.first_grid))
            if (sort_diffs++ < 10) printf("sort differs: P %lld\n", (long long)P);
    }
    // the refused arguments
    pvamd_mesh_plan_t p;
    const bool refused = pvamd_mesh_query_plan(-1, 1, 0, 0, &p) == PVAMD_E_SHAPE && pvamd_mesh_query_plan(1, -1, 0, 0, &p) == PVAMD_E_SHAPE &&
                         pvamd_mesh_query_plan(1, (1 << 26) + 1, 0, 0, &p) == PVAMD_E_SHAPE &&
                         pvamd_mesh_query_plan(PVAMD_MESH_SMALL_POINTS + 1, 1, 1, 1, &p) == PVAMD_E_SHAPE &&
                         pvamd_mesh_query_plan((int64_t)64 << 31, 1, 0, 0, &p) == PVAMD_E_SHAPE && pvamd_mesh_query_plan(1, 1, 0, 0, nullptr) == PVAMD_E_NULL &&
                         pvamd_chamfer_mesh_plan(1, -1, 1, 0, &p) == PVAMD_E_SHAPE && pvamd_chamfer_mesh_plan(-1, 1, 1, 0, &p) == PVAMD_E_SHAPE &&
                         pvamd_morton_order_kernel(-1) == PVAMD_E_SHAPE && pvamd_morton_order_bits((int64_t)1 << 31) == PVAMD_E_SHAPE;
    if (!refused) { ++diffs; printf("a refused argument was not refused\n"); }
    printf("%lld (points, rows, faces, scratch, unordered) tuples: %lld plan differences; %lld plan changes crossed, %zu distinct (path, order, "
           "scan waves, parts > 0, part waves)\n", tuples, diffs, changes, plans.size());
    printf("%lld point counts of the sort: %lld differences\n", sort_tuples, sort_diffs);
    return diffs || sort_diffs ? 1 : 0;
}
