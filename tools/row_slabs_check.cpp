// Host-only check of the two grid-row helpers of csrc/common.h: for_row_slabs yields consecutive slabs from 0, in order, each of
// 1 .. kMaxGridRows rows, that sum to `rows` -- up to INT32_MAX rows, where a 32-bit slab counter would overflow --, and grid_rows
// gives what the ternary it replaced at the launch sites gave.  Needs no GPU: main() makes no HIP call.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 [-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined]
//       tools/row_slabs_check.cpp -o check && ./check
// Prints the slabs counted per row count; exit status 1 if anything is off.  (profiles/grid_rows.md)
#include <climits>
#include <cstdio>

#include "../pytorch_volumetric_amd/csrc/common.h"

using namespace pvamd;

int main() {
    const int32_t counts[] = {0, 1, 65534, 65535, 65536, 131070, 131071, 1 << 20, INT32_MAX};
    int bad = 0;
    for (int32_t rows : counts) {
        int64_t next = 0, slabs = 0;
        for_row_slabs(rows, [&](int32_t first, int32_t count) {
            if (first != next || count < 1 || count > kMaxGridRows) {
                if (bad++ < 10) printf("rows %d: slab %lld is (%d, %d), expected to start at %lld\n", rows, (long long)slabs, first, count, (long long)next);
            }
            next = (int64_t)first + count;
            ++slabs;
        });
        if (next != rows || slabs != ((int64_t)rows + kMaxGridRows - 1) / kMaxGridRows) {
            ++bad;
            printf("rows %d: %lld slabs end at %lld\n", rows, (long long)slabs, (long long)next);
        }
        // the launch sites' `A < 65535 ? A : 65535` (they refuse A < 1 before it; grid_rows(0) is a grid of one row)
        const unsigned before = rows < 1 ? 1u : (unsigned)(rows < 65535 ? rows : 65535);
        if (grid_rows(rows) != before) {
            ++bad;
            printf("grid_rows(%d) = %u, the ternary gives %u\n", rows, grid_rows(rows), before);
        }
        printf("rows %d: %lld slabs, grid_rows %u\n", rows, (long long)slabs, grid_rows(rows));
    }
    printf("%d differences\n", bad);
    return bad ? 1 : 0;
}
