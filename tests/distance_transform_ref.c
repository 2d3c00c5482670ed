/* Brute-force restatement of include/pvamd.h "Distance transform" -- TEST INFRASTRUCTURE, compiled on the fly with
 * -O2 -ffp-contract=off (tests/distance_transform_ref.py).  O(n * |Q|): for every voxel, every site of its class in ascending
 * flat order with a strict `<`, so the smallest flat index wins an equal squared distance; then the contract's float statements,
 * one operation per statement. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define NO_SITE 2147483647

void edt_ref(const uint8_t* occ, int32_t nx, int32_t ny, int32_t nz, float r, int32_t is_signed, float* records, int32_t* sites,
             int32_t* squared) {
    const int64_t n = (int64_t)nx * ny * nz;
    /* the sites of each class, ascending flat order, as coordinates */
    int32_t* list[2];
    int64_t count[2] = {0, 0};
    list[0] = (int32_t*)malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof(int32_t)); /* free voxels */
    list[1] = (int32_t*)malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof(int32_t)); /* occupied voxels */
    for (int64_t j = 0; j < n; ++j) {
        const int c = occ[j] != 0;
        int32_t* p = list[c] + 3 * count[c]++;
        p[0] = (int32_t)(j / ((int64_t)ny * nz));
        p[1] = (int32_t)((j / nz) % ny);
        p[2] = (int32_t)(j % nz);
    }
    for (int64_t i = 0; i < n; ++i) {
        const int occupied = occ[i] != 0;
        const int32_t x = (int32_t)(i / ((int64_t)ny * nz)), y = (int32_t)((i / nz) % ny), z = (int32_t)(i % nz);
        int32_t best = NO_SITE, sx = 0, sy = 0, sz = 0, site = -1;
        if (occupied && !is_signed) {
            best = 0, sx = x, sy = y, sz = z, site = (int32_t)i;
        } else {
            const int32_t* q = list[occupied ? 0 : 1];
            const int64_t m = count[occupied ? 0 : 1];
            for (int64_t k = 0; k < m; ++k) {
                const int32_t dx = x - q[3 * k], dy = y - q[3 * k + 1], dz = z - q[3 * k + 2];
                const int32_t d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best) {
                    best = d2, sx = q[3 * k], sy = q[3 * k + 1], sz = q[3 * k + 2];
                    site = (sx * ny + sy) * nz + sz;
                }
            }
        }
        float val = occupied ? -INFINITY : INFINITY, g[3] = {0.0f, 0.0f, 0.0f};
        if (site >= 0) {
            const float s = sqrtf((float)best);
            if (is_signed) {
                const float h = s - 0.5f;
                const float v = r * h;
                val = occupied ? -v : v;
            } else {
                val = r * s;
            }
            if (best > 0) {
                const int32_t e[3] = {occupied ? sx - x : x - sx, occupied ? sy - y : y - sy, occupied ? sz - z : z - sz};
                for (int k = 0; k < 3; ++k) g[k] = (float)e[k] / s;
            }
        }
        records[4 * i] = val;
        records[4 * i + 1] = g[0];
        records[4 * i + 2] = g[1];
        records[4 * i + 3] = g[2];
        sites[i] = site;
        squared[i] = best;
    }
    free(list[0]);
    free(list[1]);
}
