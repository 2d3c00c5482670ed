/* Restatement of the pair transform of include/pvamd.h "Leaf-pair distance" 1 for tests/test_self_collision_gpu.py -- TEST
 * INFRASTRUCTURE, compiled at test time with -ffp-contract=off so that every product is rounded on its own and every fma is the
 * one written here.  tf [S*A][4][4] leaf-major, pairs [K][2] int64, out [K][A][4][4]. */
#include <math.h>
#include <stdint.h>

#define PAIR_TRANSFORMS(NAME, T, FMA)                                                                         \
    void NAME(const T* tf, int S, int A, const int64_t* pairs, int K, T* out) {                               \
        (void)S;                                                                                              \
        for (int k = 0; k < K; ++k)                                                                           \
            for (int a = 0; a < A; ++a) {                                                                     \
                const T* Ms = tf + 16 * ((int64_t)pairs[2 * k] * A + a);                                      \
                const T* Mt = tf + 16 * ((int64_t)pairs[2 * k + 1] * A + a);                                  \
                T* C = out + 16 * ((int64_t)k * A + a);                                                       \
                for (int i = 0; i < 3; ++i) {                                                                 \
                    for (int j = 0; j < 3; ++j)                                                               \
                        C[4 * i + j] = FMA(Ms[4 * i + 2], Mt[4 * j + 2],                                      \
                                           FMA(Ms[4 * i + 1], Mt[4 * j + 1], Ms[4 * i] * Mt[4 * j]));         \
                    C[4 * i + 3] = Ms[4 * i + 3] - FMA(C[4 * i + 2], Mt[11], FMA(C[4 * i + 1], Mt[7], C[4 * i] * Mt[3])); \
                }                                                                                             \
                C[12] = 0; C[13] = 0; C[14] = 0; C[15] = 1;                                                   \
            }                                                                                                 \
    }

PAIR_TRANSFORMS(pair_transforms_f32, float, fmaf)
PAIR_TRANSFORMS(pair_transforms_f64, double, fma)
