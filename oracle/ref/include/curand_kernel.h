/*
 * curand_kernel.h — stand-in (TEST INFRASTRUCTURE ONLY; this project's own
 * text, see oracle/ref/README.md).
 *
 * Assumptions made here (also listed in DESIGN.md section 2):
 *  - curand_init / curand ARE the oracle's restatement of XORWOW
 *    (orc_curand_init / orc_curand, oracle/oracle.c).  cuRAND is an external
 *    dependency of the reference, not part of its text, so the random stream
 *    itself stays UNPINNED by this build: it only pins how the reference
 *    consumes the stream.  (Subsequence and offset are 0 at the reference's one
 *    call site; other values are refused.)
 *  - The device calls sin / cos / atan on floats (the reference's
 *    genMicrofacetNormal; its other trigonometry is host sinf / cosf / tanf,
 *    which stay libm's) go to the project's single-precision sequence
 *    orc_sinf / orc_cosf / orc_atanf.  The reference build's own
 *    --use_fast_math transcendentals cannot be reproduced, so they stay
 *    UNPINNED as well.  The redirection is by function-like macros defined
 *    after every standard header this translation unit needs has been
 *    included; the harness removes them again after the reference's text.
 */
#ifndef ORC_REF_CURAND_KERNEL_H
#define ORC_REF_CURAND_KERNEL_H

#include <stdint.h>

#include "cuda_runtime.h"

extern "C" {
void orc_curand_init(unsigned long long seed, uint32_t state[6]);
uint32_t orc_curand(uint32_t state[6]);
float orc_atanf(float x);
float orc_sinf(float x);
float orc_cosf(float x);
}

/* {d, v0..v4}: the oracle's and the product's state layout */
struct curandStateXORWOW {
    uint32_t s[6];
};
typedef curandStateXORWOW curandStateXORWOW_t;
typedef curandStateXORWOW curandState;

inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                        curandStateXORWOW* state) {
    if (subsequence != 0 || offset != 0) std::abort(); /* no skip-ahead restated */
    orc_curand_init(seed, state->s);
}
inline unsigned int curand(curandStateXORWOW* state) { return orc_curand(state->s); }

#define sin(x) orc_sinf(x)
#define cos(x) orc_cosf(x)
#define atan(x) orc_atanf(x)

#endif
