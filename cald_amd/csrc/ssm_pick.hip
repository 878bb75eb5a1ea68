// ssm_pick.hip -- cald_ssm_pick_mt19937: the sub-sampling of detection/retina_ssm.py:540-542 (`keep = list(range(n)); random.shuffle(keep);
// keep[:500]`, once per class) restated on a copy of CPython's generator state, so that a sweep consumes the generator exactly as the
// reference's tail does without paying random.shuffle's interpreter time per candidate.  Host code only; nothing here touches the GPU, and
// the file builds as plain C++ too.
//   genrand_uint32   MT19937 (Matsumoto & Nishimura 2002), the generator behind CPython's _random: state word i of 624, regenerated in one
//                    pass when the index reaches 624.
//   randbelow(m)     random.Random._randbelow_with_getrandbits: k = m.bit_length(); r = getrandbits(k) = genrand_uint32() >> (32 - k), drawn
//                    again while r >= m.  m <= 2^20 + 1 here, so k <= 21 and one word a draw.
//   shuffle          random.shuffle: for i in reversed(range(1, n)): j = randbelow(i + 1); x[i], x[j] = x[j], x[i].  n of 0 or 1 draws nothing.
#include "../../include/cald_hip.h"

#include <vector>

namespace {
const int MT_N = 624, MT_M = 397;

inline uint32_t genrand_uint32(uint32_t* mt, uint32_t* index) {
    if (*index >= (uint32_t)MT_N) {
        int kk = 0;
        for (; kk < MT_N - MT_M; kk++) {
            const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
            mt[kk] = mt[kk + MT_M] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        for (; kk < MT_N - 1; kk++) {
            const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
            mt[kk] = mt[kk + (MT_M - MT_N)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        const uint32_t y = (mt[MT_N - 1] & 0x80000000u) | (mt[0] & 0x7fffffffu);
        mt[MT_N - 1] = mt[MT_M - 1] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        *index = 0;
    }
    uint32_t y = mt[(*index)++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

inline uint32_t randbelow(uint32_t m, uint32_t* mt, uint32_t* index) {      // m >= 2
    int k = 0;
    for (uint32_t t = m; t; t >>= 1) k++;
    uint32_t r = genrand_uint32(mt, index) >> (32 - k);
    while (r >= m) r = genrand_uint32(mt, index) >> (32 - k);
    return r;
}
}  // namespace

extern "C" int cald_ssm_pick_mt19937(void* user, int image, int K, const int* counts, int* picks, int* n_picks) {
    (void)image;
    if (!user || !counts || !picks || !n_picks || K < 0) return 1;
    uint32_t* mt = static_cast<uint32_t*>(user);
    uint32_t index = mt[MT_N];
    if (index > (uint32_t)MT_N) return 2;
    for (int k = 0; k < K; k++) if (counts[k] < 0) return 3;
    std::vector<int> x;
    for (int k = 0; k < K; k++) {
        const int n = counts[k];
        x.resize((size_t)n);
        for (int i = 0; i < n; i++) x[(size_t)i] = i;
        for (int i = n - 1; i >= 1; i--) {
            const uint32_t j = randbelow((uint32_t)i + 1u, mt, &index);
            const int t = x[(size_t)i]; x[(size_t)i] = x[j]; x[j] = t;
        }
        const int take = n < CALD_SSM_RETINA_TAKE ? n : CALD_SSM_RETINA_TAKE;
        for (int i = 0; i < take; i++) picks[(size_t)k * CALD_SSM_RETINA_TAKE + i] = x[(size_t)i];
        n_picks[k] = take;
    }
    mt[MT_N] = index;
    return 0;
}
