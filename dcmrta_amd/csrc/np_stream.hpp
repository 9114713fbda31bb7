// np_stream.hpp -- the random stream of np.random.default_rng(seed) for a uint64 seed, stated once.  Plain functions of integers
// behind a __host__ __device__ guard macro, no HIP and no handle, so that a host compiler alone can build it (tests/
// test_np_stream_host.py compares it with numpy that way) and instgen.hpp runs the very same code on the device.
//
// The reference makes every problem instance from such a stream (env/task_env.py:21-22,36-48,57-71): SeedSequence(seed) ->
// PCG64 (XSL-RR 128/64) -> Generator.random / Generator.integers.  What is restated here:
//   seeding   SeedSequence with the entropy as little-endian uint32 words (missing words hash as 0), pool of 4,
//             generate_state(4, uint64) = v[0..3]; pcg64 srandom with initstate = v0<<64 | v1, initseq = v2<<64 | v3
//   next64    state = state * MULT + inc, output = rotr64(hi ^ lo, state >> 122)
//   random    (next64 >> 11) * 2^-53
//   uint32    the low half of a fresh next64, the high half is kept for the next call (doubles do not touch that buffer)
//   integers  integers(lo, hi) with rng = hi - 1 - lo: nothing drawn for rng == 0, else Lemire's method on uint32 words
//   jump      state_{n+k} = A_k state_n + G_k inc with A_k = a^k, G_k = (a^k - 1) / (a - 1): a lane can start at its own draw
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NPS_HD __host__ __device__ inline
#else
#define NPS_HD inline
#endif

namespace dcm {
namespace nps {

typedef unsigned __int128 u128;

constexpr u128 make128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | (u128)lo; }
constexpr u128 MULT = make128(2549297995355413924ULL, 4865540595714422341ULL);   // PCG_DEFAULT_MULTIPLIER_128

// ---------------------------------------------------------------------------------- SeedSequence
constexpr uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
constexpr uint32_t MIX_MULT_L = 0xca01f9ddu, MIX_MULT_R = 0x4973f715u;
constexpr int XSHIFT = 16;

NPS_HD uint32_t hashmix(uint32_t value, uint32_t& hash_const) {
    value ^= hash_const;
    hash_const *= MULT_A;
    value *= hash_const;
    value ^= value >> XSHIFT;
    return value;
}
NPS_HD uint32_t mix(uint32_t x, uint32_t y) {
    uint32_t r = MIX_MULT_L * x - MIX_MULT_R * y;
    r ^= r >> XSHIFT;
    return r;
}
// SeedSequence(seed).generate_state(4, np.uint64).  A uint64 seed has at most two entropy words, i.e. never more than the pool
// holds: the words beyond the seed's own hash as 0, which is also what the absent high word of a seed below 2^32 hashes as.
NPS_HD void seed_state(uint64_t seed, uint64_t v[4]) {
    const uint32_t entropy[4] = {(uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u};
    uint32_t pool[4];
    uint32_t hash_const = INIT_A;
    for (int i = 0; i < 4; i++) pool[i] = hashmix(entropy[i], hash_const);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            if (i != j) pool[j] = mix(pool[j], hashmix(pool[i], hash_const));
    uint32_t hash_b = INIT_B, w[8];
    for (int i = 0; i < 8; i++) {
        uint32_t d = pool[i & 3];
        d ^= hash_b;
        hash_b *= MULT_B;
        d *= hash_b;
        d ^= d >> XSHIFT;
        w[i] = d;
    }
    for (int i = 0; i < 4; i++) v[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

// ---------------------------------------------------------------------------------- PCG64
struct Pcg {
    u128 state, inc;
    uint32_t has_uint32, uinteger;   // the buffered high half of the last next64 a uint32 draw took
};

NPS_HD Pcg pcg_seed(uint64_t seed) {
    uint64_t v[4];
    seed_state(seed, v);
    const u128 initstate = make128(v[0], v[1]), initseq = make128(v[2], v[3]);
    Pcg p;
    p.inc = (initseq << 1) | 1u;
    p.state = p.inc;                          // state = 0; step
    p.state += initstate;
    p.state = p.state * MULT + p.inc;         // step
    p.has_uint32 = 0; p.uinteger = 0;
    return p;
}
NPS_HD uint64_t output(u128 state) {          // XSL-RR
    const uint64_t x = (uint64_t)(state >> 64) ^ (uint64_t)state;
    const unsigned rot = (unsigned)(state >> 122);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}
NPS_HD uint64_t next64(Pcg& p) {
    p.state = p.state * MULT + p.inc;
    return output(p.state);
}
NPS_HD double to_double(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }
NPS_HD double next_double(Pcg& p) { return to_double(next64(p)); }
NPS_HD uint32_t next_uint32(Pcg& p) {
    if (p.has_uint32) { p.has_uint32 = 0; return p.uinteger; }
    const uint64_t r = next64(p);
    p.has_uint32 = 1;
    p.uinteger = (uint32_t)(r >> 32);
    return (uint32_t)r;
}

// ---------------------------------------------------------------------------------- bounded integers (Lemire)
// A word u gives m = u * (rng + 1); it is rejected when the low half of m is below (2^32 - 1 - rng) % (rng + 1) (which is below
// rng + 1, so the reference's outer test `low half < rng + 1` only saves it the division).  Needs 1 <= rng <= 2^32 - 2.
NPS_HD uint32_t lemire_threshold(uint32_t rng) { return (0xFFFFFFFFu - rng) % (rng + 1u); }
NPS_HD bool lemire_accepts(uint32_t u, uint32_t rng, uint32_t threshold, uint32_t& value) {
    const uint64_t m = (uint64_t)u * (uint64_t)(rng + 1u);
    value = (uint32_t)(m >> 32);
    return (uint32_t)m >= threshold;
}
// Generator.integers(lo, lo + rng + 1) - lo, 0 <= rng <= 2^32 - 2.  rejections (nullable): counts the redraws.
NPS_HD uint32_t bounded(Pcg& p, uint32_t rng, uint32_t* rejections = nullptr) {
    if (rng == 0) return 0;
    const uint32_t threshold = lemire_threshold(rng);
    uint32_t value;
    while (!lemire_accepts(next_uint32(p), rng, threshold, value))
        if (rejections) ++*rejections;
    return value;
}

// ---------------------------------------------------------------------------------- jump-ahead
struct Jump { u128 A, G; };                    // k steps at once: state' = A state + G inc
constexpr Jump jump_coeffs(uint64_t k) {
    u128 acc_a = 1, acc_g = 0, cur_a = MULT, cur_g = 1;
    while (k) {
        if (k & 1) { acc_a *= cur_a; acc_g = acc_g * cur_a + cur_g; }
        cur_g = (cur_a + 1) * cur_g;
        cur_a *= cur_a;
        k >>= 1;
    }
    return Jump{acc_a, acc_g};
}
NPS_HD u128 jump(u128 state, u128 inc, const Jump& j) { return j.A * state + j.G * inc; }

}  // namespace nps
}  // namespace dcm
