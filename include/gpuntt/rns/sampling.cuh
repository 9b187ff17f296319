// gpuntt/rns/sampling.cuh -- counter-based samplers for key material (extension: no counterpart in the reference).
//
// NOT A CRYPTOGRAPHIC GENERATOR.  Philox4x32-10 is a statistical generator: these samplers are for tests, benchmarks
// and reproducible experiments.  Every call of KeySwitchPlan that consumes randomness (lift_small, generate_keys,
// encrypt_symmetric: rns/key_switch.cuh) takes it as BUFFERS, so a production caller fills them from its own generator.
//
// Everything here is a pure function of (seed, stream, word index): the result does not depend on the launch shape, can
// be restated in a few lines of Python (tests/sampling_exact.py) and is capturable into a hipGraph.  No global state.
//
//   philox4x32_10(ctr[4], key[2]):  the standard Philox4x32 with ten rounds (Salmon et al., Random123): multipliers
//     0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85.  __host__ __device__ inline: the same text
//     serves the kernels and the host references.
//
//   sample_uniform<T>(out, moduli_host, mod_count, n_power, stacks, stack_stride_words, seed, stream_id, hip_stream):
//     out = T[stacks][mod_count][N]; stack s starts at s * stack_stride_words, stack_stride_words >= mod_count * N -- so
//     the `a` planes of a switching key T[D][2][M][N] are filled in place with out = key + M N, stacks = D, stride 2 M N.
//     moduli_host = mod_count HOST values q >= 1 (not necessarily prime, not necessarily distinct), 1 <= mod_count <= 256.
//     DEFINITION of the word of stack s, limb m, column j, with q = moduli_host[m] of bit length b:
//       w = (s * mod_count + m) * N + j       -- 64 bits, over the DENSE index, not the stride
//       for candidate c = 0 .. 31:  B = philox4x32_10(ctr = (w_lo, w_hi, c div k, stream_id), key = (seed_lo, seed_hi))
//         W = 64: k = 2 candidates per block, candidate = B[2 (c mod 2)] | B[2 (c mod 2) + 1] << 32
//         W = 32: k = 4 candidates per block, candidate = B[c mod 4]
//         r = candidate & (2^b - 1); the first r < q is the word
//       no candidate accepted (probability <= 2^-32): the word is the last r mod q.
//     The loop is bounded: no lane ever spins.  ONE launch, every word written once, 16 bytes per lane where `out` and
//     the stride allow it.  Allocates nothing, never synchronises; stacks = 0 launches nothing.
//     std::invalid_argument, before the launch: a null pointer, mod_count outside [1, 256], a modulus 0, n_power outside
//     [1, 28], stacks < 0, a stride below mod_count * N, a size beyond one launch's grid.
//
//   sample_small(out, polys, n_power, distribution, seed, stream_id, hip_stream):  out = int32[polys][N], w = p N + j,
//     ONE block B = philox4x32_10((w_lo, w_hi, 0, stream_id), (seed_lo, seed_hi)) per word.
//       ternary: scan the 64 two-bit fields of B from bit 0 of B[0] upward; the first field v != 3 gives v - 1 (uniform
//                on {-1, 0, 1}); all 64 fields 3: the value is 0
//       cbd21:   x = B[0] | B[1] << 32; popcount(x & (2^21 - 1)) - popcount((x >> 21) & (2^21 - 1)): the centred
//                binomial of 21 coin pairs, variance 10.5 (sigma ~ 3.24), |value| <= 21
//     ONE launch; allocates nothing, never synchronises; polys = 0 launches nothing.
//
//   reference_philox, reference_sample_uniform, reference_sample_small:  HOST only (no GPU), built from the same inline
//     functions; what tests and examples compare the kernels with, never a GPU fall-back.  The uniform reference takes
//     max_candidates (>= 1) so that the `r mod q` tail can be reached; the device always uses 32.
#pragma once

#include <cstddef>
#include <cstdint>

#include "gpuntt/common/common.cuh"

namespace gpuntt
{
    constexpr int SAMPLE_MAX_CANDIDATES = 32; // candidates per uniform word on the device
    constexpr int SAMPLE_MAX_MODULI = 256;    // moduli of one sample_uniform call (KeySwitchPlan's key_mod_count limit)

    enum class SmallDistribution : int
    {
        ternary = 0,
        cbd21 = 1
    };

    struct PhiloxBlock
    {
        std::uint32_t v[4];
    };

    __host__ __device__ inline PhiloxBlock philox4x32_10(const std::uint32_t (&ctr)[4], const std::uint32_t (&key)[2])
    {
        std::uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
        for (int round = 0; round < 10; round++)
        {
            const std::uint64_t p0 = static_cast<std::uint64_t>(0xD2511F53u) * c0;
            const std::uint64_t p1 = static_cast<std::uint64_t>(0xCD9E8D57u) * c2;
            const std::uint32_t n0 = static_cast<std::uint32_t>(p1 >> 32) ^ c1 ^ k0;
            const std::uint32_t n2 = static_cast<std::uint32_t>(p0 >> 32) ^ c3 ^ k1;
            c1 = static_cast<std::uint32_t>(p1), c3 = static_cast<std::uint32_t>(p0), c0 = n0, c2 = n2;
            k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
        }
        return PhiloxBlock{{c0, c1, c2, c3}};
    }

    // 2^b - 1 for the bit length b of q >= 1
    template <typename T> __host__ __device__ inline T sample_mask(T q)
    {
        T mask = q;
        for (unsigned s = 1; s < 8 * sizeof(T); s *= 2)
            mask |= mask >> s;
        return mask;
    }

    // one word of sample_uniform ("DEFINITION" above); mask = sample_mask(q), max_candidates >= 1
    template <typename T>
    __host__ __device__ inline T sample_uniform_word(std::uint64_t w, T q, T mask, std::uint64_t seed,
                                                     std::uint32_t stream_id, int max_candidates)
    {
        constexpr int k = sizeof(T) == 8 ? 2 : 4;
        const std::uint32_t key[2] = {static_cast<std::uint32_t>(seed), static_cast<std::uint32_t>(seed >> 32)};
        T r = 0;
        for (int c = 0; c < max_candidates; c += k)
        {
            const std::uint32_t ctr[4] = {static_cast<std::uint32_t>(w), static_cast<std::uint32_t>(w >> 32),
                                          static_cast<std::uint32_t>(c / k), stream_id};
            const PhiloxBlock b = philox4x32_10(ctr, key);
#pragma unroll
            for (int i = 0; i < k; i++) // constant indices: the block stays in registers
                if (c + i < max_candidates)
                {
                    T cand;
                    if constexpr (sizeof(T) == 8)
                        cand = static_cast<T>(b.v[2 * i]) | static_cast<T>(b.v[2 * i + 1]) << 32;
                    else
                        cand = b.v[i];
                    r = cand & mask;
                    if (r < q)
                        return r;
                }
        }
        return r % q;
    }

    // one word of sample_small ("DEFINITION" above)
    __host__ __device__ inline std::int32_t sample_small_word(std::uint64_t w, SmallDistribution distribution,
                                                              std::uint64_t seed, std::uint32_t stream_id)
    {
        const std::uint32_t key[2] = {static_cast<std::uint32_t>(seed), static_cast<std::uint32_t>(seed >> 32)};
        const std::uint32_t ctr[4] = {static_cast<std::uint32_t>(w), static_cast<std::uint32_t>(w >> 32), 0u, stream_id};
        const PhiloxBlock b = philox4x32_10(ctr, key);
        if (distribution == SmallDistribution::cbd21)
        {
            const std::uint64_t x = static_cast<std::uint64_t>(b.v[0]) | static_cast<std::uint64_t>(b.v[1]) << 32;
            const std::uint64_t m21 = (1ull << 21) - 1;
            return __builtin_popcountll(x & m21) - __builtin_popcountll((x >> 21) & m21);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const std::uint32_t x = b.v[i];
            const std::uint32_t other = ~(x & (x >> 1)) & 0x55555555u; // bit 2f set: field f is not 3
            if (other != 0)
                return static_cast<std::int32_t>((x >> __builtin_ctz(other)) & 3u) - 1;
        }
        return 0;
    }

    template <typename T>
    void sample_uniform(T* device_out, const T* moduli_host, int mod_count, int n_power, int stacks,
                        std::uint64_t stack_stride_words, std::uint64_t seed, std::uint32_t stream_id, stream_t stream);

    void sample_small(std::int32_t* device_out, int polys, int n_power, SmallDistribution distribution,
                      std::uint64_t seed, std::uint32_t stream_id, stream_t stream);

    // host only (no GPU)
    void reference_philox(const std::uint32_t ctr[4], const std::uint32_t key[2], std::uint32_t out[4]);
    template <typename T>
    void reference_sample_uniform(T* out_host, const T* moduli_host, int mod_count, int n_power, int stacks,
                                  std::uint64_t stack_stride_words, std::uint64_t seed, std::uint32_t stream_id,
                                  int max_candidates = SAMPLE_MAX_CANDIDATES);
    void reference_sample_small(std::int32_t* out_host, int polys, int n_power, SmallDistribution distribution,
                                std::uint64_t seed, std::uint32_t stream_id);
} // namespace gpuntt
