// gpuntt/ntt_merge/galois.cuh -- Galois automorphisms (extension: no counterpart in the reference).
//
// The ring automorphism sigma_k: a(X) -> a(X^k), k odd, in Z_q[X]/(X^N + 1) (X_N_plus) or Z_q[X]/(X^N - 1)
// (X_N_minus), N = 2^n_power.  It is what slot rotations and conjugation in CKKS / BFV / BGV are built from.
// The Galois element k is reduced mod 2N (X_N_plus) or mod N (X_N_minus); an even element is refused.
//
// Coefficient domain (natural order), gather form:
//   X_N_plus : j = (k^-1 * i) mod 2N;  out[i] = j < N ? in[j] : (q - in[j - N]) mod q   (0 stays 0)
//   X_N_minus: out[(k * j) mod N] = in[j]                                               (no sign)
// NTT domain, in the order GPU_NTT writes (slot i of a negacyclic transform holds a(psi^(2 brev_n(i) + 1)), slot i
// of a cyclic one a(omega^brev_n(i))) -- a pure permutation, no modulus:
//   X_N_plus : out[i] = in[brev_n(((k * (2 brev_n(i) + 1)) mod 2N - 1) / 2)]
//   X_N_minus: out[i] = in[brev_n((k * brev_n(i)) mod N)]
// so that NTT(sigma_k(a)) == GPU_Automorphism_NTT(NTT(a)) and INTT(GPU_Automorphism_NTT(NTT(a))) == sigma_k(a).
//
//   * layout: in is T[batch][N] (PerPolynomial), out is T[galois_count][batch][N]: element g of galois_elts_host
//     writes out + g * batch * N.  One call applies 1..64 elements to one input (hoisting: the input is read once)
//   * the elements travel as kernel arguments: no scratch, no preparation launch, no allocation -- one kernel
//     launch per call, so a call can be captured into a hipGraph as it is
//   * in and out must not overlap (a permutation cannot run in place across workgroups)
//   * RNS form: polynomial p uses modulus_device[p % mod_count], as in GPU_NTT
//   * throws std::invalid_argument for overlapping buffers, an even (or zero) element, galois_count outside
//     [1, 64], n_power outside [1, 28] ("Invalid n_power range!") or an unknown reduction polynomial;
//     HipException on a failed launch.  Asynchronous on `stream`.
//   * unsigned types only (Data32, Data64).  The 4-step output order (GPU_4STEP_NTT) is not supported: the NTT-domain
//     call expects the Merge order of GPU_NTT / NTTPlan.
#pragma once

#include <cstdint>

#include "gpuntt/ntt_merge/ntt.cuh"

namespace gpuntt
{
    constexpr int GALOIS_MAX_COUNT = 64;

    // ---- the index maps (host and device): the source of output slot i --------------------------------------------
    // bit reversal of the low `bits` bits of v (bits in [1, 31])
    __host__ __device__ __forceinline__ std::uint32_t galois_brev(std::uint32_t v, int bits)
    {
        return __builtin_bitreverse32(v) >> (32 - bits);
    }

    // NTT domain: the slot of `in` that output slot i reads.  k odd; products wrap in 32 bits, exact because 2N
    // divides 2^32.
    __host__ __device__ __forceinline__ std::uint32_t galois_ntt_source(std::uint32_t i, std::uint32_t k, int n_power,
                                                                       bool negacyclic)
    {
        if (negacyclic)
        {
            const std::uint32_t mask = (2u << n_power) - 1u;
            const std::uint32_t e = ((k * (2u * galois_brev(i, n_power) + 1u)) & mask) >> 1;
            return galois_brev(e, n_power);
        }
        const std::uint32_t mask = (1u << n_power) - 1u;
        return galois_brev((k * galois_brev(i, n_power)) & mask, n_power);
    }

    // k^-1 mod 2^32 for odd k (Newton: every step doubles the correct low bits; k * k = 1 mod 8 to start), so also
    // mod every power of two
    __host__ __device__ __forceinline__ std::uint32_t galois_inverse(std::uint32_t k)
    {
        std::uint32_t x = k;
        for (int i = 0; i < 4; i++)
            x *= 2u - k * x;
        return x;
    }

    // coefficient domain: the source of output coefficient i given k_inv = k^-1 (mod 2N for X_N_plus, mod N for
    // X_N_minus).  X_N_plus returns j in [0, 2N): j >= N means "negate in[j - N]"; X_N_minus returns j in [0, N).
    __host__ __device__ __forceinline__ std::uint32_t galois_coeff_source(std::uint32_t i, std::uint32_t k_inv,
                                                                         int n_power, bool negacyclic)
    {
        const std::uint32_t mask = negacyclic ? (2u << n_power) - 1u : (1u << n_power) - 1u;
        return (k_inv * i) & mask;
    }

    // ---- Galois elements ---------------------------------------------------------------------------------------------
    // 5^steps mod 2N (negative steps: the inverse), the element that rotates CKKS / BGV slots by `steps`
    std::uint32_t GaloisElementForRotation(int steps, int n_power);
    // 2N - 1: complex conjugation of CKKS slots (the row swap of BGV / BFV)
    std::uint32_t GaloisElementForConjugation(int n_power);

    // ---- NTT domain: input is GPU_NTT's output, same layout; no modulus ---------------------------------------------
    template <typename T>
    __host__ void GPU_Automorphism_NTT(const T* device_in, T* device_out, const std::uint32_t* galois_elts_host,
                                       int galois_count, int n_power, ReductionPolynomial reduction_poly,
                                       int batch_size, stream_t stream);

    // ---- coefficient domain, single modulus ---------------------------------------------------------------------------
    template <typename T>
    __host__ void GPU_Automorphism(const T* device_in, T* device_out, const std::uint32_t* galois_elts_host,
                                   int galois_count, Modulus<T> modulus, int n_power,
                                   ReductionPolynomial reduction_poly, int batch_size, stream_t stream);

    // ---- coefficient domain, RNS: polynomial p uses modulus_device[p % mod_count] -----------------------------------
    template <typename T>
    __host__ void GPU_Automorphism(const T* device_in, T* device_out, const std::uint32_t* galois_elts_host,
                                   int galois_count, const Modulus<T>* modulus_device, int mod_count, int n_power,
                                   ReductionPolynomial reduction_poly, int batch_size, stream_t stream);

} // namespace gpuntt
