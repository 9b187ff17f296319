// gpuntt/rns/bfv_encode.cuh -- BFV batching: the slot <-> coefficient map of a plaintext (extension: no counterpart in
// the reference).  DESIGN.md 3.24; the kernel is in csrc/bfv_encode.hip.
//
// THE SLOT CONVENTION, stated once.  N = 2^n_power, m = 2 N; t is prime with t = 1 (mod 2 N); psi is the 2N-th root
// of unity modulo t that the caller's forward table was built from.  A plaintext a(X) in Z_t[X]/(X^N + 1) holds N
// slots, a 2 x N/2 matrix: slot (r, c), r in {0, 1}, c in [0, N/2), has the linear index r N/2 + c and holds
//   a(psi^e(r, c)),   e(0, c) = 5^c mod 2N,   e(1, c) = 2N - (5^c mod 2N).
// GPU_NTT writes a(psi^(2 brev_n(i) + 1)) at place i (ntt_merge/galois.cuh), so slot (r, c) stands at
//   pos(r, c) = brev_n((e(r, c) - 1) / 2)                                         -- bfv_slot_position below.
// The generator is 5, as in GaloisElementForRotation, so on the slots
//   * sigma_k with k = 5^s mod 2N (GaloisElementForRotation(s)) rotates BOTH rows LEFT by s:
//       new[r][c] = old[r][(c + s) mod N/2]
//   * k = 2N - 1 (GaloisElementForConjugation) swaps the two rows
//   * the negacyclic product modulo t is the slot-wise product
// and GPU_Automorphism_NTT's index formula agrees with all three (tests/test_bfv_encode_host.py checks each by brute
// force: Horner evaluation and the coefficient-domain sigma_k).  pos is a bijection onto [0, N).  n_power = 1 (one
// column) is legal.
//
// BfvBatchEncoder<T>(t, n_power, forward_table, inverse_table, n_inverse, batch_hint, stream, workspace)
//   t: the Modulus<T> of the plaintext modulus; the tables: the caller's tables modulo t on the device exactly as
//   GPU_NTT / GPU_INTT take them for X_N_plus (they must outlive the plan, as for NTTPlan); n_inverse: the host value
//   N^-1 mod t.  The plan builds its two NTTPlan<T> (forward and inverse modulo t) and stores both uint32 maps --
//   to_position[N], indexed by slot, and to_slot[N], its inverse, derived on the host in exact integers -- in
//   workspace_bytes(n_power) bytes of device memory (nullptr: the plan allocates and owns it).  The constructor waits
//   for `stream` once for the maps and once in each NTTPlan; no call waits afterwards.
//   std::invalid_argument: (t - 1) mod 2N != 0 ("Plaintext modulus does not support batching!"), a modulus that is not
//   the Modulus<T> of its value ("Invalid modulus!"), n_power outside [1, 28] ("Invalid n_power range!"), a missing
//   table ("null pointer argument").  Primality of t is the caller's business, as it is for the transforms.
//
//   encode(values, plain, count):  values = T[count][N], any word, read modulo t, indexed by slot; plain = T[count][N],
//     the coefficients modulo t, canonical.  DEFINITION: w[p][pos(slot)] = values[p][slot] mod t, then GPU_INTT modulo t
//     in place.  What runs: ONE launch of bfv_slot_permute in gather form (plain[p][i] = values[p][to_slot[i]] mod t:
//     contiguous writes, the map read once), then the inverse plan.  No scratch.  values must not overlap plain.
//   decode(plain, values, count, scratch):  the inverse.  GPU_NTT modulo t from plain into the scratch (plain is left
//     untouched and must hold canonical words, as for any transform), then ONE bfv_slot_permute gathers
//     values[p][slot] = scratch[p][to_position[slot]].  scratch_bytes(count) = T[count][N], 256-byte aligned, owned by
//     the caller.
//   Both calls allocate nothing, never synchronise, run on one stream and can be captured into a hipGraph as they are;
//   count = 0 launches nothing.  std::invalid_argument, before anything is launched: a null pointer, values overlapping
//   plain or the scratch overlapping either ("encode input and output overlap!" / "decode input and output overlap!" /
//   "The scratch overlaps an operand!"), a scratch that is not 256-byte aligned ("The scratch is not 256-byte
//   aligned!"), count < 0 or beyond the grid and int limits ("Invalid count!").
//
// A plaintext that multiplies a ciphertext -- an operand of KeySwitchPlan::multiply_plain, a diagonal of
// rotate_hoisted_sum / linear_transform_bsgs -- goes on through KeySwitchPlan::lift_centred (rns/key_switch.cuh,
// "Plaintext operands"): centred modulo t, so that it multiplies the noise by at most t / 2 and not by t.
#pragma once

#include <cstddef>
#include <cstdint>

#include "gpuntt/common/common.cuh"
#include "gpuntt/common/modular_arith.cuh"
#include "gpuntt/common/nttparameters.cuh"
#include "gpuntt/ntt_merge/galois.cuh"

namespace gpuntt
{
    // pos(r, c) for the linear slot index r N/2 + c < N: where GPU_NTT's output holds the slot.  Walks the c powers of
    // 5 (a host loop for one slot; bfv_slot_maps fills all N in one walk).  Products wrap in 32 bits, exact because 2N
    // divides 2^32
    __host__ __device__ __forceinline__ std::uint32_t bfv_slot_position(std::uint32_t slot, int n_power)
    {
        const std::uint32_t mask = (2u << n_power) - 1u, half = (1u << n_power) >> 1;
        const std::uint32_t c = slot & (half - 1u); // n_power >= 1: half >= 1
        std::uint32_t e = 1u;
        for (std::uint32_t i = 0; i < c; i++)
            e = (e * 5u) & mask;
        if (slot >= half)
            e = (mask + 1u - e) & mask; // 2N - 5^c
        return galois_brev((e - 1u) >> 1, n_power);
    }

    // host only (no GPU): to_position[slot] = pos(slot) and to_slot[pos(slot)] = slot, N entries each.
    // std::invalid_argument: n_power outside [1, 28], a null pointer
    void bfv_slot_maps(int n_power, std::uint32_t* to_position_host, std::uint32_t* to_slot_host);

    template <typename T> class BfvBatchEncoder
    {
      public:
        static size_t workspace_bytes(int n_power);
        static size_t scratch_bytes(int n_power, int count); // decode: T[count][N], 256-byte aligned

        BfvBatchEncoder(Modulus<T> plain_modulus, int n_power, const Root<T>* forward_table_device,
                        const Root<T>* inverse_table_device, Ninverse<T> n_inverse_host, int batch_hint, stream_t stream,
                        void* workspace_device = nullptr);
        ~BfvBatchEncoder();
        BfvBatchEncoder(const BfvBatchEncoder&) = delete;
        BfvBatchEncoder& operator=(const BfvBatchEncoder&) = delete;

        void encode(const T* device_values, T* device_plain, int count, stream_t stream) const;
        void decode(const T* device_plain, T* device_values, int count, void* scratch_device, stream_t stream) const;

        size_t scratch_bytes(int count) const;
        int n_power() const;
        Modulus<T> plain_modulus() const;
        bool owns_workspace() const; // false: the plan lives in the caller's workspace and has allocated nothing

      private:
        struct Impl;
        Impl* p_;
    };
} // namespace gpuntt
