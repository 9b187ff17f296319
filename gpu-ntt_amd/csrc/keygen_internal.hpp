// keygen_internal.hpp -- what key_switch.hip needs of keygen.hip: the kernel argument of one generate_keys /
// encrypt_symmetric call and the launchers of lift_small and keygen_combine.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpuntt/rns/inner_product.cuh"
#include "gpuntt/rns/key_switch.cuh"
#include "inner_product_internal.hpp"
#include "relinearize_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // Everything of a call that is not a buffer travels as ONE kernel argument (as RelinArgs does): no device copy,
        // nothing a captured graph has to keep alive.  1024 bytes for u64, inside the 4 KiB argument segment
        template <typename T> struct KeygenArgs
        {
            T* group[KEYGEN_MAX_KEYS];     // generate_keys: the keys; encrypt_symmetric: group[0] = out
            T mult[INNERPROD_MAX_MODULI];  // the multiplier of the gadget term of limb m: P mod q_m, or 1 (the message)
        };
        static_assert(sizeof(KeygenArgs<Data64>) == 1024 && sizeof(KeygenArgs<Data32>) == 768,
                      "KeygenArgs has to stay inside the 4 KiB argument segment");

        // Where keygen_combine finds its words, all in words.  A call has `groups` groups of `rows` rows of B limbs:
        //   generate_keys:      group = key g, row = digit d, B = M:   row = 2 M N, a_at = M N, g_group = M N, g_row = 0
        //   encrypt_symmetric:  one group (out), row = ciphertext r, B = L:  row = L N, a_at = count L N, g_group = 0,
        //                       g_row = L N
        // E is dense: T[groups][rows][B][N].  alpha > 0: the gadget term is present on the limbs of digit `row` only
        // ([row alpha, min((row + 1) alpha, L))); alpha = 0: on every limb
        struct KeygenShape
        {
            unsigned long long row, a_at, g_group, g_row;
            int rows, B, L, alpha;
        };
    } // namespace kern

    namespace host
    {
        // small: int32[polys][N] -> out: T[polys][B][N], the canonical residue of every signed value under the first B
        // moduli of the fold image `consts` (stride M).  One launch.  enqueue false: only the checks
        template <typename T>
        void keygen_lift_launch(const std::int32_t* small, T* out, const T* consts, int polys, int B, int M, int n_power,
                                bool enqueue, hipStream_t stream);

        // words: T[polys][N], any word, read modulo t and centred -> out: T[polys][B][N], the canonical residues under the
        // first B moduli of the fold image.  t in [2, 2^(W-1)).  One launch.  enqueue false: only the checks
        template <typename T>
        void lift_centred_launch(const T* words, T* out, const T* consts, T t, int polys, int B, int M, int n_power,
                                 bool enqueue, hipStream_t stream);

        // ct, out: T[2][count][L][N] (out may be exactly ct), pt: T[plain_count][L][N], plain_count 1 (shared) or count.
        // One launch.  enqueue false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void multiply_plain_launch(const T* ct, const T* pt, T* out, const T* consts, int count, int plain_count, int L,
                                   int M, int n_power, bool enqueue, hipStream_t stream);

        // keygen_combine: for every group g, row d, limb m < B and column j
        //   group[g][d * row + m N + j] = (E[g][d][m][j] - a * s[m][j] + [gadget on] mult[m] * gadget[...]) mod q_m
        // with a = group[g][d * row + a_at + m N + j]; gadget may be nullptr (no gadget term at all).  One launch.
        // enqueue false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void keygen_combine_launch(const T* e, const T* s, const T* gadget, const kern::KeygenArgs<T>& args,
                                   const kern::KeygenShape& shape, int groups, const T* consts, int M, int n_power,
                                   bool enqueue, hipStream_t stream);
    } // namespace host
} // namespace gpuntt
