// decrypt_internal.hpp -- what key_switch.hip and bfv_multiply.hip need of decrypt.hip: the kernel arguments of
// bfv_scale_message and bfv_decode and the launchers of the four kernels; and what the host emulator
// (tests/cpp/emulate_decrypt.cpp) needs to call them.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "base_conversion_internal.hpp"
#include "gpuntt/rns/inner_product.cuh"
#include "inner_product_internal.hpp"
#include "relinearize_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // The constants of the plaintext modulus travel as ONE kernel argument each (as KeygenArgs does): they are no
        // part of the plan's workspace, so workspace_bytes and every older launch stay as they were.  An argument lives
        // in the kernel argument segment: read at a wave-uniform index it is a scalar load

        // bfv_scale_message: out_i = ((h - r) * [t^-1 mod q_i]) mod q_i, r = ((Q mod t) m + h) mod t, h = floor(t / 2)
        template <typename T> struct BfvScaleArgs
        {
            T t_inv[INNERPROD_MAX_MODULI];       // t^-1 mod q_i, i < L
            T t_inv_shoup[INNERPROD_MAX_MODULI]; // floor((t^-1 mod q_i) 2^W / q_i)
            T t, one_shoup_t;                    // t and floor(2^W / t): the Shoup companion of 1 modulo t
            T q_mod_t, q_mod_t_shoup;            // Q mod t and floor((Q mod t) 2^W / t)
            T half;                              // h
        };
        // bfv_decode: (a_i, r_i) = divmod(t y_i, q_i) by one Shoup quotient against floor(t 2^W / q_i)
        template <typename T> struct BfvDecodeArgs
        {
            T t_shoup[INNERPROD_MAX_MODULI]; // floor(t 2^W / q_i), i < L (t < q_i)
            T t, one_shoup_t;                // t and floor(2^W / t)
        };
        static_assert(sizeof(BfvScaleArgs<Data64>) == 1064 && sizeof(BfvDecodeArgs<Data64>) == 528,
                      "the arguments have to stay inside the 4 KiB argument segment");
    } // namespace kern

    namespace host
    {
        // decrypt_phase: ct: T[components][count][L][N], s: T[>= L][N], out: T[count][L][N] (may be exactly ct);
        // consts: the fold image (stride M).  One launch.  enqueue false: only the checks.  Throws
        // std::invalid_argument beyond the grid limits
        template <typename T>
        void decrypt_phase_launch(const T* ct, const T* s, T* out, const T* consts, int count, int components, int L,
                                  int M, int n_power, bool enqueue, hipStream_t stream);

        // encrypt_public_combine: pk: T[2][L][N], lifted: T[3][count][L][N] = (U, E0, E1) in NTT form, message:
        // T[count][L][N] or nullptr, out: T[2][count][L][N].  One launch, as above
        template <typename T>
        void encrypt_public_combine_launch(const T* pk, const T* lifted, const T* message, T* out, const T* consts,
                                           int count, int L, int M, int n_power, bool enqueue, hipStream_t stream);

        // bfv_scale_message: message: T[count][N], out: T[count][L][N]; consts: the fold image (stride M; q_i at i)
        template <typename T>
        void bfv_scale_message_launch(const T* message, T* out, const T* consts, const kern::BfvScaleArgs<T>& args,
                                      int count, int L, int n_power, bool enqueue, hipStream_t stream);

        // bfv_decode: x: T[stacks][L][N], message: T[stacks][N], noise_max: T[stacks] or nullptr; partials: nullptr
        // (noise_max zeroed by the caller, one atomicMax per workgroup) or T[stacks][tiles] -- at most
        // decode_partial_words(stacks, n_power) words -- and then a second launch, bfv_decode_merge, stores noise_max;
        // consts / up: the plan's run of constants and its {q} -> {b} image
        template <typename T>
        void bfv_decode_launch(const T* x, T* message, T* noise_max, T* partials, const T* consts,
                               const kern::BcOffsets& up, const kern::BfvDecodeArgs<T>& args, int stacks, int L,
                               int n_power, bool enqueue, hipStream_t stream);
        // the words of `partials` for either loader: the column tiles of the one-word loader, per stack
        inline size_t decode_partial_words(int stacks, int n_power)
        {
            const RelinGrid g = relin_grid(n_power, 1, 1);
            return static_cast<size_t>(stacks) * g.tiles;
        }
    } // namespace host
} // namespace gpuntt
