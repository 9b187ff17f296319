// relinearize_internal.hpp -- what key_switch.hip needs of relinearize.hip: the kernel argument of one
// multiply_relinearize call and the launchers of tensor_top and inner_product_tensor; and what relinearize_sum.hip shares
// with it: the grid and the choice of the loader.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <stdexcept>

#include "gpuntt/rns/inner_product.cuh"
#include "inner_product_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // Everything of a call that is not a buffer travels as ONE kernel argument (as HoistArgs does): no device copy,
        // nothing a captured graph has to keep alive.  1088 bytes for u64, inside the 4 KiB argument segment
        template <typename T> struct RelinArgs
        {
            IpLimbs limbs;                         // the key limb of every modulus of the full base
            T p_mod_q[INNERPROD_MAX_MODULI];       // P mod q_m, m < L ...
            T p_mod_q_shoup[INNERPROD_MAX_MODULI]; // ... and floor((P mod q_m) 2^W / q_m)
        };
        static_assert(sizeof(RelinArgs<Data64>) == 1088 && sizeof(RelinArgs<Data32>) == 576,
                      "RelinArgs has to stay inside the 4 KiB argument segment");
    } // namespace kern

    namespace host
    {
        // lanes per workgroup and column tiles per polynomial for V columns per lane; throws when `rows` of them
        // pass what HIP launches in one dimension
        struct RelinGrid
        {
            unsigned nt, tiles, blocks;
        };
        inline RelinGrid relin_grid(int n_power, int V, unsigned long long rows)
        {
            const unsigned long long lanes = (1ull << n_power) / V; // per polynomial
            unsigned nt = 64;
            while (nt < kern::IP_NT && nt < lanes)
                nt *= 2;
            const unsigned long long tiles = (lanes + nt - 1) / nt;
            const unsigned long long blocks = tiles * rows;
            if (blocks * nt > 0xFFFFFFFFull) // HIP caps a launch at 2^32 - 1 work-items per dimension
                throw std::invalid_argument("Invalid count!");
            return RelinGrid{nt, static_cast<unsigned>(tiles), static_cast<unsigned>(blocks)};
        }
        // a 16-byte group must stay inside one polynomial and be aligned (every stride is a multiple of N words);
        // bits: the OR of every base pointer
        template <typename T> bool relin_wide_bits(int n_power, uintptr_t bits)
        {
            return n_power >= (sizeof(T) == 8 ? 1 : 2) && (bits & 15u) == 0;
        }
        template <typename T> bool relin_wide(int n_power, std::initializer_list<const void*> bases)
        {
            uintptr_t bits = 0;
            for (const void* p : bases)
                bits |= reinterpret_cast<uintptr_t>(p);
            return relin_wide_bits<T>(n_power, bits);
        }

        // x1, y1: T[count][L][N] (the second components of the two operands, NTT form), d2: T[count][L][N]; consts: the
        // workspace image of InnerProductPlan for the M moduli of the full base.  One launch.  enqueue false: only the
        // checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void relin_top_launch(const T* x1, const T* y1, T* d2, const T* consts, int count, int L, int M, int n_power,
                              bool enqueue, hipStream_t stream);

        // a: T[D][count][M][N], key: T[D_key][2][KM][N], x, y: T[2][count][L][N], acc: T[2][count][M][N].  One launch.
        // enqueue false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void relin_inner_launch(const T* a, const T* key, T* acc, const T* consts, const T* x, const T* y,
                                const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                bool enqueue, hipStream_t stream);

        // inner_product_seeded: a, key, acc as above; c01: T[2][count][L][N] in NTT form, any word.  One launch.
        // enqueue false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void relin_seeded_launch(const T* a, const T* key, T* acc, const T* consts, const T* c01,
                                 const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                 bool enqueue, hipStream_t stream);
    } // namespace host
} // namespace gpuntt
