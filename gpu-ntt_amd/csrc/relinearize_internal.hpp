// relinearize_internal.hpp -- what key_switch.hip needs of relinearize.hip: the kernel argument of one
// multiply_relinearize call and the launchers of tensor_top and inner_product_tensor.
#pragma once

#include <hip/hip_runtime.h>

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
    } // namespace host
} // namespace gpuntt
