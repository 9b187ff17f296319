// relinearize_sum_internal.hpp -- what key_switch.hip needs of relinearize_sum.hip: the kernel argument of one
// multiply_relinearize_sum call and the launchers of tensor_top_sum and inner_product_tensor_sum.
#pragma once

#include <hip/hip_runtime.h>

#include "gpuntt/rns/key_switch.cuh"
#include "relinearize_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // RelinArgs plus the 2 * terms operand pointers, still ONE kernel argument: nothing is copied to the device per
        // call and a captured graph keeps nothing alive.  The pointers are read at the wave-uniform t: scalar loads.
        // 1608 bytes for u64, 1096 for u32, inside the 4 KiB argument segment with the kernels' other 64 bytes
        template <typename T> struct RelinSumArgs
        {
            RelinArgs<T> r;
            const T* x[KEYSWITCH_MAX_TERMS]; // x_t, y_t: T[2][count][L][N]
            const T* y[KEYSWITCH_MAX_TERMS];
            int terms;
        };
        static_assert(sizeof(RelinSumArgs<Data64>) == 1608 && sizeof(RelinSumArgs<Data32>) == 1096,
                      "RelinSumArgs has to stay inside the 4 KiB argument segment");
        static_assert(2 * KEYSWITCH_MAX_TERMS <= INNERPROD_MAX_DIGITS,
                      "the cross term of the definition is one InnerProductPlan call with D = 2 * terms");

        // inputs per pass over the key of inner_product_tensor_sum, at most.  Blocks of 2 and of 4 both keep 3 waves per
        // SIMD for u64; timed against each other, 2 was the faster (DESIGN.md 3.16 has the register table and the A/B)
        constexpr int RELIN_SUM_BLOCK = 2;
    } // namespace kern

    namespace host
    {
        // args.x[t], args.y[t]: T[2][count][L][N], t < args.terms; d2: T[count][L][N]; consts: the workspace image of
        // InnerProductPlan for the M moduli of the full base.  One launch.  enqueue false: only the checks.  Throws
        // std::invalid_argument beyond the grid limits
        template <typename T>
        void relin_sum_top_launch(T* d2, const T* consts, const kern::RelinSumArgs<T>& args, int count, int L, int M,
                                  int n_power, bool enqueue, hipStream_t stream);

        // a: T[D][count][M][N], key: T[D_key][2][KM][N], acc: T[2][count][M][N].  One launch.  enqueue false: only the
        // checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void relin_sum_inner_launch(const T* a, const T* key, T* acc, const T* consts, const kern::RelinSumArgs<T>& args,
                                    int D, int count, int L, int M, int KM, int n_power, bool enqueue,
                                    hipStream_t stream);
    } // namespace host
} // namespace gpuntt
