// bfv_multiply_sum_internal.hpp -- what bfv_multiply.hip needs of bfv_multiply_sum.hip: the kernel argument of one
// BfvMultiplyPlan::multiply_sum call and the launcher of bfv_tensor_sum.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>

#include "gpuntt/rns/bfv_multiply.cuh"
#include "relinearize_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // Which extended operand every term multiplies: slot s is T[2][count][M][N] at 2 * s * count * M * N words into
        // the operand region.  ONE kernel argument, as RelinSumArgs carries its pointers: nothing is copied to the device
        // per call and a captured graph keeps nothing alive.  The bytes are read at the wave-uniform t.  68 bytes
        struct BfvSumArgs
        {
            unsigned char x_slot[BFV_MAX_TERMS];
            unsigned char y_slot[BFV_MAX_TERMS];
            int terms;
        };
        static_assert(sizeof(BfvSumArgs) == 68, "BfvSumArgs travels by value with the kernel's other 40 bytes");
        static_assert(2 * BFV_MAX_TERMS <= INNERPROD_MAX_DIGITS,
                      "the cross term of the definition is one InnerProductPlan call with D = 2 * terms");
        static_assert(2 * BFV_MAX_TERMS <= 256, "a slot index is one byte");
    } // namespace kern

    namespace host
    {
        // e: the operand region T[slots][2][count][M][N], slots >= max(2, every index in args) + 1; d0, d1, d2 are written
        // over its first three component planes.  fold: the six arrays of M words IpFold reads.  One launch.  enqueue
        // false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void bfv_tensor_sum_launch(T* e, const T* fold, const kern::BfvSumArgs& args, int count, int M, int n_power,
                                   bool enqueue, hipStream_t stream);
    } // namespace host
} // namespace gpuntt
