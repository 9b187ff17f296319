// hoisted_sum_internal.hpp -- what key_switch.hip needs of hoisted_sum.hip: the kernel arguments of one
// rotate_hoisted_sum call and the launcher of inner_product_galois_sum.
#pragma once

#include "hoisted_rotation_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // HoistArgs plus the G weight pointers, still ONE kernel argument: 2632 bytes for u64, 2120 for u32, inside the
        // 4 KiB argument segment with the kernel's other 72 bytes
        template <typename T> struct HoistSumArgs
        {
            HoistArgs<T> h;
            const T* weight[GALOIS_MAX_COUNT]; // pt_g: T[M][N] over the full base, or nullptr (weight 1)
        };
        static_assert(sizeof(HoistSumArgs<Data64>) == 2632 && sizeof(HoistSumArgs<Data32>) == 2120,
                      "HoistSumArgs has to stay inside the 4 KiB argument segment");
    } // namespace kern

    namespace host
    {
        // log2 of the destination chunk of inner_product_galois_sum: one slot per lane, so at most 256 slots; the largest
        // power of two in [64, 256] with (D + 1) chunk word_bytes inside the LDS budget, at most N.  The test hook
        // keyswitch_hoist_chunk replaces the budget rule (not the caps at N, at 256 slots and at 64 KiB of LDS)
        int hoist_sum_chunk_log(size_t word_bytes, int D, int n_power);
        void keyswitch_set_hoist_sum_chunk(int v); // test hook: 0 = the rule above, 6 .. 13 = log2 of the chunk

        // a: T[D][count][M][N], c0: T[count][L][N] or nullptr, acc: T[2][count][M][N]; consts: the workspace image of
        // InnerProductPlan for the M moduli.  One launch; throws std::invalid_argument beyond the grid limits
        template <typename T>
        void hoist_sum_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistSumArgs<T>& args, int D,
                              int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream);
    } // namespace host
} // namespace gpuntt
