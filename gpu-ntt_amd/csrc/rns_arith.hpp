// rns_arith.hpp -- the word arithmetic every RNS kernel shares (base_conversion_internal.hpp, inner_product_internal.hpp
// and through them key_switch.hip and hoisted_rotation.hip): the double-width type, the high product and the canonical
// Shoup product.  One copy, so all of them compute the same words.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>

#include "gpuntt/common/modular_arith.cuh"

namespace gpuntt
{
    namespace kern
    {
        template <typename T> struct RnsWide;
        template <> struct RnsWide<Data32>
        {
            using type = Data64;
        };
        template <> struct RnsWide<Data64>
        {
            using type = unsigned __int128;
        };

        // (plain C++, so that the kernels' text also compiles for the host: the emulators of tests/cpp)
        __device__ __forceinline__ constexpr int ip_min(int a, int b) { return a < b ? a : b; }

        __device__ __forceinline__ Data32 rns_mulhi(Data32 a, Data32 b) { return __umulhi(a, b); }
        __device__ __forceinline__ Data64 rns_mulhi(Data64 a, Data64 b) { return __umul64hi(a, b); }

        // (x * w) mod m, canonical, for ANY word x, w < m < 2^(W-1) and wp = floor(w 2^W / m): the quotient estimate
        // hi(x * wp) is floor(x w / m) or one less, so the remainder lies in [0, 2m)
        template <typename T> __device__ __forceinline__ T rns_shoup(T x, T w, T wp, T m)
        {
            const T r = x * w - rns_mulhi(x, wp) * m;
            return r >= m ? r - m : r;
        }
    } // namespace kern
} // namespace gpuntt
