// inner_product_internal.hpp -- the device arithmetic of the RNS inner product, shared by inner_product.hip and
// hoisted_rotation.hip (the inner products that permute while they multiply): the exact three-word accumulator and the
// three-product fold, over the Shoup product of rns_arith.hpp.  One copy, so all kernels compute the same words (DESIGN.md
// 3.11, 3.13).
#pragma once

#include <hip/hip_runtime.h>

#include "gpuntt/rns/inner_product.cuh"
#include "rns_arith.hpp"

namespace gpuntt
{
    namespace kern
    {
        // the key limb of every modulus, as a kernel argument: read at blockIdx.y, a scalar load
        struct IpLimbs
        {
            unsigned char v[INNERPROD_MAX_MODULI];
        };

        // RnsWide, rns_mulhi, rns_shoup: rns_arith.hpp

        __device__ __forceinline__ Data32 ip_addc(Data32 a, Data32 b, Data32 cin, Data32* cout)
        {
            return __builtin_addc(a, b, cin, cout);
        }
        __device__ __forceinline__ Data64 ip_addc(Data64 a, Data64 b, Data64 cin, Data64* cout)
        {
            return __builtin_addcl(a, b, cin, cout);
        }

        template <typename T> struct IpAcc
        {
            T lo, hi;
            unsigned carry;
            // += x * y, exact
            __device__ __forceinline__ void mac(T x, T y)
            {
                using W2 = typename RnsWide<T>::type;
                const W2 p = static_cast<W2>(x) * y;
                T k0, k1;
                lo = ip_addc(lo, static_cast<T>(p), T(0), &k0);
                hi = ip_addc(hi, static_cast<T>(p >> (8 * sizeof(T))), k0, &k1);
                carry += static_cast<unsigned>(k1);
            }
        };

        // the plan's constants of modulus m, from the workspace image of InnerProductPlan: six arrays of M words (q,
        // 2^W mod q and its Shoup companion, 2^2W mod q and its companion, the companion of 1), read through the
        // CONSTANT address space -- nothing writes the workspace while a call runs, and a load from that address space
        // at a wave-uniform address is a scalar load
        template <typename T> struct IpFold
        {
            T q, t1, t1p, t2, t2p, onep;
            __device__ __forceinline__ IpFold(const T* consts, int M, unsigned m)
            {
                using CP = const T __attribute__((address_space(4)))*;
                const CP k = (CP) (consts);
                q = k[m], t1 = k[M + m], t1p = k[2 * M + m], t2 = k[3 * M + m], t2p = k[4 * M + m], onep = k[5 * M + m];
            }
            // (h [2^W]_q + c [2^2W]_q + l), three exact Shoup products, each canonical: the sum is below 3 q < 2^W
            __device__ __forceinline__ T sum(const IpAcc<T>& s) const
            {
                T x = rns_shoup<T>(s.hi, t1, t1p, q);
                x += rns_shoup<T>(static_cast<T>(s.carry), t2, t2p, q);
                x += rns_shoup<T>(s.lo, T(1), onep, q);
                return x;
            }
            // x < 3 q -> x mod q
            __device__ __forceinline__ T reduce(T x) const
            {
                x = x >= q ? x - q : x;
                return x >= q ? x - q : x;
            }
        };
    } // namespace kern
} // namespace gpuntt
