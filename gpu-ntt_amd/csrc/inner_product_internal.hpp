// inner_product_internal.hpp -- the device arithmetic of the RNS inner product, shared by inner_product.hip,
// hoisted_rotation.hip (the inner products that permute while they multiply) and relinearize.hip (the one that multiplies
// two ciphertexts while it switches): the exact three-word accumulator and the three-product fold, over the Shoup product
// of rns_arith.hpp, and ip_digit_loop -- the body of inner_product, parameterised by how the accumulators are seeded.
// One copy, so all kernels compute the same words.
#pragma once

#include <hip/hip_runtime.h>

#include "gpuntt/rns/inner_product.cuh"
#include "rns_arith.hpp"

namespace gpuntt
{
    namespace kern
    {
        constexpr int IP_NT = 256; // lanes per workgroup at most (a ring narrower than that gets a narrower workgroup)

        // inputs per pass over the key, at most: RB * C * V accumulators of 5 (u64) or 3 (u32) registers are live, and
        // 8 (r, c) pairs are what the register file holds at 3 waves per SIMD for u64
        constexpr int ip_block(int C) { return C <= 2 ? 4 : 2; }

        // the key limb of every modulus, as a kernel argument: read at blockIdx.y, a scalar load
        struct IpLimbs
        {
            unsigned char v[INNERPROD_MAX_MODULI];
        };

        // RnsWide, rns_mulhi, rns_shoup, ip_min: rns_arith.hpp

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

        // a lane's 16-byte group (V = 1: one word)
        template <typename T, int V> struct alignas(V * sizeof(T)) IpVec
        {
            T x[V];
        };

        // where a lane of ip_digit_loop stands: modulus m, first column col, inputs r0 .. r0 + nr - 1 of its block; `at`
        // is the lane's word inside a T[count][M][N] stack array, `stack` one input's M limbs, `comp` one component
        // (count stacks), all in words
        struct IpPlace
        {
            unsigned m;
            int r0, nr;
            unsigned long long col, at, stack, comp;
        };

        // How inner_product seeds its accumulators: zero, or -- `accumulate` -- the words of `out`
        template <typename T> struct IpSeedOut
        {
            int accumulate;
            template <int RB, int C, int V>
            __device__ __forceinline__ void operator()(IpAcc<T> (&acc)[RB][C][V], const IpPlace& p, const T* out) const
            {
#pragma unroll
                for (int r = 0; r < RB; r++)
#pragma unroll
                    for (int c = 0; c < C; c++)
                    {
                        IpVec<T, V> o{};
                        if (accumulate != 0 && r < p.nr)
                            o = *reinterpret_cast<const IpVec<T, V>*>(out + p.at + c * p.comp + r * p.stack);
#pragma unroll
                        for (int v = 0; v < V; v++)
                            acc[r][c][v] = IpAcc<T>{o.x[v], T(0), 0u};
                    }
            }
        };

        // The body of inner_product (inner_product.hip has the mapping): a lane owns V columns of modulus m = blockIdx.y
        // of a block of RB inputs, seeds its RB * C * V accumulators through `seed(acc, place, out)`, walks the D digits once and stores
        // the canonical words.  a: T[D][count][M][N], key: T[D][C][KM][N], out: T[C][count][M][N]
        template <typename T, int V, int C, int RB, typename Seed>
        __device__ __forceinline__ void ip_digit_loop(const T* __restrict__ a, const T* __restrict__ key,
                                                      T* __restrict__ out, const T* __restrict__ consts,
                                                      const IpLimbs& limbs, int D, int count, int M, int KM, int n_power,
                                                      unsigned tiles, const Seed& seed)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, rblock = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const int r0 = static_cast<int>(rblock) * RB;
            const int nr = ip_min(RB, count - r0); // inputs of this block: wave-uniform

            // all index arithmetic in 64 bits: D_key * C * key_mod_count * N passes 2^32 words at real sizes
            const unsigned long long poly = 1ull << n_power;
            const unsigned long long stack = static_cast<unsigned long long>(M) << n_power;         // one input's limbs
            const unsigned long long a_digit = static_cast<unsigned long long>(count) * stack;       // a: [D][count][M][N]
            const unsigned long long key_comp = static_cast<unsigned long long>(KM) << n_power;      // key: [D][C][KM][N]
            const unsigned long long key_digit = static_cast<unsigned long long>(C) * key_comp;
            const unsigned long long at = static_cast<unsigned long long>(r0) * stack + m * poly + col;
            const T* pa = a + at;
            const T* pk = key + static_cast<unsigned long long>(limbs.v[m]) * poly + col;
            T* po = out + at; // out: [C][count][M][N], component stride = a_digit

            IpAcc<T> acc[RB][C][V];
            seed(acc, IpPlace{m, r0, nr, col, at, stack, a_digit}, out);

            // the loads of one digit carry no condition, so all RB + C of them are in flight before the first product:
            // an input past the end of the last block re-reads the block's last one (its results are never stored)
            unsigned long long a_in[RB];
#pragma unroll
            for (int r = 0; r < RB; r++)
                a_in[r] = static_cast<unsigned long long>(ip_min(r, nr - 1)) * stack;
            for (int d = 0; d < D; d++)
            {
                Vec kv[C], av[RB];
#pragma unroll
                for (int c = 0; c < C; c++)
                    kv[c] = *reinterpret_cast<const Vec*>(pk + c * key_comp);
#pragma unroll
                for (int r = 0; r < RB; r++)
                    av[r] = *reinterpret_cast<const Vec*>(pa + a_in[r]);
#pragma unroll
                for (int r = 0; r < RB; r++)
#pragma unroll
                    for (int c = 0; c < C; c++)
#pragma unroll
                        for (int v = 0; v < V; v++)
                            acc[r][c][v].mac(av[r].x[v], kv[c].x[v]);
                pa += a_digit;
                pk += key_digit;
            }

            const IpFold<T> fold(consts, M, m);
#pragma unroll
            for (int r = 0; r < RB; r++)
                if (r < nr)
                {
#pragma unroll
                    for (int c = 0; c < C; c++)
                    {
                        Vec o;
#pragma unroll
                        for (int v = 0; v < V; v++)
                        {
                            o.x[v] = fold.reduce(fold.sum(acc[r][c][v])); // the sum is below 3 q < 2^W
                        }
                        *reinterpret_cast<Vec*>(po + c * a_digit + r * stack) = o;
                    }
                }
        }
    } // namespace kern
} // namespace gpuntt
