// base_conversion_internal.hpp -- what key_switch.hip shares with base_conversion.hip: the constants of one pair of
// bases in exact integers, their image in a workspace, the output-split policy and the kernel itself.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "gpuntt/rns/base_conversion.cuh"
#include "rns_arith.hpp"

namespace gpuntt
{
    namespace kern
    {
        constexpr int BC_NT = 128; // lanes per workgroup: L = 64 u64 words per lane are 64 KiB of LDS
        constexpr int BC_KB = 4;   // outputs per pass over the y_i

        // where the plan's constants lie in the workspace, in words: L = in_count, KP = out_count rounded up to BC_KB
        // (the padding columns of the matrix are zero and are never stored)
        struct BcOffsets
        {
            unsigned q;      // [L]
            unsigned w;      // [L] qhat_i^-1 mod q_i
            unsigned wp;     // [L] its Shoup companion
            unsigned recip;  // [L] R_i (0: q_i is a power of two)
            unsigned shift;  // [L] b_i - 1
            unsigned matrix; // [L][KP] qhat_i mod p_j
            unsigned p;      // [KP]
            unsigned negq;   // [KP] (-Q) mod p_j
            unsigned qinv;   // [KP] Q^-1 mod p_j
            unsigned qinvp;  // [KP] its Shoup companion
            unsigned t1;     // [KP] 2^W mod p_j
            unsigned t1p;
            unsigned t2;     // [KP] 2^2W mod p_j
            unsigned t2p;
            unsigned onep;   // [KP] floor(2^W / p_j): the Shoup companion of 1
        };

        // RnsWide, rns_mulhi, rns_shoup: rns_arith.hpp

        // the same as pointers into the workspace `base`, in the CONSTANT address space: nothing writes the workspace
        // while a conversion runs, and a load from that address space at a wave-uniform address is a scalar load
        // whatever the stores around it are (as plain global pointers the compiler could not rule out the stores to
        // `out` -- which may alias c, so neither is __restrict__ -- and fetched the matrix rows with vector loads)
        template <typename T> struct BcConsts
        {
            using CP = const T __attribute__((address_space(4)))*;
            CP q, w, wp, recip, shift, matrix, p, negq, qinv, qinvp, t1, t1p, t2, t2p, onep;
            __device__ BcConsts(const T* workspace, const BcOffsets& o)
            {
                const CP base = (CP) (workspace);
                q = base + o.q, w = base + o.w, wp = base + o.wp, recip = base + o.recip, shift = base + o.shift;
                matrix = base + o.matrix, p = base + o.p, negq = base + o.negq, qinv = base + o.qinv;
                qinvp = base + o.qinvp, t1 = base + o.t1, t1p = base + o.t1p, t2 = base + o.t2, t2p = base + o.t2p;
                onep = base + o.onep;
            }
        };

        constexpr int BC_CHUNK = 16; // terms below 2^(2W-4) (moduli below 2^(W-2)) that a 2W-bit sum holds

        // STRIDED: stack e of in, c and out starts e * stride words behind its pointer instead of at the dense
        // e L N, e K N and e K N -- a plan that converts limbs in place inside wider stacks (key_switch.hip).  A
        // compile-time switch, with the strides in an argument that is empty for the dense form: as run-time arguments
        // of one kernel they took the dense u64 `convert` from 73 / 69 to 90 / 86 VGPRs
        template <bool STRIDED> struct BcStrides
        {
            unsigned long long in, c, out;
        };
        template <> struct BcStrides<false>
        {
        };

        template <typename T, bool CENTRED, bool DIVIDE, bool STRIDED = false>
        __global__ __launch_bounds__(BC_NT) void base_convert(const T* __restrict__ in, const T* c_in, T* out,
                                                              const T* __restrict__ consts, BcOffsets off,
                                                              int L, int K, int KP, int n_power,
                                                              unsigned long long total, BcStrides<STRIDED> strides)
        {
            const BcConsts<T> k(consts, off);
            using W2 = typename RnsWide<T>::type;
            constexpr int W = static_cast<int>(8 * sizeof(T));
            extern __shared__ __align__(16) unsigned char bc_smem[];
            T* ys = reinterpret_cast<T*>(bc_smem) + threadIdx.x;

            const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * BC_NT + threadIdx.x;
            if (t >= total)
                return; // (no barrier below)
            const unsigned long long e = t >> n_power, col = t & ((1ull << n_power) - 1ull);
            const T* src;
            if constexpr (STRIDED)
                src = in + e * strides.in + col;
            else
                src = in + ((e * static_cast<unsigned>(L)) << n_power) + col;

            W2 zsum = static_cast<W2>(1) << (W - 1);
#pragma unroll 4
            for (int i = 0; i < L; i++)
            {
                const T q = k.q[i];
                const T y = rns_shoup<T>(src[static_cast<unsigned long long>(i) << n_power], k.w[i], k.wp[i], q);
                ys[i * BC_NT] = y;
                if constexpr (CENTRED)
                {
                    const T r = k.recip[i];
                    const int sh = static_cast<int>(k.shift[i]);
                    // z_i = (y R_i) >> (b_i - 1) < 2^W; a power of two q_i = 2^(b_i - 1) has R_i = 2^W
                    const T z = (r != 0) ? static_cast<T>((static_cast<W2>(y) * r) >> sh) : (y << (W - sh));
                    zsum += z;
                }
            }
            T v = 0;
            if constexpr (CENTRED)
                v = static_cast<T>(zsum >> W);

            unsigned long long obase, cbase;
            if constexpr (STRIDED)
                obase = e * strides.out + col, cbase = e * strides.c + col;
            else
                obase = cbase = ((e * static_cast<unsigned>(K)) << n_power) + col;
            for (int j0 = static_cast<int>(blockIdx.y) * BC_KB; j0 < K; j0 += static_cast<int>(gridDim.y) * BC_KB)
            {
                // BC_CHUNK terms at a time go into a plain 2W-bit sum (no carry to watch); the sums go into the
                // three-word accumulator {carry, acc}, one carry test per chunk and output
                W2 acc[BC_KB];
                T carry[BC_KB];
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    acc[b] = CENTRED ? static_cast<W2>(v) * k.negq[j0 + b] : static_cast<W2>(0);
                    carry[b] = 0;
                }
                typename BcConsts<T>::CP row = k.matrix + j0;
                for (int i0 = 0; i0 < L; i0 += BC_CHUNK)
                {
                    const int i1 = min(i0 + BC_CHUNK, L);
                    W2 part[BC_KB];
#pragma unroll
                    for (int b = 0; b < BC_KB; b++)
                        part[b] = 0;
#pragma unroll 2
                    for (int i = i0; i < i1; i++)
                    {
                        const T y = ys[i * BC_NT];
#pragma unroll
                        for (int b = 0; b < BC_KB; b++)
                            part[b] += static_cast<W2>(y) * row[b];
                        row += KP;
                    }
#pragma unroll
                    for (int b = 0; b < BC_KB; b++)
                    {
                        acc[b] += part[b];
                        carry[b] += (acc[b] < part[b]) ? 1u : 0u;
                    }
                }
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    const int j = j0 + b;
                    if (j < K)
                    {
                        const T p = k.p[j];
                        T r = rns_shoup<T>(static_cast<T>(acc[b] >> W), k.t1[j], k.t1p[j], p);
                        r += rns_shoup<T>(carry[b], k.t2[j], k.t2p[j], p);
                        r += rns_shoup<T>(static_cast<T>(acc[b]), T(1), k.onep[j], p); // r < 3 p < 2^W
                        r = r >= p ? r - p : r;
                        r = r >= p ? r - p : r;
                        const unsigned long long o = obase + (static_cast<unsigned long long>(j) << n_power);
                        if constexpr (DIVIDE)
                        {
                            const T cj = c_in[cbase + (static_cast<unsigned long long>(j) << n_power)];
                            // c - conv as a word that is congruent to it: any word c is read modulo p
                            const T d = cj >= r ? cj - r : cj + (p - r);
                            r = rns_shoup<T>(d, k.qinv[j], k.qinvp[j], p);
                        }
                        out[o] = r;
                    }
                }
            }
        }
    } // namespace kern

    namespace host
    {
        // the constants in exact integers (64-bit words for both widths)
        struct BcHostConsts
        {
            int L, K;
            std::vector<std::uint64_t> q, p, w, wp, recip, blen, matrix, qmod, negq, qinv, qinvp, t1, t1p, t2, t2p, onep;
        };

        // the value of a modulus after the checks every RNS plan applies ("Invalid modulus!")
        template <typename T> std::uint64_t bc_checked_value(const Modulus<T>& m);
        // the checks of BaseConvPlan's constructor, then the constants
        template <typename T> BcHostConsts bc_derive(const Modulus<T>* qm, int L, const Modulus<T>* pm, int K);
        // words of the image below
        size_t bc_image_words(int L, int K);
        // the workspace image of these constants (bc_image_words(L, K) words) and where its parts lie
        template <typename T> std::vector<T> bc_image(const BcHostConsts& h, kern::BcOffsets& off);

        // workgroups per column tile that share the tile's outputs (base_conv_ksplit, with its test hook)
        int bc_ksplit(unsigned long long tiles, int K);
    } // namespace host
} // namespace gpuntt
