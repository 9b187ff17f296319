// base_conversion_internal.hpp -- what key_switch.hip and bfv_multiply.hip share with base_conversion.hip: the conversion
// unit every conversion kernel of the library is made of (bc_z, bc_block_mac, bc_fold, with the proofs of their bounds),
// the kernel base_convert itself and mod_down_add, its strided division with an addend epilogue, the constants of one pair of bases in exact integers, their image in a workspace, the
// exact-integer column reference and the output-split policy.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "gpuntt/rns/base_conversion.cuh"
#include "rns_arith.hpp"
#include "rns_host.hpp"

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

        // RnsWide, rns_mulhi, rns_shoup, ip_min: rns_arith.hpp

        // Pointers into a workspace are in the CONSTANT address space: nothing writes the workspace while a conversion
        // runs, and a load from that address space at a wave-uniform address is a scalar load whatever the stores around
        // it are (as plain global pointers the compiler could not rule out the stores to `out` -- which may alias c, so
        // neither is __restrict__ -- and fetched the matrix rows with vector loads)
        template <typename T> using BcCP = const T __attribute__((address_space(4)))*;

        // the five arrays bc_fold reads, indexed by the output modulus: what BcConsts and key_switch.hip's KsConsts share
        template <typename T> struct BcFoldConsts
        {
            BcCP<T> t1, t1p, t2, t2p, onep;
        };

        // BcOffsets as pointers into the workspace `base`
        template <typename T> struct BcConsts : BcFoldConsts<T>
        {
            using CP = BcCP<T>;
            CP q, w, wp, recip, shift, matrix, p, negq, qinv, qinvp;
            __device__ BcConsts(const T* workspace, const BcOffsets& o)
            {
                const CP base = (CP) (workspace);
                q = base + o.q, w = base + o.w, wp = base + o.wp, recip = base + o.recip, shift = base + o.shift;
                matrix = base + o.matrix, p = base + o.p, negq = base + o.negq, qinv = base + o.qinv;
                qinvp = base + o.qinvp, this->t1 = base + o.t1, this->t1p = base + o.t1p, this->t2 = base + o.t2;
                this->t2p = base + o.t2p, this->onep = base + o.onep;
            }
        };

        constexpr int BC_CHUNK = 16; // terms below 2^(2W-4) (moduli below 2^(W-2)) that a 2W-bit sum holds

        // ---- the conversion unit: what base_convert, key_switch.hip's ks_mod_up and bfv_multiply.hip's two kernels are
        // made of.  A lane owns one coefficient column; its y_i = x_i * qhat_i^-1 mod q_i lie in LDS at ys[i * ystride]

        // z = (y R) >> (b - 1) < 2^W, the term of base_conversion.cuh's v; a power of two q = 2^(b - 1) has R = 2^W,
        // stored as 0.  The z_i are summed from 2^(W-1) in a 2W-bit word whose high word is v
        template <typename T> __device__ __forceinline__ T bc_z(T y, T recip, T shift)
        {
            using W2 = typename RnsWide<T>::type;
            constexpr int W = static_cast<int>(8 * sizeof(T));
            const int sh = static_cast<int>(shift);
            return (recip != 0) ? static_cast<T>((static_cast<W2>(y) * recip) >> sh) : (y << (W - sh));
        }

        // BC_KB outputs of one conversion: acc[b] + carry[b] 2^2W = v * negq[b] + sum_{i < n} ys[i * ystride] * row[i *
        // rstride + b]; without CENTRED the sum alone, and v and negq are not read.  row and negq point at the block's
        // first column; both are padded with zeros to a multiple of BC_KB.  Blocking the OUTPUTS keeps the live state at
        // BC_KB accumulators whatever n and the number of outputs are.  A term is below 2^(2W-4), so BC_CHUNK = 16 of
        // them go into a plain 2W-bit sum with no carry to watch; the sums go into the three-word accumulator {carry,
        // acc}, one carry test per chunk and output: n = 64 terms of 2^124 do not fit 128 bits, 64 carries fit any word.
        // n >= 1 at every caller (every base has a modulus, every digit a limb); n = 0 would leave the seed alone
        template <typename T, bool CENTRED>
        __device__ __forceinline__ void bc_block_mac(const T* ys, int ystride, BcCP<T> row, int rstride, int n, T v,
                                                     BcCP<T> negq, typename RnsWide<T>::type (&acc)[BC_KB],
                                                     T (&carry)[BC_KB])
        {
            using W2 = typename RnsWide<T>::type;
#pragma unroll
            for (int b = 0; b < BC_KB; b++)
            {
                if constexpr (CENTRED)
                    acc[b] = static_cast<W2>(v) * negq[b];
                else
                    acc[b] = 0;
                carry[b] = 0;
            }
            for (int i0 = 0; i0 < n; i0 += BC_CHUNK)
            {
                const int i1 = ip_min(i0 + BC_CHUNK, n);
                W2 part[BC_KB];
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                    part[b] = 0;
#pragma unroll 2
                for (int i = i0; i < i1; i++)
                {
                    const T y = ys[i * ystride];
#pragma unroll
                    for (int b = 0; b < BC_KB; b++)
                        part[b] += static_cast<W2>(y) * row[b];
                    row += rstride;
                }
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    acc[b] += part[b];
                    carry[b] += (acc[b] < part[b]) ? 1u : 0u;
                }
            }
        }

        // The accumulator S = carry 2^2W + h 2^W + l modulo p, the output modulus at index j of k's arrays:
        // h [2^W]_p + carry [2^2W]_p + l as three exact Shoup products against the plan's constants, each canonical, so
        // their sum is below 3 p < 2^W, and two conditional subtractions.  Modulus<T>::mu is not used: its Barrett step is
        // exact only for operands below 2^(2 bit + 1), and a 20-bit p_j under 62-bit q_i sums to 2^88.  Each constant is
        // loaded where its product needs it.  (IpFold of inner_product_internal.hpp is the same fold over words held in
        // registers; one function over the eight words for both put all five loads before the first product here and
        // the four kernels were scheduled differently: DESIGN.md 3.10)
        template <typename T>
        __device__ __forceinline__ T bc_fold(typename RnsWide<T>::type acc, T carry, const BcFoldConsts<T>& k, int j, T p)
        {
            constexpr int W = static_cast<int>(8 * sizeof(T));
            T r = rns_shoup<T>(static_cast<T>(acc >> W), k.t1[j], k.t1p[j], p);
            r += rns_shoup<T>(carry, k.t2[j], k.t2p[j], p);
            r += rns_shoup<T>(static_cast<T>(acc), T(1), k.onep[j], p);
            r = r >= p ? r - p : r;
            return r >= p ? r - p : r;
        }

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

        // ADD: an addend epilogue -- out = (the conversion's word + (addend mod p_j)) mod p_j, canonical, with addend laid
        // out as `out` is, so a lane reads its addend word at the index it then writes: addend may be exactly out.  Any
        // word is accepted: one Shoup product against the companion of 1 makes it canonical, and two canonical words of a
        // modulus below 2^(W-1) add without a carry.  A compile-time switch like STRIDED, and for the same reason: the
        // argument is empty where there is no addend, and the kernels without one keep their registers
        template <typename T, bool ADD> struct BcAddend
        {
            const T* words;
        };
        template <typename T> struct BcAddend<T, false>
        {
        };

        // The body of every launch of this unit: base_convert below, and mod_down_add, which is the strided centred
        // division with the addend epilogue under a name of its own, so that the launch log tells the two apart
        template <typename T, bool CENTRED, bool DIVIDE, bool STRIDED, bool ADD>
        __device__ __forceinline__ void bc_convert_body(const T* __restrict__ in, const T* c_in, T* out,
                                                        const T* __restrict__ consts, const BcOffsets& off, int L, int K,
                                                        int KP, int n_power, unsigned long long total,
                                                        const BcStrides<STRIDED>& strides, const BcAddend<T, ADD>& addend)
        {
            // the plan refuses an empty input base.  Said here because with bc_block_mac inlined the compiler otherwise
            // keeps an empty-sum path through every output block and zeroes the accumulators on both: 12 VALU
            // instructions per block, 3 % of the u64 4 -> 28 ModUp
            __builtin_assume(L > 0);
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
                    zsum += bc_z<T>(y, k.recip[i], k.shift[i]);
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
                W2 acc[BC_KB];
                T carry[BC_KB];
                bc_block_mac<T, CENTRED>(ys, BC_NT, k.matrix + j0, KP, L, v, k.negq + j0, acc, carry);
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    const int j = j0 + b;
                    if (j < K)
                    {
                        const T p = k.p[j];
                        T r = bc_fold<T>(acc[b], carry[b], k, j, p);
                        const unsigned long long o = obase + (static_cast<unsigned long long>(j) << n_power);
                        if constexpr (DIVIDE)
                        {
                            const T cj = c_in[cbase + (static_cast<unsigned long long>(j) << n_power)];
                            // c - conv as a word that is congruent to it: any word c is read modulo p
                            const T d = cj >= r ? cj - r : cj + (p - r);
                            r = rns_shoup<T>(d, k.qinv[j], k.qinvp[j], p);
                        }
                        if constexpr (ADD)
                        {
                            r += rns_shoup<T>(addend.words[o], T(1), k.onep[j], p);
                            r = r >= p ? r - p : r;
                        }
                        out[o] = r;
                    }
                }
            }
        }

        template <typename T, bool CENTRED, bool DIVIDE, bool STRIDED = false>
        __global__ __launch_bounds__(BC_NT) void base_convert(const T* __restrict__ in, const T* c_in, T* out,
                                                              const T* __restrict__ consts, BcOffsets off,
                                                              int L, int K, int KP, int n_power,
                                                              unsigned long long total, BcStrides<STRIDED> strides)
        {
            bc_convert_body<T, CENTRED, DIVIDE, STRIDED, false>(in, c_in, out, consts, off, L, K, KP, n_power, total,
                                                                strides, BcAddend<T, false>{});
        }

        // KeySwitchPlan::mod_down_add: base_convert<T, centred, divide, STRIDED> with the addend epilogue.  addend:
        // T[stacks][K][N], dense like out; it may be exactly out and must not overlap anything else (the host refuses)
        template <typename T>
        __global__ __launch_bounds__(BC_NT) void mod_down_add(const T* __restrict__ in, const T* c_in, const T* addend,
                                                              T* out, const T* __restrict__ consts, BcOffsets off, int L,
                                                              int K, int KP, int n_power, unsigned long long total,
                                                              BcStrides<true> strides)
        {
            bc_convert_body<T, true, true, true, true>(in, c_in, out, consts, off, L, K, KP, n_power, total, strides,
                                                       BcAddend<T, true>{addend});
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

        // base_conversion.cuh's formulas for one column in exact integers, every step reduced with %: x[i] (any words)
        // of the input base of `c` -> conv[j]
        template <typename T>
        void bc_ref_convert(const BcHostConsts& c, const std::uint64_t* x, bool centred, std::uint64_t* conv);

        // a count of outputs rounded up to whole blocks of BC_KB
        inline int bc_padded(int count) { return (count + kern::BC_KB - 1) / kern::BC_KB * kern::BC_KB; }
        // workgroups per column tile that share the tile's K outputs: rns_split over the blocks of BC_KB, with the test
        // hook baseconv_ksplit
        int bc_ksplit(unsigned long long tiles, int K);
    } // namespace host
} // namespace gpuntt
