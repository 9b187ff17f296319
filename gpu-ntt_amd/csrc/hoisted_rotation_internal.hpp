// hoisted_rotation_internal.hpp -- what key_switch.hip needs of hoisted_rotation.hip: the kernel arguments of one
// rotate_hoisted, rotate_hoisted_sum or linear_transform_bsgs call, the chunk rule and the launchers of
// inner_product_galois, inner_product_galois_sum and the three kernels of the baby-step/giant-step transform.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gpuntt/ntt_merge/galois.cuh"
#include "gpuntt/rns/inner_product.cuh"
#include "gpuntt/rns/key_switch.cuh"

namespace gpuntt
{
    namespace kern
    {
        // Everything of a call that is not a buffer travels as ONE kernel argument (as GaloisArgs and IpLimbs do): no
        // device copy, nothing a captured graph has to keep alive.  2.1 KiB for u64, inside the 4 KiB argument segment.
        template <typename T> struct HoistArgs
        {
            const T* key[GALOIS_MAX_COUNT];          // key_g: T[D_key][2][key_mod_count][N]
            T p_mod_q[INNERPROD_MAX_MODULI];         // P mod q_m, m < L ...
            T p_mod_q_shoup[INNERPROD_MAX_MODULI];   // ... and floor((P mod q_m) 2^W / q_m)
            std::uint32_t elt[GALOIS_MAX_COUNT];     // k_g, reduced
            std::uint32_t inv[GALOIS_MAX_COUNT];     // k_g^-1, same modulus
            unsigned char limb[INNERPROD_MAX_MODULI]; // the key limb of every modulus of the full base
            int count;                               // G
        };

        // HoistArgs plus the G weight pointers, still ONE kernel argument: 2632 bytes for u64, 2120 for u32, inside the
        // 4 KiB argument segment with the kernel's other 72 bytes
        template <typename T> struct HoistSumArgs
        {
            HoistArgs<T> h;
            const T* weight[GALOIS_MAX_COUNT]; // pt_g: T[M][N] over the full base, or nullptr (weight 1)
        };
        static_assert(sizeof(HoistSumArgs<Data64>) == 2632 && sizeof(HoistSumArgs<Data32>) == 2120,
                      "HoistSumArgs has to stay inside the 4 KiB argument segment");

        // The n2 * n1 weight pointers of one linear_transform_bsgs call, in the order of the scratch (keyed steps first on
        // both axes), ONE kernel argument: 2056 bytes, inside the 4 KiB argument segment with the kernel's other 40
        template <typename T> struct BsgsWeights
        {
            const T* w[KEYSWITCH_MAX_DIAGONALS]; // pt_{g,b} at [g * n1 + b]: T[M][N] over the full base, or nullptr (absent)
            int n1, n2;
        };
        static_assert(sizeof(BsgsWeights<Data64>) == 2056 && sizeof(BsgsWeights<Data32>) == 2056,
                      "BsgsWeights has to stay inside the 4 KiB argument segment");
    } // namespace kern

    namespace host
    {
        constexpr int HOIST_LOG_MAX = 13;    // inner_product_galois: lanes walk the chunk, any chunk the hook can name
        constexpr int HOIST_SUM_LOG_MAX = 8; // inner_product_galois_sum: one slot per lane, at most 256 lanes

        // log2 of the chunk for words of `word_bytes`, D digits and a ring of 2^n_power: the largest power of two with
        // (D + 1) chunk word_bytes inside the LDS budget, at least 64 slots, at most 2^max_log and at most N.  The test
        // hook keyswitch_hoist_chunk replaces the budget rule (not the caps at N, at 2^max_log and at 64 KiB of LDS)
        int hoist_chunk_log(size_t word_bytes, int D, int n_power, int max_log);
        void keyswitch_set_hoist_chunk(int v); // test hook: 0 = the rule above, 6 .. 13 = log2 of the chunk

        // a: T[D][count][M][N], c0: T[count][L][N] or nullptr; consts: the workspace image of InnerProductPlan for the M
        // moduli.  acc: T[G][2][count][M][N] (hoist_launch) or T[2][count][M][N] (hoist_sum_launch).  One launch; throws
        // std::invalid_argument beyond the grid limits
        template <typename T>
        void hoist_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistArgs<T>& args, int D,
                          int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream);
        template <typename T>
        void hoist_sum_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistSumArgs<T>& args, int D,
                              int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream);

        // The kernels of linear_transform_bsgs.  S = count * M * N words, one component of `count` stacks.
        // bsgs_scale_launch: u[b][c][r][m][j] = [m < L] (P mod q_m) * c_c[r][m][j] mod q_m for first <= b < n1 (c_0 = c0,
        //   zero when null; c_1 = c1); u: T[n1][2][count][M][N].  One launch
        // bsgs_sum_launch: v[c][g][r][m][j] = (sum_{b: w[g n1 + b] != null} w[g n1 + b][m][j] * u[b][c][r][m][j]) mod q_m;
        //   v: T[2][n2][count][M][N].  One launch; u and v 16-byte aligned (they live in the scratch)
        // bsgs_giant_launch: acc[c][r][m][j] = (sum_{g < n2k} (sum_d a[d][g count + r][m][pi_g(j)] * key_g[d][c][limb(m)][j]
        //   + [c = 0] v[0][g][r][m][pi_g(j)]) + sum_{n2k <= g < n2} v[c][g][r][m][j]) mod q_m with n2k = args.count;
        //   a: T[D][n2k * count][M][N], acc: T[2][count][M][N].  One launch; a and v 16-byte aligned
        // All three throw std::invalid_argument beyond the grid limits, before the launch
        // bsgs_sum_shape: the words per lane (a 16-byte group, or 1) and the lanes per workgroup of bsgs_weighted_sum
        void bsgs_sum_shape(size_t word_bytes, int n1, int n_power, bool aligned, int& V, unsigned& nt);
        template <typename T>
        void bsgs_scale_launch(const T* c0, const T* c1, T* u, const T* consts, const kern::HoistArgs<T>& args, int first,
                               int n1, int count, int L, int M, int n_power, hipStream_t stream);
        template <typename T>
        void bsgs_sum_launch(const T* u, T* v, const T* consts, const kern::BsgsWeights<T>& weights, int count, int M,
                             int n_power, hipStream_t stream);
        template <typename T>
        void bsgs_giant_launch(const T* a, const T* v, T* acc, const T* consts, const kern::HoistArgs<T>& args, int n2,
                               int D, int count, int M, int KM, int n_power, bool negacyclic, hipStream_t stream);
    } // namespace host
} // namespace gpuntt
