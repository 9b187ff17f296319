// relinearize.hip -- the kernels of KeySwitchPlan<T>::multiply_relinearize and ::relinearize
// (include/gpuntt/rns/key_switch.cuh).  multiply_relinearize: the
// product of two ciphertexts x = (x0, x1), y = (y0, y1) with the top component x1 y1 switched back under the
// relinearization key, in ONE key switch.
//
//   tensor_top:            d2[r][m][j] = x1[r][m][j] * y1[r][m][j] mod q_m,  m < L                -- what is decomposed
//   inner_product_tensor:  acc[c][r][m][j] = ( sum_{d<D} a[d][r][m][j] * key[d][c][limb(m)][j]
//                                              + [m < L] (P mod q_m) * d_c[r][m][j] ) mod q_m,  c < 2
//                          d_0 = x0 y0,  d_1 = x0 y1 + x1 y0
//
// inner_product_tensor is inner_product with another seed: the mapping, the digit loop, the ragged last block and the
// fold are ip_digit_loop of inner_product_internal.hpp, the ONE copy of that body.  Where inner_product starts its
// accumulators at zero or at `out`, this kernel starts them at the tensor terms, formed on the fly from the four input
// words of the lane's columns: d_0 and d_1 are never written to memory.  blockIdx.y is m, so m < L is workgroup-uniform:
// the workgroups of the K special limbs load nothing of x or y and start at zero.
//
// The seed (IpSeedTensor).  x0' = rns_shoup(x0, P mod q_m) and x1' = rns_shoup(x1, P mod q_m) are canonical for ANY word
// x0, x1; then three exact macs: x0' y0 into c = 0, x0' y1 and x1' y0 into c = 1.  mac is exact for any two words, so y is
// not reduced.  Bound: the accumulator is exact up to its 32-bit carry count, one carry at most per term, and the fold's
// product with the carry word is an exact Shoup product for any word -- D + 2 terms (D <= 64) need no new bound.
//
// inner_product_seeded (KeySwitchPlan::relinearize with input_ntt): the same inner product for a three-component ciphertext
// whose low components c01 = T[2][count][L][N] already exist.  Its seed (IpSeedLow) is ONE exact mac per word, (P mod q_m)
// times the word as it stands: the accumulator is exact for any two words, so c01 is not reduced first.  D + 1 terms.
//
// tensor_top is the same arithmetic for one term: one mac into a zero accumulator, IpFold::sum, IpFold::reduce.
//
// Both kernels: a lane owns a 16-byte group (V = 16 / sizeof(T) columns), V = 1 for a base pointer that is not 16-byte
// aligned or N below a group; constants through the constant address space; 64-bit indices.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "inner_product_internal.hpp"
#include "launch.hpp"
#include "relinearize_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // How inner_product_tensor seeds its accumulators: (P mod q_m) d_0 and (P mod q_m) d_1 for m < L, zero for the
        // special limbs.  x, y: T[2][count][L][N]; an input past the end of the last block re-reads the block's last one,
        // as the digit loop does
        template <typename T> struct IpSeedTensor
        {
            const T* x;
            const T* y;
            T q, pq, pqs; // q_m, P mod q_m and its Shoup companion
            int L, count, n_power;
            bool on; // m < L
            template <int RB, int C, int V>
            __device__ __forceinline__ void operator()(IpAcc<T> (&acc)[RB][C][V], const IpPlace& p, const T*) const
            {
                static_assert(C == 2, "a product of two ciphertexts has two components after the switch");
                using Vec = IpVec<T, V>;
#pragma unroll
                for (int r = 0; r < RB; r++)
#pragma unroll
                    for (int c = 0; c < C; c++)
#pragma unroll
                        for (int v = 0; v < V; v++)
                            acc[r][c][v] = IpAcc<T>{T(0), T(0), 0u};
                if (!on)
                    return;
                const unsigned long long in_stack = static_cast<unsigned long long>(L) << n_power; // one input's limbs
                const unsigned long long in_comp = static_cast<unsigned long long>(count) * in_stack;
                const unsigned long long first =
                    static_cast<unsigned long long>(p.r0) * in_stack + (static_cast<unsigned long long>(p.m) << n_power) +
                    p.col;
#pragma unroll
                for (int r = 0; r < RB; r++)
                {
                    const unsigned long long at = first + static_cast<unsigned long long>(ip_min(r, p.nr - 1)) * in_stack;
                    const Vec x0 = *reinterpret_cast<const Vec*>(x + at);
                    const Vec x1 = *reinterpret_cast<const Vec*>(x + in_comp + at);
                    const Vec y0 = *reinterpret_cast<const Vec*>(y + at);
                    const Vec y1 = *reinterpret_cast<const Vec*>(y + in_comp + at);
#pragma unroll
                    for (int v = 0; v < V; v++)
                    {
                        const T s0 = rns_shoup<T>(x0.x[v], pq, pqs, q), s1 = rns_shoup<T>(x1.x[v], pq, pqs, q);
                        acc[r][0][v].mac(s0, y0.x[v]);
                        acc[r][1][v].mac(s0, y1.x[v]);
                        acc[r][1][v].mac(s1, y0.x[v]);
                    }
                }
            }
        };

        // grid: x = rblock * tiles + tile, y = m < M; the mapping of inner_product
        template <typename T, int V, int RB>
        __global__ __launch_bounds__(IP_NT) void inner_product_tensor(const T* __restrict__ a, const T* __restrict__ key,
                                                                      T* __restrict__ acc, const T* __restrict__ consts,
                                                                      const T* x, const T* y, RelinArgs<T> ra, int D,
                                                                      int count, int L, int M, int KM, int n_power,
                                                                      unsigned tiles)
        {
            using CP = const T __attribute__((address_space(4)))*;
            const unsigned m = blockIdx.y;
            const bool on = m < static_cast<unsigned>(L);
            const IpSeedTensor<T> seed{x, y, ((CP) (consts))[m], ra.p_mod_q[m], ra.p_mod_q_shoup[m], L, count, n_power, on};
            ip_digit_loop<T, V, 2, RB>(a, key, acc, consts, ra.limbs, D, count, M, KM, n_power, tiles, seed);
        }

        // How inner_product_seeded seeds its accumulators: (P mod q_m) c01[c] for m < L, zero for the special limbs.
        // c01: T[2][count][L][N] in NTT form, any word: mac is exact for any two words, so nothing is reduced first -- ONE
        // mac per seed word.  An input past the end of the last block re-reads the block's last one, as the digit loop does
        template <typename T> struct IpSeedLow
        {
            const T* c01;
            T pq; // P mod q_m
            int L, count, n_power;
            bool on; // m < L
            template <int RB, int C, int V>
            __device__ __forceinline__ void operator()(IpAcc<T> (&acc)[RB][C][V], const IpPlace& p, const T*) const
            {
                static_assert(C == 2, "a three-component ciphertext has two components after the switch");
                using Vec = IpVec<T, V>;
#pragma unroll
                for (int r = 0; r < RB; r++)
#pragma unroll
                    for (int c = 0; c < C; c++)
#pragma unroll
                        for (int v = 0; v < V; v++)
                            acc[r][c][v] = IpAcc<T>{T(0), T(0), 0u};
                if (!on)
                    return;
                const unsigned long long in_stack = static_cast<unsigned long long>(L) << n_power; // one input's limbs
                const unsigned long long in_comp = static_cast<unsigned long long>(count) * in_stack;
                const unsigned long long first =
                    static_cast<unsigned long long>(p.r0) * in_stack + (static_cast<unsigned long long>(p.m) << n_power) +
                    p.col;
#pragma unroll
                for (int r = 0; r < RB; r++)
                {
                    const unsigned long long at = first + static_cast<unsigned long long>(ip_min(r, p.nr - 1)) * in_stack;
#pragma unroll
                    for (int c = 0; c < C; c++)
                    {
                        const Vec s = *reinterpret_cast<const Vec*>(c01 + c * in_comp + at);
#pragma unroll
                        for (int v = 0; v < V; v++)
                            acc[r][c][v].mac(pq, s.x[v]);
                    }
                }
            }
        };

        // inner_product with the low components of a three-component ciphertext as the seed: KeySwitchPlan::relinearize
        // with input_ntt.  grid: x = rblock * tiles + tile, y = m < M; the mapping of inner_product
        template <typename T, int V, int RB>
        __global__ __launch_bounds__(IP_NT) void inner_product_seeded(const T* __restrict__ a, const T* __restrict__ key,
                                                                      T* __restrict__ acc, const T* __restrict__ consts,
                                                                      const T* c01, RelinArgs<T> ra, int D, int count,
                                                                      int L, int M, int KM, int n_power, unsigned tiles)
        {
            const unsigned m = blockIdx.y;
            const bool on = m < static_cast<unsigned>(L);
            const IpSeedLow<T> seed{c01, ra.p_mod_q[m], L, count, n_power, on};
            ip_digit_loop<T, V, 2, RB>(a, key, acc, consts, ra.limbs, D, count, M, KM, n_power, tiles, seed);
        }

        // grid: x = r * tiles + tile, y = m < L; x1, y1, d2: T[count][L][N]
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void tensor_top(const T* x1, const T* y1, T* __restrict__ d2,
                                                            const T* __restrict__ consts, int L, int M, int n_power,
                                                            unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, r = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long at =
                ((static_cast<unsigned long long>(r) * static_cast<unsigned>(L) + m) << n_power) + col;
            const Vec xv = *reinterpret_cast<const Vec*>(x1 + at);
            const Vec yv = *reinterpret_cast<const Vec*>(y1 + at);
            const IpFold<T> fold(consts, M, m);
            Vec o;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                IpAcc<T> s{T(0), T(0), 0u};
                s.mac(xv.x[v], yv.x[v]);
                o.x[v] = fold.reduce(fold.sum(s)); // the sum is below 3 q < 2^W
            }
            *reinterpret_cast<Vec*>(d2 + at) = o;
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            template <typename T, int V>
            void relin_top_as(const T* x1, const T* y1, T* d2, const T* consts, int count, int L, int M, int n_power,
                              bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::tensor_top<T, V>), dim3(g.blocks, static_cast<unsigned>(L)), dim3(g.nt), 0, stream, x1,
                              y1, d2, consts, L, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V, int RB>
            void relin_inner_as(const T* a, const T* key, T* acc, const T* consts, const T* x, const T* y,
                                const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, (static_cast<unsigned long long>(count) + RB - 1) / RB);
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::inner_product_tensor<T, V, RB>), dim3(g.blocks, static_cast<unsigned>(M)), dim3(g.nt),
                              0, stream, a, key, acc, consts, x, y, args, D, count, L, M, KM, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V, int RB>
            void relin_seeded_as(const T* a, const T* key, T* acc, const T* consts, const T* c01,
                                 const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                 bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, (static_cast<unsigned long long>(count) + RB - 1) / RB);
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::inner_product_seeded<T, V, RB>), dim3(g.blocks, static_cast<unsigned>(M)), dim3(g.nt),
                              0, stream, a, key, acc, consts, c01, args, D, count, L, M, KM, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            // the blocks of relin_inner_v below
            template <typename T, int V>
            void relin_seeded_v(const T* a, const T* key, T* acc, const T* consts, const T* c01,
                                const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                bool enqueue, hipStream_t stream)
            {
                if (count >= 4)
                    relin_seeded_as<T, V, 4>(a, key, acc, consts, c01, args, D, count, L, M, KM, n_power, enqueue, stream);
                else if (count >= 2)
                    relin_seeded_as<T, V, 2>(a, key, acc, consts, c01, args, D, count, L, M, KM, n_power, enqueue, stream);
                else
                    relin_seeded_as<T, V, 1>(a, key, acc, consts, c01, args, D, count, L, M, KM, n_power, enqueue, stream);
            }

            // a block of 4 inputs where count has them, of 2 for count = 2 or 3 (a block past the end of count multiplies
            // for nothing), one input per lane for count = 1: inner_product's launch_c for C = 2
            template <typename T, int V>
            void relin_inner_v(const T* a, const T* key, T* acc, const T* consts, const T* x, const T* y,
                               const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                               bool enqueue, hipStream_t stream)
            {
                static_assert(kern::ip_block(2) == 4, "the blocks below are those of inner_product for C = 2");
                if (count >= 4)
                    relin_inner_as<T, V, 4>(a, key, acc, consts, x, y, args, D, count, L, M, KM, n_power, enqueue, stream);
                else if (count >= 2)
                    relin_inner_as<T, V, 2>(a, key, acc, consts, x, y, args, D, count, L, M, KM, n_power, enqueue, stream);
                else
                    relin_inner_as<T, V, 1>(a, key, acc, consts, x, y, args, D, count, L, M, KM, n_power, enqueue, stream);
            }
        } // namespace

        template <typename T>
        void relin_top_launch(const T* x1, const T* y1, T* d2, const T* consts, int count, int L, int M, int n_power,
                              bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {x1, y1, d2}))
                relin_top_as<T, VW>(x1, y1, d2, consts, count, L, M, n_power, enqueue, stream);
            else
                relin_top_as<T, 1>(x1, y1, d2, consts, count, L, M, n_power, enqueue, stream);
        }

        template <typename T>
        void relin_inner_launch(const T* a, const T* key, T* acc, const T* consts, const T* x, const T* y,
                                const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {a, key, acc, x, y}))
                relin_inner_v<T, VW>(a, key, acc, consts, x, y, args, D, count, L, M, KM, n_power, enqueue, stream);
            else
                relin_inner_v<T, 1>(a, key, acc, consts, x, y, args, D, count, L, M, KM, n_power, enqueue, stream);
        }

        template <typename T>
        void relin_seeded_launch(const T* a, const T* key, T* acc, const T* consts, const T* c01,
                                 const kern::RelinArgs<T>& args, int D, int count, int L, int M, int KM, int n_power,
                                 bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {a, key, acc, c01}))
                relin_seeded_v<T, VW>(a, key, acc, consts, c01, args, D, count, L, M, KM, n_power, enqueue, stream);
            else
                relin_seeded_v<T, 1>(a, key, acc, consts, c01, args, D, count, L, M, KM, n_power, enqueue, stream);
        }

        template void relin_seeded_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*, const Data32*,
                                                  const kern::RelinArgs<Data32>&, int, int, int, int, int, int, bool,
                                                  hipStream_t);
        template void relin_seeded_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*, const Data64*,
                                                  const kern::RelinArgs<Data64>&, int, int, int, int, int, int, bool,
                                                  hipStream_t);
        template void relin_top_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*, int, int, int, int, bool,
                                               hipStream_t);
        template void relin_top_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*, int, int, int, int, bool,
                                               hipStream_t);
        template void relin_inner_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*, const Data32*,
                                                 const Data32*, const kern::RelinArgs<Data32>&, int, int, int, int, int, int,
                                                 bool, hipStream_t);
        template void relin_inner_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*, const Data64*,
                                                 const Data64*, const kern::RelinArgs<Data64>&, int, int, int, int, int, int,
                                                 bool, hipStream_t);
    } // namespace host
} // namespace gpuntt
