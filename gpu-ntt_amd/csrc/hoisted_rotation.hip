// hoisted_rotation.hip -- inner_product_galois: the inner product of hybrid key switching for G rotations of ONE
// decomposition (KeySwitchPlan<T>::rotate_hoisted, include/gpuntt/rns/key_switch.cuh).
//
//   acc[g][c][r][m][j] = ( sum_{d<D} a[d][r][m][pi_g(j)] * key_g[d][c][limb(m)][j]
//                          + [c = 0, m < L, c0 != null] (P mod q_m) * c0[r][m][pi_g(j)] ) mod q_m
//
// pi_g = galois_ntt_source(., k_g): the permutation GPU_Automorphism_NTT applies.  The mapping is automorphism_ntt's
// (galois.hip, the chunk property of DESIGN.md 3.9): a workgroup owns (modulus m, input r, source chunk).  It loads that
// chunk of all D digits -- and of c0 when m < L -- into LDS once, linearly, with 16-byte loads; then, for each of the G
// elements, it walks the ONE destination chunk this source chunk fills: LDS read in permuted order (the low 6 slot bits
// permute within 64 consecutive words: a wave reads a permutation of 64 consecutive words, conflict-free as measured for
// automorphism_ntt), the two key components of element g streamed from global memory with consecutive loads, consecutive
// stores of acc.  Per call every word of a and c0 is read from memory once, every key word once per input and every acc
// word is written once.  Inputs are not blocked per workgroup: the `count` workgroups that share a key tile are adjacent
// in the grid (blockIdx.x = chunk * count + r), so the reuse of key words across inputs rests on L2.
//
// The arithmetic is inner_product's (inner_product_internal.hpp): the exact three-word accumulator, any input word read
// modulo q_m, the three-product fold.  The c0 term is one more exact Shoup product, joined after the first conditional
// subtraction of the fold (see the bound at the store).
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdexcept>

#include "hoisted_rotation_internal.hpp"
#include "inner_product_internal.hpp"
#include "launch.hpp"

namespace gpuntt
{
    namespace kern
    {
        constexpr int HOIST_NT = 256;         // lanes per workgroup at most (a chunk narrower than that gets fewer)
        constexpr size_t HOIST_LDS = 32768;   // the budget of the chunk rule: five workgroups per CU
        constexpr size_t HOIST_LDS_MAX = 65536; // what one workgroup may take at all (D = 64, u64, 64 slots: 33 KiB)

        // the workgroup copies `len` consecutive words of `in` to `tile` (16-byte loads when VEC; no barrier)
        template <typename T, bool VEC> __device__ __forceinline__ void hoist_load(T* tile, const T* __restrict__ in, unsigned len)
        {
            if constexpr (VEC)
            {
                constexpr unsigned V = 16 / sizeof(T);
                struct alignas(16) Vec
                {
                    T x[V];
                };
                for (unsigned v = threadIdx.x; v < len / V; v += blockDim.x) // len is a multiple of V when VEC
                    reinterpret_cast<Vec*>(tile)[v] = reinterpret_cast<const Vec*>(in)[v];
            }
            else
            {
                for (unsigned t = threadIdx.x; t < len; t += blockDim.x)
                    tile[t] = in[t];
            }
        }

        // grid: x = chunk * count + r, y = m; LDS: (D + 1) << logc words; n >= logc (a ring below the chunk is one chunk)
        template <typename T, bool VEC>
        __global__ __launch_bounds__(HOIST_NT) void inner_product_galois(const T* __restrict__ a, const T* __restrict__ c0,
                                                                         T* __restrict__ acc, const T* __restrict__ consts,
                                                                         HoistArgs<T> ha, int D, int count, int L, int M,
                                                                         int KM, int n, int logc, int negacyclic)
        {
            extern __shared__ __align__(16) unsigned char hoist_smem[];
            T* tile = reinterpret_cast<T*>(hoist_smem); // digit d at tile[d << logc], c0 at tile[D << logc]
            const unsigned C = 1u << logc;
            const bool neg = negacyclic != 0;
            const unsigned m = blockIdx.y;
            const unsigned r = blockIdx.x % static_cast<unsigned>(count), chunk = blockIdx.x / static_cast<unsigned>(count);
            const bool with_c0 = c0 != nullptr && m < static_cast<unsigned>(L); // workgroup-uniform

            // all index arithmetic in 64 bits: G * 2 * count * M * N passes 2^32 words at real sizes
            const unsigned long long poly = 1ull << n;
            const unsigned long long stack = static_cast<unsigned long long>(M) << n;           // one input's limbs
            const unsigned long long a_digit = static_cast<unsigned long long>(count) * stack;   // a: [D][count][M][N]
            const unsigned long long key_comp = static_cast<unsigned long long>(KM) << n;        // key: [D][2][KM][N]
            const unsigned long long first = static_cast<unsigned long long>(chunk) << logc;     // the source chunk
            const unsigned long long in_stack = static_cast<unsigned long long>(r) * stack + m * poly;

            const T* src = a + in_stack + first;
            for (int d = 0; d < D; d++)
                hoist_load<T, VEC>(tile + (static_cast<unsigned>(d) << logc), src + d * a_digit, C);
            if (with_c0)
                hoist_load<T, VEC>(tile + (static_cast<unsigned>(D) << logc),
                                   c0 + ((static_cast<unsigned long long>(r) * L + m) << n) + first, C);
            __syncthreads();

            const IpFold<T> fold(consts, M, m);
            const T pq = with_c0 ? ha.p_mod_q[m] : T(0), pqs = with_c0 ? ha.p_mod_q_shoup[m] : T(0);
            const T* tc0 = tile + (static_cast<unsigned>(D) << logc);
            const unsigned long long limb = static_cast<unsigned long long>(ha.limb[m]) * poly;
            for (int g = 0; g < ha.count; g++)
            {
                const std::uint32_t k = ha.elt[g];
                // the chunk this source chunk lands in: where its first slot goes under sigma_k, i.e. the source of
                // that slot under sigma_k^-1 (automorphism_ntt)
                const unsigned dc = galois_ntt_source(chunk << logc, ha.inv[g], n, neg) >> logc;
                const unsigned long long to = static_cast<unsigned long long>(dc) << logc;
                const T* pk = ha.key[g] + limb + to;
                // acc: [G][2][count][M][N], component stride = a_digit
                T* po = acc + static_cast<unsigned long long>(g) * 2ull * a_digit + in_stack + to;
                for (unsigned l = threadIdx.x; l < C; l += blockDim.x)
                {
                    const std::uint32_t j = galois_ntt_source((dc << logc) | l, k, n, neg) & (C - 1u);
                    IpAcc<T> s0{T(0), T(0), 0u}, s1{T(0), T(0), 0u};
                    const T* kd = pk + l;
#pragma unroll 2
                    for (int d = 0; d < D; d++)
                    {
                        const T x = tile[(static_cast<unsigned>(d) << logc) + j];
                        s0.mac(x, kd[0]);
                        s1.mac(x, kd[key_comp]);
                        kd += 2ull * key_comp;
                    }
                    T x0 = fold.sum(s0); // below 3 q
                    if (with_c0)
                    {
                        // one conditional subtraction leaves x0 below 2 q; the c0 term is canonical (an exact Shoup
                        // product of ANY word with P mod q_m < q_m), so the sum stays below 3 q < 2^W -- the bound the
                        // two subtractions of reduce() are for
                        x0 = x0 >= fold.q ? x0 - fold.q : x0;
                        x0 += ip_shoup<T>(tc0[j], pq, pqs, fold.q);
                    }
                    po[l] = fold.reduce(x0);
                    po[a_digit + l] = fold.reduce(fold.sum(s1));
                }
            }
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            std::atomic<int> g_hoist_chunk{0}; // test hook keyswitch_hoist_chunk
        }
        void keyswitch_set_hoist_chunk(int v) { g_hoist_chunk.store(v, std::memory_order_relaxed); }

        int hoist_chunk_log(size_t word_bytes, int D, int n_power)
        {
            const size_t rows = static_cast<size_t>(D) + 1;
            int lc = g_hoist_chunk.load(std::memory_order_relaxed);
            if (lc > 0)
                while (lc > 6 && (rows << lc) * word_bytes > kern::HOIST_LDS_MAX) // a forced chunk still has to fit
                    lc--;
            else
                for (lc = 6; (rows << (lc + 1)) * word_bytes <= kern::HOIST_LDS; lc++)
                    ;
            return lc < n_power ? lc : n_power;
        }

        template <typename T>
        void hoist_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistArgs<T>& args, int D,
                          int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream)
        {
            const int logc = hoist_chunk_log(sizeof(T), D, n_power);
            unsigned nt = 64;
            while (nt < static_cast<unsigned>(kern::HOIST_NT) && nt < (1u << logc))
                nt *= 2;
            const unsigned long long blocks = static_cast<unsigned long long>(count) << (n_power - logc);
            if (blocks * nt > 0xFFFFFFFFull) // HIP caps a launch at 2^32 - 1 work-items per dimension
                throw std::invalid_argument("Invalid count!");
            const size_t lds = ((static_cast<size_t>(D) + 1) << logc) * sizeof(T);
            const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(M));
            // a 16-byte group must stay inside one chunk and be aligned (every stride is a multiple of N words)
            const bool wide = ((sizeof(T) << logc) % 16 == 0) &&
                              ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(c0)) & 15u) == 0;
            if (wide)
                GPUNTT_LAUNCH((kern::inner_product_galois<T, true>), grid, dim3(nt), lds, stream, a, c0, acc, consts, args,
                              D, count, L, M, KM, n_power, logc, negacyclic ? 1 : 0);
            else
                GPUNTT_LAUNCH((kern::inner_product_galois<T, false>), grid, dim3(nt), lds, stream, a, c0, acc, consts,
                              args, D, count, L, M, KM, n_power, logc, negacyclic ? 1 : 0);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        template void hoist_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                           const kern::HoistArgs<Data32>&, int, int, int, int, int, int, bool, hipStream_t);
        template void hoist_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                           const kern::HoistArgs<Data64>&, int, int, int, int, int, int, bool, hipStream_t);
    } // namespace host
} // namespace gpuntt
