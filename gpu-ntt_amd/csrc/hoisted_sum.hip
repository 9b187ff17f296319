// hoisted_sum.hip -- inner_product_galois_sum: the inner product of hybrid key switching for G rotations of ONE
// decomposition, weighted and SUMMED over the rotations before anything leaves the extended base
// (KeySwitchPlan<T>::rotate_hoisted_sum, include/gpuntt/rns/key_switch.cuh; "double hoisting").
//
//   u_g[c][r][m][j] = ( sum_{d<D} a[d][r][m][pi_g(j)] * key_g[d][c][limb(m)][j]
//                       + [c = 0, m < L, c0 != null] (P mod q_m) * c0[r][m][pi_g(j)] ) mod q_m   -- inner_product_galois
//   acc[c][r][m][j] = ( sum_{g<G} w_g[m][j] * u_g[c][r][m][j] ) mod q_m                          -- canonical
//
// inner_product_galois (hoisted_rotation.hip) owns SOURCE chunks and scatters every element to another destination
// chunk, so it cannot sum over g.  Here a workgroup owns (modulus m, input r, DESTINATION chunk), one slot per lane.
// By the chunk property the chunk is filled from exactly one source chunk per element: for each g the
// workgroup finds it (the source of the chunk's first slot), loads that chunk of all D digits -- and of c0 when m < L --
// into LDS linearly with 16-byte loads, waits, forms u_g for its slot as inner_product_galois does (LDS read in permuted
// order: a wave reads a permutation of 64 consecutive words; the two key components streamed with consecutive loads),
// multiplies by the weight word (consecutive loads) into a second pair of exact three-word accumulators that lives in
// registers across the g loop, and waits again before the next element overwrites the tile.  After the last g: one fold
// per component, consecutive stores.  The price of owning destinations: every word of a (and c0) is read once PER
// ELEMENT, where inner_product_galois reads it once per call.
//
// The arithmetic is inner_product's (inner_product_internal.hpp), no second copy.  The value handed to the across-g
// accumulator is the UNREDUCED fold sum (below 3 q < 2^W): mac is exact for any two words, so neither u_g nor the weight
// (any word, read modulo q_m by the final fold) is reduced per element, and at most 64 terms leave the carry word at 64.
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdexcept>

#include "hoisted_sum_internal.hpp"
#include "inner_product_internal.hpp"
#include "launch.hpp"

namespace gpuntt
{
    namespace kern
    {
        constexpr int HSUM_NT = 256;           // lanes per workgroup at most = slots per chunk at most (one slot per lane)
        constexpr int HSUM_LOG_MAX = 8;        // log2(HSUM_NT)
        constexpr size_t HSUM_LDS = 32768;     // the budget of the chunk rule
        constexpr size_t HSUM_LDS_MAX = 65536; // what one workgroup may take at all (D = 64, u64, 64 slots: 33 KiB)

        // the workgroup copies `len` consecutive words of `in` to `tile` (16-byte loads when VEC; no barrier)
        template <typename T, bool VEC> __device__ __forceinline__ void hsum_load(T* tile, const T* __restrict__ in, unsigned len)
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

        // grid: x = chunk * count + r, y = m; block: max(64, 1 << logc) lanes; LDS: (D + 1) << logc words; n >= logc
        template <typename T, bool VEC>
        __global__ __launch_bounds__(HSUM_NT) void inner_product_galois_sum(const T* __restrict__ a,
                                                                             const T* __restrict__ c0, T* __restrict__ acc,
                                                                             const T* __restrict__ consts,
                                                                             HoistSumArgs<T> ha, int D, int count, int L,
                                                                             int M, int KM, int n, int logc, int negacyclic)
        {
            extern __shared__ __align__(16) unsigned char hsum_smem[];
            T* tile = reinterpret_cast<T*>(hsum_smem); // digit d at tile[d << logc], c0 at tile[D << logc]
            const unsigned C = 1u << logc;
            const bool neg = negacyclic != 0;
            const unsigned m = blockIdx.y;
            const unsigned r = blockIdx.x % static_cast<unsigned>(count), chunk = blockIdx.x / static_cast<unsigned>(count);
            const bool with_c0 = c0 != nullptr && m < static_cast<unsigned>(L); // workgroup-uniform
            const unsigned l = threadIdx.x;
            const bool owner = l < C; // a ring below 64 slots leaves lanes without a slot; they still load and wait

            // all index arithmetic in 64 bits, as in inner_product_galois
            const unsigned long long poly = 1ull << n;
            const unsigned long long stack = static_cast<unsigned long long>(M) << n;           // one input's limbs
            const unsigned long long a_digit = static_cast<unsigned long long>(count) * stack;   // a: [D][count][M][N]
            const unsigned long long key_comp = static_cast<unsigned long long>(KM) << n;        // key: [D][2][KM][N]
            const unsigned long long to = static_cast<unsigned long long>(chunk) << logc;        // the destination chunk
            const unsigned long long in_stack = static_cast<unsigned long long>(r) * stack + m * poly;

            const IpFold<T> fold(consts, M, m);
            const T pq = with_c0 ? ha.h.p_mod_q[m] : T(0), pqs = with_c0 ? ha.h.p_mod_q_shoup[m] : T(0);
            const T* tc0 = tile + (static_cast<unsigned>(D) << logc);
            const unsigned long long limb = static_cast<unsigned long long>(ha.h.limb[m]) * poly;
            const unsigned slot = (chunk << logc) | (owner ? l : 0u);

            IpAcc<T> t0{T(0), T(0), 0u}, t1{T(0), T(0), 0u}; // sum_g w_g u_g, exact, across the g loop
            for (int g = 0; g < ha.h.count; g++)
            {
                const std::uint32_t k = ha.h.elt[g];
                // the ONE source chunk this destination chunk is filled from under sigma_k: where its first slot reads
                const unsigned long long first =
                    static_cast<unsigned long long>(galois_ntt_source(chunk << logc, k, n, neg) >> logc) << logc;
                const T* src = a + in_stack + first;
                for (int d = 0; d < D; d++)
                    hsum_load<T, VEC>(tile + (static_cast<unsigned>(d) << logc), src + d * a_digit, C);
                if (with_c0)
                    hsum_load<T, VEC>(tile + (static_cast<unsigned>(D) << logc),
                                      c0 + ((static_cast<unsigned long long>(r) * L + m) << n) + first, C);
                __syncthreads();
                if (owner)
                {
                    const std::uint32_t j = galois_ntt_source(slot, k, n, neg) & (C - 1u);
                    IpAcc<T> s0{T(0), T(0), 0u}, s1{T(0), T(0), 0u};
                    const T* kd = ha.h.key[g] + limb + to + l;
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
                        // as in inner_product_galois: one conditional subtraction leaves x0 below 2 q, the c0 term is
                        // canonical, the sum stays below 3 q < 2^W
                        x0 = x0 >= fold.q ? x0 - fold.q : x0;
                        x0 += ip_shoup<T>(tc0[j], pq, pqs, fold.q);
                    }
                    const T* pw = ha.weight[g]; // workgroup-uniform
                    const T w = pw != nullptr ? pw[m * poly + to + l] : T(1);
                    t0.mac(x0, w);
                    t1.mac(fold.sum(s1), w);
                }
                __syncthreads(); // the next element loads another source chunk over this one
            }
            if (owner)
            {
                T* po = acc + in_stack + to + l; // acc: [2][count][M][N], component stride = a_digit
                po[0] = fold.reduce(fold.sum(t0));
                po[a_digit] = fold.reduce(fold.sum(t1));
            }
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            std::atomic<int> g_hoist_sum_chunk{0}; // test hook keyswitch_hoist_chunk (shared with inner_product_galois)
        }
        void keyswitch_set_hoist_sum_chunk(int v) { g_hoist_sum_chunk.store(v, std::memory_order_relaxed); }

        int hoist_sum_chunk_log(size_t word_bytes, int D, int n_power)
        {
            const size_t rows = static_cast<size_t>(D) + 1;
            int lc = g_hoist_sum_chunk.load(std::memory_order_relaxed);
            if (lc > 0)
            {
                lc = lc < kern::HSUM_LOG_MAX ? lc : kern::HSUM_LOG_MAX; // one slot per lane: a forced chunk has to fit
                while (lc > 6 && (rows << lc) * word_bytes > kern::HSUM_LDS_MAX)
                    lc--;
            }
            else
                for (lc = 6; lc < kern::HSUM_LOG_MAX && (rows << (lc + 1)) * word_bytes <= kern::HSUM_LDS; lc++)
                    ;
            return lc < n_power ? lc : n_power;
        }

        template <typename T>
        void hoist_sum_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistSumArgs<T>& args, int D,
                              int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream)
        {
            const int logc = hoist_sum_chunk_log(sizeof(T), D, n_power);
            const unsigned nt = logc > 6 ? (1u << logc) : 64u;
            const unsigned long long blocks = static_cast<unsigned long long>(count) << (n_power - logc);
            if (blocks * nt > 0xFFFFFFFFull) // HIP caps a launch at 2^32 - 1 work-items per dimension
                throw std::invalid_argument("Invalid count!");
            const size_t lds = ((static_cast<size_t>(D) + 1) << logc) * sizeof(T);
            const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(M));
            // a 16-byte group must stay inside one chunk and be aligned (every stride is a multiple of N words)
            const bool wide = ((sizeof(T) << logc) % 16 == 0) &&
                              ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(c0)) & 15u) == 0;
            if (wide)
                GPUNTT_LAUNCH((kern::inner_product_galois_sum<T, true>), grid, dim3(nt), lds, stream, a, c0, acc, consts,
                              args, D, count, L, M, KM, n_power, logc, negacyclic ? 1 : 0);
            else
                GPUNTT_LAUNCH((kern::inner_product_galois_sum<T, false>), grid, dim3(nt), lds, stream, a, c0, acc, consts,
                              args, D, count, L, M, KM, n_power, logc, negacyclic ? 1 : 0);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        template void hoist_sum_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                               const kern::HoistSumArgs<Data32>&, int, int, int, int, int, int, bool,
                                               hipStream_t);
        template void hoist_sum_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                               const kern::HoistSumArgs<Data64>&, int, int, int, int, int, int, bool,
                                               hipStream_t);
    } // namespace host
} // namespace gpuntt
