// hoisted_rotation.hip -- the two inner products of hybrid key switching for G rotations of ONE decomposition
// (KeySwitchPlan<T>::rotate_hoisted and rotate_hoisted_sum, include/gpuntt/rns/key_switch.cuh).  Both form, per slot,
//
//   u_g[c][r][m][j] = ( sum_{d<D} a[d][r][m][pi_g(j)] * key_g[d][c][limb(m)][j]
//                       + [c = 0, m < L, c0 != null] (P mod q_m) * c0[r][m][pi_g(j)] ) mod q_m
//
// with pi_g = galois_ntt_source(., k_g): the permutation GPU_Automorphism_NTT applies.
//
//   inner_product_galois:      acc[g][c][r][m][j] = u_g[c][r][m][j]                                   -- G rotations
//   inner_product_galois_sum:  acc[c][r][m][j] = ( sum_{g<G} w_g[m][j] * u_g[c][r][m][j] ) mod q_m    -- "double hoisting"
//
// What they share is hoist_term (one copy of u_g), HoistIndex (the strides, the indices and the tile load), HoistC0 and
// hoist_load.
//
// inner_product_galois: the mapping is automorphism_ntt's (galois.hip, the chunk property of DESIGN.md 3.9): a workgroup
// owns (modulus m, input r, SOURCE chunk).  It loads that chunk of all D digits -- and of c0 when m < L -- into LDS once,
// linearly, with 16-byte loads; then, for each of the G elements, it walks the ONE destination chunk this source chunk
// fills: LDS read in permuted order (the low 6 slot bits permute within 64 consecutive words: a wave reads a permutation
// of 64 consecutive words, conflict-free as measured for automorphism_ntt), the two key components of element g streamed
// from global memory with consecutive loads, consecutive stores of acc.  Per call every word of a and c0 is read from
// memory once, every key word once per input and every acc word is written once.  Inputs are not blocked per workgroup:
// the `count` workgroups that share a key tile are adjacent in the grid (blockIdx.x = chunk * count + r), so the reuse of
// key words across inputs rests on L2.
//
// inner_product_galois_sum: a workgroup that owns source chunks scatters every element to another destination chunk, so
// it cannot sum over g.  Here a workgroup owns (modulus m, input r, DESTINATION chunk), one slot per lane.  By the chunk
// property the chunk is filled from exactly one source chunk per element: for each g the workgroup finds it (the source of
// the chunk's first slot), loads that chunk of all D digits -- and of c0 when m < L -- into LDS, waits, forms u_g for its
// slot, multiplies by the weight word (consecutive loads) into a second pair of exact three-word accumulators that lives
// in registers across the g loop, and waits again before the next element overwrites the tile.  After the last g: one
// fold per component, consecutive stores.  The price of owning destinations: every word of a (and c0) is read once PER
// ELEMENT, where inner_product_galois reads it once per call.
//
// The arithmetic is inner_product's (inner_product_internal.hpp): the exact three-word accumulator, any input word read
// modulo q_m, the three-product fold.  The c0 term is one more exact Shoup product, joined after the first conditional
// subtraction of the fold (see the bound in hoist_term).  The value inner_product_galois_sum hands to the across-g
// accumulator is the UNREDUCED fold sum (below 3 q < 2^W): mac is exact for any two words, so neither u_g nor the weight
// (any word, read modulo q_m by the final fold) is reduced per element, and at most 64 terms leave the carry word at 64.
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

        // What a workgroup derives once from its place in the grid (x = chunk * count + r, y = m): all workgroup-uniform.
        // All index arithmetic in 64 bits: G * 2 * count * M * N passes 2^32 words at real sizes.  The constructor reads no
        // memory, so it can stand in front of the first tile load
        template <typename T> struct HoistIndex
        {
            unsigned C, m, r, chunk;
            bool neg, with_c0;
            unsigned long long poly, a_digit, key_comp, in_stack;
            __device__ __forceinline__ HoistIndex(const T* c0, int count, int L, int M, int KM, int n, int logc,
                                                  int negacyclic)
            {
                C = 1u << logc;
                neg = negacyclic != 0;
                m = blockIdx.y;
                r = blockIdx.x % static_cast<unsigned>(count), chunk = blockIdx.x / static_cast<unsigned>(count);
                with_c0 = c0 != nullptr && m < static_cast<unsigned>(L);
                poly = 1ull << n;
                const unsigned long long stack = static_cast<unsigned long long>(M) << n; // one input's limbs
                a_digit = static_cast<unsigned long long>(count) * stack;                  // a: [D][count][M][N]
                key_comp = static_cast<unsigned long long>(KM) << n;                       // key: [D][2][KM][N]
                in_stack = static_cast<unsigned long long>(r) * stack + m * poly;
            }
            // where the key limb of modulus m starts inside a key component, in words
            __device__ __forceinline__ unsigned long long key_limb(const HoistArgs<T>& ha) const
            {
                return static_cast<unsigned long long>(ha.limb[m]) * poly;
            }
            // the source chunk at word `first` of all D digits -- and of c0 -- to the tile: digit d at tile[d << logc],
            // c0 at tile[D << logc] (no barrier)
            template <bool VEC>
            __device__ __forceinline__ void load(T* tile, const T* __restrict__ a, const T* __restrict__ c0,
                                                 unsigned long long first, int D, int L, int n, int logc) const
            {
                const T* src = a + in_stack + first;
                for (int d = 0; d < D; d++)
                    hoist_load<T, VEC>(tile + (static_cast<unsigned>(d) << logc), src + d * a_digit, C);
                if (with_c0)
                    hoist_load<T, VEC>(tile + (static_cast<unsigned>(D) << logc),
                                       c0 + ((static_cast<unsigned long long>(r) * L + m) << n) + first, C);
            }
        };

        // The c0 term of a workgroup.  The kernels fill it themselves, from their own argument (two scalar loads): read
        // through a reference to HoistArgs inside a helper, the same two loads took the u64 inner_product_galois_sum
        // from 56 / 60 to 78 / 82 VGPRs
        template <typename T> struct HoistC0
        {
            T pq, pqs;     // P mod q_m and its Shoup companion (0 when off)
            const T* tile; // c0's chunk in LDS: tile + (D << logc)
            bool on;       // m < L and the call has a c0
        };

        // u_g of one slot, both components, as UNREDUCED fold sums below 3 q: x0 (component 0, the c0 term joined) and
        // x1.  j: the slot's source index inside the tile; kd: the slot's word of digit 0, component 0 of key_g.  All but
        // j and kd are workgroup-uniform
        template <typename T>
        __device__ __forceinline__ void hoist_term(const T* tile, std::uint32_t j, const T* kd, int D, int logc,
                                                   unsigned long long key_comp, const IpFold<T>& fold,
                                                   const HoistC0<T>& c0, T& x0, T& x1)
        {
            IpAcc<T> s0{T(0), T(0), 0u}, s1{T(0), T(0), 0u};
#pragma unroll 2
            for (int d = 0; d < D; d++)
            {
                const T x = tile[(static_cast<unsigned>(d) << logc) + j];
                s0.mac(x, kd[0]);
                s1.mac(x, kd[key_comp]);
                kd += 2ull * key_comp;
            }
            x0 = fold.sum(s0); // below 3 q
            if (c0.on)
            {
                // one conditional subtraction leaves x0 below 2 q; the c0 term is canonical (an exact Shoup product of
                // ANY word with P mod q_m < q_m), so the sum stays below 3 q < 2^W -- the bound the two subtractions of
                // reduce() are for
                x0 = x0 >= fold.q ? x0 - fold.q : x0;
                x0 += rns_shoup<T>(c0.tile[j], c0.pq, c0.pqs, fold.q);
            }
            x1 = fold.sum(s1);
        }

        extern __shared__ __align__(16) unsigned char hoist_smem[]; // (D + 1) << logc words, both kernels

        // grid: x = chunk * count + r, y = m; LDS: (D + 1) << logc words; n >= logc (a ring below the chunk is one chunk)
        template <typename T, bool VEC>
        __global__ __launch_bounds__(HOIST_NT) void inner_product_galois(const T* __restrict__ a, const T* __restrict__ c0,
                                                                         T* __restrict__ acc, const T* __restrict__ consts,
                                                                         HoistArgs<T> ha, int D, int count, int L, int M,
                                                                         int KM, int n, int logc, int negacyclic)
        {
            T* tile = reinterpret_cast<T*>(hoist_smem);
            const HoistIndex<T> ix(c0, count, L, M, KM, n, logc, negacyclic);
            ix.template load<VEC>(tile, a, c0, static_cast<unsigned long long>(ix.chunk) << logc, D, L, n, logc);
            __syncthreads();

            const IpFold<T> fold(consts, M, ix.m);
            const HoistC0<T> pc0{ix.with_c0 ? ha.p_mod_q[ix.m] : T(0), ix.with_c0 ? ha.p_mod_q_shoup[ix.m] : T(0),
                                 tile + (static_cast<unsigned>(D) << logc), ix.with_c0};
            const unsigned long long limb = ix.key_limb(ha);
            for (int g = 0; g < ha.count; g++)
            {
                const std::uint32_t k = ha.elt[g];
                // the chunk this source chunk lands in: where its first slot goes under sigma_k, i.e. the source of
                // that slot under sigma_k^-1 (automorphism_ntt)
                const unsigned dc = galois_ntt_source(ix.chunk << logc, ha.inv[g], n, ix.neg) >> logc;
                const unsigned long long to = static_cast<unsigned long long>(dc) << logc;
                const T* pk = ha.key[g] + limb + to;
                // acc: [G][2][count][M][N], component stride = a_digit
                T* po = acc + static_cast<unsigned long long>(g) * 2ull * ix.a_digit + ix.in_stack + to;
                for (unsigned l = threadIdx.x; l < ix.C; l += blockDim.x)
                {
                    const std::uint32_t j = galois_ntt_source((dc << logc) | l, k, n, ix.neg) & (ix.C - 1u);
                    T x0, x1;
                    hoist_term<T>(tile, j, pk + l, D, logc, ix.key_comp, fold, pc0, x0, x1);
                    po[l] = fold.reduce(x0);
                    po[ix.a_digit + l] = fold.reduce(x1);
                }
            }
        }

        // grid: x = chunk * count + r, y = m; block: max(64, 1 << logc) lanes; LDS: (D + 1) << logc words; n >= logc
        template <typename T, bool VEC>
        __global__ __launch_bounds__(HOIST_NT) void inner_product_galois_sum(const T* __restrict__ a,
                                                                             const T* __restrict__ c0, T* __restrict__ acc,
                                                                             const T* __restrict__ consts,
                                                                             HoistSumArgs<T> ha, int D, int count, int L,
                                                                             int M, int KM, int n, int logc, int negacyclic)
        {
            T* tile = reinterpret_cast<T*>(hoist_smem);
            const HoistIndex<T> ix(c0, count, L, M, KM, n, logc, negacyclic);
            const unsigned l = threadIdx.x;
            const bool owner = l < ix.C; // a ring below 64 slots leaves lanes without a slot; they still load and wait
            const unsigned long long to = static_cast<unsigned long long>(ix.chunk) << logc; // the destination chunk
            const IpFold<T> fold(consts, M, ix.m);
            const HoistC0<T> pc0{ix.with_c0 ? ha.h.p_mod_q[ix.m] : T(0), ix.with_c0 ? ha.h.p_mod_q_shoup[ix.m] : T(0),
                                 tile + (static_cast<unsigned>(D) << logc), ix.with_c0};
            const unsigned long long limb = ix.key_limb(ha.h);
            const unsigned slot = (ix.chunk << logc) | (owner ? l : 0u);

            IpAcc<T> t0{T(0), T(0), 0u}, t1{T(0), T(0), 0u}; // sum_g w_g u_g, exact, across the g loop
            for (int g = 0; g < ha.h.count; g++)
            {
                const std::uint32_t k = ha.h.elt[g];
                // the ONE source chunk this destination chunk is filled from under sigma_k: where its first slot reads
                const unsigned long long first =
                    static_cast<unsigned long long>(galois_ntt_source(ix.chunk << logc, k, n, ix.neg) >> logc) << logc;
                ix.template load<VEC>(tile, a, c0, first, D, L, n, logc);
                __syncthreads();
                if (owner)
                {
                    const std::uint32_t j = galois_ntt_source(slot, k, n, ix.neg) & (ix.C - 1u);
                    T x0, x1;
                    hoist_term<T>(tile, j, ha.h.key[g] + limb + to + l, D, logc, ix.key_comp, fold, pc0, x0, x1);
                    const T* pw = ha.weight[g]; // workgroup-uniform
                    const T w = pw != nullptr ? pw[ix.m * ix.poly + to + l] : T(1);
                    t0.mac(x0, w);
                    t1.mac(x1, w);
                }
                __syncthreads(); // the next element loads another source chunk over this one
            }
            if (owner)
            {
                T* po = acc + ix.in_stack + to + l; // acc: [2][count][M][N], component stride = a_digit
                po[0] = fold.reduce(fold.sum(t0));
                po[ix.a_digit] = fold.reduce(fold.sum(t1));
            }
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            std::atomic<int> g_hoist_chunk{0}; // test hook keyswitch_hoist_chunk, for both kernels
        }
        void keyswitch_set_hoist_chunk(int v) { g_hoist_chunk.store(v, std::memory_order_relaxed); }

        int hoist_chunk_log(size_t word_bytes, int D, int n_power, int max_log)
        {
            const size_t rows = static_cast<size_t>(D) + 1;
            int lc = g_hoist_chunk.load(std::memory_order_relaxed);
            if (lc > 0)
            {
                lc = lc < max_log ? lc : max_log;
                while (lc > 6 && (rows << lc) * word_bytes > kern::HOIST_LDS_MAX) // a forced chunk still has to fit
                    lc--;
            }
            else
                for (lc = 6; lc < max_log && (rows << (lc + 1)) * word_bytes <= kern::HOIST_LDS; lc++)
                    ;
            return lc < n_power ? lc : n_power;
        }

        namespace
        {
            // what the two launches share: the chunk, the grid with its limit, the LDS bytes and whether the loaders
            // may use 16-byte groups; `launch(grid, nt, lds, logc, wide)` enqueues the kernel
            template <typename T, typename Launch>
            void hoist_dispatch(const T* a, const T* c0, int D, int count, int M, int n_power, int max_log, Launch launch)
            {
                const int logc = hoist_chunk_log(sizeof(T), D, n_power, max_log);
                unsigned nt = 64; // one lane per slot, between a wave and HOIST_NT
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
                launch(grid, dim3(nt), lds, logc, wide);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }
        } // namespace

        template <typename T>
        void hoist_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistArgs<T>& args, int D,
                          int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream)
        {
            hoist_dispatch<T>(a, c0, D, count, M, n_power, HOIST_LOG_MAX,
                              [&](dim3 grid, dim3 block, size_t lds, int logc, bool wide) {
                                  if (wide)
                                      GPUNTT_LAUNCH((kern::inner_product_galois<T, true>), grid, block, lds, stream, a, c0,
                                                    acc, consts, args, D, count, L, M, KM, n_power, logc, negacyclic ? 1 : 0);
                                  else
                                      GPUNTT_LAUNCH((kern::inner_product_galois<T, false>), grid, block, lds, stream, a, c0,
                                                    acc, consts, args, D, count, L, M, KM, n_power, logc, negacyclic ? 1 : 0);
                              });
        }

        template <typename T>
        void hoist_sum_launch(const T* a, const T* c0, T* acc, const T* consts, const kern::HoistSumArgs<T>& args, int D,
                              int count, int L, int M, int KM, int n_power, bool negacyclic, hipStream_t stream)
        {
            hoist_dispatch<T>(a, c0, D, count, M, n_power, HOIST_SUM_LOG_MAX,
                              [&](dim3 grid, dim3 block, size_t lds, int logc, bool wide) {
                                  if (wide)
                                      GPUNTT_LAUNCH((kern::inner_product_galois_sum<T, true>), grid, block, lds, stream, a,
                                                    c0, acc, consts, args, D, count, L, M, KM, n_power, logc,
                                                    negacyclic ? 1 : 0);
                                  else
                                      GPUNTT_LAUNCH((kern::inner_product_galois_sum<T, false>), grid, block, lds, stream, a,
                                                    c0, acc, consts, args, D, count, L, M, KM, n_power, logc,
                                                    negacyclic ? 1 : 0);
                              });
        }

        template void hoist_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                           const kern::HoistArgs<Data32>&, int, int, int, int, int, int, bool, hipStream_t);
        template void hoist_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                           const kern::HoistArgs<Data64>&, int, int, int, int, int, int, bool, hipStream_t);
        template void hoist_sum_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                               const kern::HoistSumArgs<Data32>&, int, int, int, int, int, int, bool,
                                               hipStream_t);
        template void hoist_sum_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                               const kern::HoistSumArgs<Data64>&, int, int, int, int, int, int, bool,
                                               hipStream_t);
    } // namespace host
} // namespace gpuntt
