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
//
// linear_transform_bsgs (the double-hoisted baby-step/giant-step transform) adds three kernels behind the
// two above: bsgs_scale_input (the baby steps without a key), bsgs_weighted_sum (all n2 weighted sums of the n1 baby
// accumulators from one read of them) and inner_product_galois_giant (inner_product_galois_sum's mapping over the giant
// steps: the re-decomposed digits against the giant keys plus the first component, summed over g).  They share
// hoist_term, HoistIndex, HoistC0 and hoist_load with the two above.
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

        // ---- linear_transform_bsgs.  S = count * M * N words: one component of `count` stacks ----

        // The baby steps WITHOUT a key (element 1): u[b][c][r][m][j] = [m < L] (P mod q_m) * c_c[r][m][j] mod q_m for
        // first <= b < n1, c_0 = c0 (zero when null), c_1 = c1; zeros on the special limbs.  One word per lane; every such
        // b holds the same words, so the product is formed once and stored n1 - first times.
        // grid: x = tile * (2 count) + c * count + r, y = m; u: T[n1][2][count][M][N]
        template <typename T>
        __global__ __launch_bounds__(HOIST_NT) void bsgs_scale_input(const T* __restrict__ c0, const T* __restrict__ c1,
                                                                     T* __restrict__ u, const T* __restrict__ consts,
                                                                     HoistArgs<T> ha, int first, int n1, int count, int L,
                                                                     int M, int n)
        {
            const unsigned m = blockIdx.y;
            const unsigned both = 2u * static_cast<unsigned>(count);
            const unsigned cr = blockIdx.x % both, c = cr / static_cast<unsigned>(count);
            const unsigned r = cr % static_cast<unsigned>(count);
            const unsigned long long col = static_cast<unsigned long long>(blockIdx.x / both) * blockDim.x + threadIdx.x;
            if (col >= (1ull << n))
                return;
            const T* src = c == 0 ? c0 : c1;
            T x = 0;
            if (m < static_cast<unsigned>(L) && src != nullptr)
            {
                const IpFold<T> fold(consts, M, m);
                x = rns_shoup<T>(src[((static_cast<unsigned long long>(r) * L + m) << n) + col], ha.p_mod_q[m],
                                 ha.p_mod_q_shoup[m], fold.q); // canonical for ANY word
            }
            const unsigned long long stack = static_cast<unsigned long long>(M) << n, group = count * stack;
            T* po = u + c * group + r * stack + (static_cast<unsigned long long>(m) << n) + col;
            for (int b = first; b < n1; b++)
                po[static_cast<unsigned long long>(b) * 2ull * group] = x;
        }

        // v[c][g][r][m][j] = (sum_{b: present} w_{g,b}[m][j] * u[b][c][r][m][j]) mod q_m: all n2 weighted sums from ONE read
        // of the n1 baby accumulators.  A lane owns V consecutive columns of one (c, r, m): it parks its n1 groups in LDS
        // at [b][lane] -- a lane only reads back what it wrote: no barrier -- then walks the n2 rows; the exact three-word
        // accumulator takes any two words (the weight is read modulo q_m by the fold), at most 64 terms, one fold per
        // output.  The weights are re-read per (c, r): the 2 * count workgroups that share a weight tile are adjacent in
        // the grid, so that reuse rests on L2.
        // grid: x = tile * (2 count) + c * count + r, y = m; LDS: n1 * blockDim.x * V words;
        // u: T[n1][2][count][M][N], v: T[2][n2][count][M][N]
        template <typename T, int V>
        __global__ __launch_bounds__(HOIST_NT) void bsgs_weighted_sum(const T* __restrict__ u, T* __restrict__ v,
                                                                      const T* __restrict__ consts, BsgsWeights<T> wa,
                                                                      int count, int M, int n)
        {
            using Vec = IpVec<T, V>;
            const unsigned m = blockIdx.y;
            const unsigned both = 2u * static_cast<unsigned>(count);
            const unsigned cr = blockIdx.x % both, c = cr / static_cast<unsigned>(count);
            const unsigned r = cr % static_cast<unsigned>(count);
            const unsigned long long col =
                (static_cast<unsigned long long>(blockIdx.x / both) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n))
                return; // (no barrier below)
            const unsigned long long stack = static_cast<unsigned long long>(M) << n, group = count * stack;
            const unsigned long long limb = (static_cast<unsigned long long>(m) << n) + col; // inside one T[M][N]
            const unsigned long long at = r * stack + limb;
            Vec* mine = reinterpret_cast<Vec*>(hoist_smem) + threadIdx.x; // row b at mine[b * blockDim.x]
            const T* pu = u + c * group + at;
            for (int b = 0; b < wa.n1; b++)
                mine[static_cast<unsigned>(b) * blockDim.x] =
                    *reinterpret_cast<const Vec*>(pu + static_cast<unsigned long long>(b) * 2ull * group);

            const IpFold<T> fold(consts, M, m);
            T* pv = v + static_cast<unsigned long long>(c) * wa.n2 * group + at;
            for (int g = 0; g < wa.n2; g++)
            {
                IpAcc<T> s[V];
#pragma unroll
                for (int i = 0; i < V; i++)
                    s[i] = IpAcc<T>{T(0), T(0), 0u};
                for (int b = 0; b < wa.n1; b++)
                {
                    const T* pw = wa.w[g * wa.n1 + b]; // workgroup-uniform
                    if (pw == nullptr)
                        continue; // the term is absent
                    const Vec x = mine[static_cast<unsigned>(b) * blockDim.x];
                    const Vec w = *reinterpret_cast<const Vec*>(pw + limb);
#pragma unroll
                    for (int i = 0; i < V; i++)
                        s[i].mac(x.x[i], w.x[i]);
                }
                Vec o;
#pragma unroll
                for (int i = 0; i < V; i++)
                    o.x[i] = fold.reduce(fold.sum(s[i]));
                *reinterpret_cast<Vec*>(pv + static_cast<unsigned long long>(g) * group) = o;
            }
        }

        // The giant steps, summed: inner_product_galois_sum's mapping -- a workgroup owns (modulus m, input r, DESTINATION
        // chunk), one slot per lane -- over the n2k = ha.count giant steps WITH a key.  For each it loads the source chunk
        // of the D digits of row g * count + r of a (the re-decomposed second components) and, in c0's place in the tile,
        // of v[0][g] -- for EVERY m < M, with multiplier 1: v already lives at scale P -- and forms the term with
        // hoist_term.  The v word is read modulo q_m (one Shoup product against the companion of 1), so after the one
        // conditional subtraction the sum stays below 3 q, hoist_term's own bound.  The terms, unreduced, and the two
        // components of the giant steps WITHOUT a key (element 1: no permutation, read at the lane's own slot) go into the
        // exact accumulators across g: at most 64 additions of words, one fold per component.
        // grid: x = chunk * count + r, y = m; block: max(64, 1 << logc) lanes; LDS: (D + 1) << logc words; n >= logc;
        // a: T[D][n2k * count][M][N], v: T[2][n2][count][M][N] (the keyed steps first), acc: T[2][count][M][N]
        template <typename T, bool VEC>
        __global__ __launch_bounds__(HOIST_NT) void inner_product_galois_giant(const T* __restrict__ a,
                                                                               const T* __restrict__ v, T* __restrict__ acc,
                                                                               const T* __restrict__ consts,
                                                                               HoistArgs<T> ha, int n2, int D, int count,
                                                                               int M, int KM, int n, int logc,
                                                                               int negacyclic)
        {
            T* tile = reinterpret_cast<T*>(hoist_smem);
            const HoistIndex<T> ix(nullptr, count, 0, M, KM, n, logc, negacyclic);
            const unsigned l = threadIdx.x;
            const bool owner = l < ix.C;
            const unsigned long long to = static_cast<unsigned long long>(ix.chunk) << logc; // the destination chunk
            const IpFold<T> fold(consts, M, ix.m);
            const HoistC0<T> pv{T(1), fold.onep, tile + (static_cast<unsigned>(D) << logc), true};
            const unsigned long long limb = ix.key_limb(ha);
            const unsigned slot = (ix.chunk << logc) | (owner ? l : 0u);
            const unsigned long long group = ix.a_digit; // `count` stacks: one giant step of a component of v
            const unsigned long long digit = static_cast<unsigned long long>(ha.count) * group;
            const T* v1 = v + static_cast<unsigned long long>(n2) * group;

            IpAcc<T> t0{T(0), T(0), 0u}, t1{T(0), T(0), 0u}; // sum_g s_g, exact, across the g loop
            for (int g = 0; g < ha.count; g++)
            {
                const std::uint32_t k = ha.elt[g];
                const unsigned long long first =
                    static_cast<unsigned long long>(galois_ntt_source(ix.chunk << logc, k, n, ix.neg) >> logc) << logc;
                const unsigned long long src = static_cast<unsigned long long>(g) * group + ix.in_stack + first;
                for (int d = 0; d < D; d++)
                    hoist_load<T, VEC>(tile + (static_cast<unsigned>(d) << logc), a + d * digit + src, ix.C);
                hoist_load<T, VEC>(tile + (static_cast<unsigned>(D) << logc), v + src, ix.C);
                __syncthreads();
                if (owner)
                {
                    const std::uint32_t j = galois_ntt_source(slot, k, n, ix.neg) & (ix.C - 1u);
                    T x0, x1;
                    hoist_term<T>(tile, j, ha.key[g] + limb + to + l, D, logc, ix.key_comp, fold, pv, x0, x1);
                    t0.mac(x0, T(1));
                    t1.mac(x1, T(1));
                }
                __syncthreads(); // the next giant step loads another source chunk over this one
            }
            if (owner)
            {
                const unsigned long long at = ix.in_stack + to + l;
                for (int g = ha.count; g < n2; g++)
                {
                    t0.mac(v[static_cast<unsigned long long>(g) * group + at], T(1));
                    t1.mac(v1[static_cast<unsigned long long>(g) * group + at], T(1));
                }
                acc[at] = fold.reduce(fold.sum(t0)); // acc: [2][count][M][N]
                acc[group + at] = fold.reduce(fold.sum(t1));
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

        template <typename T>
        void bsgs_scale_launch(const T* c0, const T* c1, T* u, const T* consts, const kern::HoistArgs<T>& args, int first,
                               int n1, int count, int L, int M, int n_power, hipStream_t stream)
        {
            const unsigned nt = kern::HOIST_NT;
            const unsigned long long tiles = ((1ull << n_power) + nt - 1) / nt;
            const unsigned long long blocks = tiles * 2ull * static_cast<unsigned>(count);
            if (blocks * nt > 0xFFFFFFFFull) // HIP caps a launch at 2^32 - 1 work-items per dimension
                throw std::invalid_argument("Invalid count!");
            GPUNTT_LAUNCH((kern::bsgs_scale_input<T>), dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(M)),
                          dim3(nt), 0, stream, c0, c1, u, consts, args, first, n1, count, L, M, n_power);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        void bsgs_sum_shape(size_t word_bytes, int n1, int n_power, bool aligned, int& V, unsigned& nt)
        {
            const unsigned long long N = 1ull << n_power;
            V = static_cast<int>(16 / word_bytes);
            // one word per lane when a weight is off 16 bytes, when the ring is shorter than a group, and when 64 lanes of
            // n1 groups pass the LDS budget (n1 = 64 at either width)
            if (!aligned || N % static_cast<unsigned>(V) != 0 ||
                static_cast<size_t>(n1) * 64 * 16 > kern::HOIST_LDS)
                V = 1;
            nt = kern::HOIST_NT;
            while (nt > 64 && (static_cast<size_t>(n1) * nt * V * word_bytes > kern::HOIST_LDS ||
                               static_cast<unsigned long long>(nt / 2) * V >= N))
                nt /= 2;
        }

        template <typename T>
        void bsgs_sum_launch(const T* u, T* v, const T* consts, const kern::BsgsWeights<T>& weights, int count, int M,
                             int n_power, hipStream_t stream)
        {
            uintptr_t low = reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v);
            for (int i = 0; i < weights.n1 * weights.n2; i++)
                low |= reinterpret_cast<uintptr_t>(weights.w[i]);
            int V;
            unsigned nt;
            bsgs_sum_shape(sizeof(T), weights.n1, n_power, (low & 15u) == 0, V, nt);
            const unsigned long long per = static_cast<unsigned long long>(nt) * V;
            const unsigned long long tiles = ((1ull << n_power) + per - 1) / per;
            const unsigned long long blocks = tiles * 2ull * static_cast<unsigned>(count);
            if (blocks * nt > 0xFFFFFFFFull)
                throw std::invalid_argument("Invalid count!");
            const size_t lds = static_cast<size_t>(weights.n1) * nt * V * sizeof(T);
            const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(M));
            if (V > 1)
                GPUNTT_LAUNCH((kern::bsgs_weighted_sum<T, 16 / sizeof(T)>), grid, dim3(nt), lds, stream, u, v, consts,
                              weights, count, M, n_power);
            else
                GPUNTT_LAUNCH((kern::bsgs_weighted_sum<T, 1>), grid, dim3(nt), lds, stream, u, v, consts, weights, count,
                              M, n_power);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        template <typename T>
        void bsgs_giant_launch(const T* a, const T* v, T* acc, const T* consts, const kern::HoistArgs<T>& args, int n2,
                               int D, int count, int M, int KM, int n_power, bool negacyclic, hipStream_t stream)
        {
            hoist_dispatch<T>(a, v, D, count, M, n_power, HOIST_SUM_LOG_MAX,
                              [&](dim3 grid, dim3 block, size_t lds, int logc, bool wide) {
                                  if (wide)
                                      GPUNTT_LAUNCH((kern::inner_product_galois_giant<T, true>), grid, block, lds, stream,
                                                    a, v, acc, consts, args, n2, D, count, M, KM, n_power, logc,
                                                    negacyclic ? 1 : 0);
                                  else
                                      GPUNTT_LAUNCH((kern::inner_product_galois_giant<T, false>), grid, block, lds, stream,
                                                    a, v, acc, consts, args, n2, D, count, M, KM, n_power, logc,
                                                    negacyclic ? 1 : 0);
                              });
        }

        template void bsgs_scale_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                                const kern::HoistArgs<Data32>&, int, int, int, int, int, int, hipStream_t);
        template void bsgs_scale_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                                const kern::HoistArgs<Data64>&, int, int, int, int, int, int, hipStream_t);
        template void bsgs_sum_launch<Data32>(const Data32*, Data32*, const Data32*, const kern::BsgsWeights<Data32>&, int,
                                              int, int, hipStream_t);
        template void bsgs_sum_launch<Data64>(const Data64*, Data64*, const Data64*, const kern::BsgsWeights<Data64>&, int,
                                              int, int, hipStream_t);
        template void bsgs_giant_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                                const kern::HoistArgs<Data32>&, int, int, int, int, int, int, bool,
                                                hipStream_t);
        template void bsgs_giant_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                                const kern::HoistArgs<Data64>&, int, int, int, int, int, int, bool,
                                                hipStream_t);

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
