// key_switch.hip -- hybrid key switching (extension, include/gpuntt/rns/key_switch.cuh).
//
// ks_mod_up: ModUp of ALL digits from one read of the input.  One lane owns one coefficient column of one input: it
// reads its L words once (coalesced: consecutive lanes, consecutive columns) and parks two words per limb in LDS, at
// [i][lane] -- y_i, one exact Shoup product with the constants of the limb's OWN digit, and the canonical word, one Shoup
// product against the companion of 1 (a conditional subtraction does not reduce a 64-bit word modulo a 20-bit q).  A lane
// only reads back what it wrote: no barrier.  The outputs are then walked as (digit d, block of BC_KB moduli) pairs: a
// block inside S_d is BC_KB stores of parked words; any other block goes through the conversion unit of
// base_conversion_internal.hpp over i in S_d only (bc_z, bc_block_mac, bc_fold: the bounds are proved there; alpha may
// exceed a chunk of the multiply-accumulate), with the parked word stored instead for the moduli of the block that do lie
// in S_d (their matrix column is zero).  The live state is BC_KB accumulators whatever L, M and D are.  The centred mode's
// v_d is recomputed only when the walk enters another digit: once per digit and workgroup.  Stores (D M words per column)
// dominate loads (L words) and carry no lane condition.  Every constant is indexed by wave-uniform values and comes
// through the constant address space, hence the scalar cache.
//
// Small count * N: blockIdx.y splits the (d, block) pairs of a column tile over several workgroups, each of which
// re-reads the tile's input (from L2) and recomputes the parked words -- host::rns_split(), as for base_convert.
//
// mod_down: kern::base_convert<T, centred, divide, STRIDED> of base_conversion_internal.hpp -- the shared kernel, the same
// constants image (bc_image) -- with the stack strides of the full base: the special limbs and the q-limbs are read where
// the inner product left them, inside the M-limb stacks.  The strides are a compile-time form of the kernel, so the dense
// instantiations behind BaseConvPlan keep their registers.
//
// Every switch ends in Impl::finish: the plan's own full-base INTT, mod_down and the optional q-base NTT.
//
// rotate_hoisted: inner_product_galois of hoisted_rotation.hip (the inner product that permutes while it multiplies, all
// G elements in one launch), then finish over G * 2 * count stacks.
//
// rotate_hoisted_sum: inner_product_galois_sum of hoisted_rotation.hip (the same inner product, weighted and summed over
// the G elements in the extended base), then finish over 2 * count stacks whatever G is.  The two share
// Impl::hoist_prepare: every refusal of the call and the kernel arguments.
//
// linear_transform_bsgs: the double-hoisted baby-step/giant-step transform.  Impl::bsgs_axis sorts each
// axis (the steps with a key first) and refuses what the header lists; then inner_product_galois over the keyed baby
// steps and bsgs_scale_input over the others, bsgs_weighted_sum, the plan's own INTT, mod_down, mod_up and NTT over the
// second components of all keyed giant steps at once, inner_product_galois_giant (all of hoisted_rotation.hip) and finish
// over 2 * count stacks.
//
// multiply_relinearize: tensor_top of relinearize.hip (x1 y1 into the scratch), the plan's own decompose steps on it,
// inner_product_tensor (the inner product seeded with P (x0 y0) and P (x0 y1 + x1 y0)), then finish over 2 * count stacks
// (DESIGN.md 3.15).
//
// multiply_relinearize_sum: the same sequence with tensor_top_sum and inner_product_tensor_sum of relinearize_sum.hip,
// which loop over the terms: one key switch and one ModDown for sum_t x_t y_t.
//
// relinearize: the key switch of a three-component ciphertext whose components exist already.  In NTT
// form decompose, inner_product_seeded of relinearize.hip (the inner product seeded with P c01) and finish; in coefficient
// form mod_up, the transforms and the plain inner product, then mod_down_add -- mod_down's kernel with an addend epilogue
// (base_conversion_internal.hpp) -- so c01 is never transformed on its own.
//
// Key material.  lift_small, generate_keys and encrypt_symmetric make what every call above reads:
// lift_small of keygen.hip takes signed errors into the base, the plan's forward transform follows, and keygen_combine
// (one launch over all keys and digits) forms E - a s + P g_d s_from with the exact accumulator.  encrypt_symmetric is the
// same kernel over the q-base with the message in the gadget term's place.
//
// Rescaling (a plan built with rescale_limbs = R > 0).  mod_down_rescale is mod_down's launch with a second
// constants image, {q_{L-R} .. q_{L-1}, p_0 .. p_{K-1}} -> {q_0 .. q_{L-R-1}}: the R dropped q-limbs and the K special
// limbs are one contiguous run of the full-base stack, (L - R) N words behind its start, so the strided kernel reads them
// in place and divides by P q_{L-R} ... q_{L-1} with ONE rounding.  Impl::finish takes a flag and ends the three
// *_rescale pipeline calls with it.  rescale divides a q-base stack by the dropped primes alone (a third image): in
// coefficient form the same single launch; in NTT form rescale_gather, the inverse transform of the R dropped limbs only,
// the dense centred conversion, the forward transform over the kept moduli and rescale_sub_scale (rescale.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

#include "base_conversion_internal.hpp"
#include "decrypt_internal.hpp"
#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/key_switch.cuh"
#include "hoisted_rotation_internal.hpp"
#include "keygen_internal.hpp"
#include "launch.hpp"
#include "relinearize_internal.hpp"
#include "relinearize_sum_internal.hpp"
#include "rescale_internal.hpp"
#include "rns_call.hpp"

namespace gpuntt
{
    namespace kern
    {
        constexpr int KS_NT = 128;    // lanes per workgroup at most; 64 when two words per limb and lane pass 64 KiB of LDS
        constexpr size_t KS_LDS = 65536;

        // RnsWide, rns_shoup: rns_arith.hpp; BC_KB, bc_z, bc_block_mac, bc_fold: base_conversion_internal.hpp

        // where the ModUp constants lie in the workspace, in words; MP = M rounded up to BC_KB (padding: zero)
        struct KsOffsets
        {
            unsigned q;      // [L]
            unsigned w;      // [L] (Q_d(i) / q_i)^-1 mod q_i
            unsigned wp;     // [L] its Shoup companion
            unsigned recip;  // [L] R_i (0: q_i is a power of two)
            unsigned shift;  // [L] b_i - 1
            unsigned matrix; // [L][MP] (Q_d(i) / q_i) mod modulus m, 0 for m in S_d(i)
            unsigned mod;    // [MP] the full base
            unsigned t1;     // [MP] 2^W mod modulus m
            unsigned t1p;
            unsigned t2;     // [MP] 2^2W mod modulus m
            unsigned t2p;
            unsigned onep;   // [MP] floor(2^W / modulus m): the Shoup companion of 1
            unsigned negq;   // [D][MP] (-Q_d) mod modulus m
        };
        template <typename T> struct KsConsts : BcFoldConsts<T>
        {
            using CP = BcCP<T>;
            CP q, w, wp, recip, shift, matrix, mod, negq;
            __device__ KsConsts(const T* workspace, const KsOffsets& o)
            {
                const CP base = (CP) (workspace);
                q = base + o.q, w = base + o.w, wp = base + o.wp, recip = base + o.recip, shift = base + o.shift;
                matrix = base + o.matrix, mod = base + o.mod, this->t1 = base + o.t1, this->t1p = base + o.t1p;
                this->t2 = base + o.t2, this->t2p = base + o.t2p, this->onep = base + o.onep, negq = base + o.negq;
            }
        };

        // in: T[count][L][N]; a: T[D][count][M][N], digit_stride = count M N words; total = count N columns
        template <typename T, bool CENTRED>
        __global__ __launch_bounds__(KS_NT) void ks_mod_up(const T* __restrict__ in, T* __restrict__ a,
                                                           const T* __restrict__ consts, KsOffsets off, int L, int M,
                                                           int MP, int alpha, int D, int n_power,
                                                           unsigned long long total, unsigned long long digit_stride)
        {
            const KsConsts<T> k(consts, off);
            using W2 = typename RnsWide<T>::type;
            constexpr int W = static_cast<int>(8 * sizeof(T));
            extern __shared__ __align__(16) unsigned char ks_smem[];
            const int nt = static_cast<int>(blockDim.x);
            T* ys = reinterpret_cast<T*>(ks_smem) + threadIdx.x; // y_i at ys[i * nt]
            T* cs = ys + L * nt;                                  // in[i] mod q_i at cs[i * nt]

            const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * nt + threadIdx.x;
            if (t >= total)
                return; // (no barrier below)
            const unsigned long long e = t >> n_power, col = t & ((1ull << n_power) - 1ull);
            const T* src = in + ((e * static_cast<unsigned>(L)) << n_power) + col;
#pragma unroll 4
            for (int i = 0; i < L; i++)
            {
                const T q = k.q[i];
                const T x = src[static_cast<unsigned long long>(i) << n_power];
                ys[i * nt] = rns_shoup<T>(x, k.w[i], k.wp[i], q);
                cs[i * nt] = rns_shoup<T>(x, T(1), k.onep[i], q);
            }

            const unsigned long long abase = ((e * static_cast<unsigned>(M)) << n_power) + col;
            const int jblocks = MP / BC_KB, pairs = D * jblocks;
            int v_digit = -1;
            T v = 0;
            for (int pi = static_cast<int>(blockIdx.y); pi < pairs; pi += static_cast<int>(gridDim.y))
            {
                const int d = pi / jblocks, j0 = (pi - d * jblocks) * BC_KB;
                const int lo = d * alpha, hi = ip_min(lo + alpha, L); // S_d
                T* dst = a + static_cast<unsigned long long>(d) * digit_stride + abase;
                if (j0 >= lo && j0 + BC_KB <= hi)
                {
#pragma unroll
                    for (int b = 0; b < BC_KB; b++)
                        dst[static_cast<unsigned long long>(j0 + b) << n_power] = cs[(j0 + b) * nt];
                    continue;
                }
                if constexpr (CENTRED)
                {
                    if (d != v_digit) // pi only grows: once per digit
                    {
                        W2 zsum = static_cast<W2>(1) << (W - 1);
                        for (int i = lo; i < hi; i++)
                            zsum += bc_z<T>(ys[i * nt], k.recip[i], k.shift[i]);
                        v = static_cast<T>(zsum >> W);
                        v_digit = d;
                    }
                }
                W2 acc[BC_KB];
                T carry[BC_KB];
                bc_block_mac<T, CENTRED>(ys + lo * nt, nt, k.matrix + lo * MP + j0, MP, hi - lo, v,
                                         k.negq + d * MP + j0, acc, carry);
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    const int m = j0 + b;
                    if (m < M)
                    {
                        T r;
                        if (m >= lo && m < hi)
                            r = cs[m * nt];
                        else
                            r = bc_fold<T>(acc[b], carry[b], k, m, k.mod[m]);
                        dst[static_cast<unsigned long long>(m) << n_power] = r;
                    }
                }
            }
        }

    } // namespace kern

    namespace host
    {
        namespace
        {
            std::atomic<int> g_ks_split{0}; // test hook keyswitch_split: 0 = rns_split(), n = n workgroups per column tile
        }
        void keyswitch_set_split(int v) { g_ks_split.store(v, std::memory_order_relaxed); }
    } // namespace host

    namespace
    {
        using U128 = unsigned __int128;

        // rns_host.hpp, rns_call.hpp and, for bc_padded, base_conversion_internal.hpp
        using host::bc_padded;
        using host::column_tiles;
        using host::need_aligned_scratch;
        using host::need_int_batch;
        using host::need_pointers;
        using host::refuse_overlap;
        using host::rns_align;
        using host::rns_check_n_power;
        using host::rns_overlap;
        using host::words_at;

        // everything the host derives for one (q-base, special base, alpha), in exact integers
        struct KsHost
        {
            int L = 0, K = 0, M = 0, alpha = 0, D = 0;
            std::vector<std::uint64_t> mod;                                // [M] the full base
            std::vector<host::BcHostConsts> up;                            // [D] {q_i : i in S_d} -> the complement
            host::BcHostConsts down;                                       // {p_k} -> {q_j}
            std::vector<std::uint64_t> t1, t1p, t2, t2p, onep;             // [M]
            int lo(int d) const { return d * alpha; }
            int hi(int d) const { return std::min((d + 1) * alpha, L); }
        };

        void ks_check_counts(int L, int K, int alpha)
        {
            if (L < 1 || L > INNERPROD_MAX_MODULI)
                throw std::invalid_argument("Invalid q_count!");
            if (K < 1 || K > INNERPROD_MAX_MODULI || L + K > INNERPROD_MAX_MODULI)
                throw std::invalid_argument("Invalid p_count!");
            if (alpha < 1)
                throw std::invalid_argument("Invalid alpha!");
        }
        int ks_digits(int L, int alpha) { return static_cast<int>((static_cast<long long>(L) + alpha - 1) / alpha); }

        template <typename T>
        KsHost ks_derive(const Modulus<T>* qm, int L, const Modulus<T>* pm, int K, int alpha, bool digits = true)
        {
            constexpr int W = static_cast<int>(8 * sizeof(T));
            ks_check_counts(L, K, alpha);
            if (qm == nullptr || pm == nullptr)
                throw std::invalid_argument("null pointer argument");
            KsHost h;
            h.L = L, h.K = K, h.M = L + K, h.alpha = alpha > L ? L : alpha, h.D = ks_digits(L, h.alpha);
            std::vector<Modulus<T>> full(qm, qm + L);
            full.insert(full.end(), pm, pm + K);
            for (const Modulus<T>& m : full)
                h.mod.push_back(host::bc_checked_value<T>(m));
            // {p} -> {q} checks p pairwise and every p against every q; the q among themselves here (the digits would
            // find the same pairs, but reference_mod_down derives none)
            h.down = host::bc_derive<T>(pm, K, qm, L);
            for (int i = 0; i < L; i++)
                for (int o = i + 1; o < L; o++)
                    if (std::__gcd(h.mod[i], h.mod[o]) != 1)
                        throw std::invalid_argument("Input base moduli are not pairwise coprime!");
            for (int d = 0; digits && d < h.D; d++)
            {
                std::vector<Modulus<T>> rest(full.begin(), full.begin() + h.lo(d));
                rest.insert(rest.end(), full.begin() + h.hi(d), full.end());
                h.up.push_back(host::bc_derive<T>(qm + h.lo(d), h.hi(d) - h.lo(d), rest.data(),
                                                  static_cast<int>(rest.size())));
            }
            for (int m = 0; m < h.M; m++)
            {
                const host::RnsFoldConsts f = host::rns_fold_consts(h.mod[m], W);
                h.t1.push_back(f.t1), h.t1p.push_back(f.t1p), h.t2.push_back(f.t2), h.t2p.push_back(f.t2p);
                h.onep.push_back(f.onep);
            }
            return h;
        }

        // column of modulus m in the output base of digit d (the complement of S_d in full-base order); m not in S_d
        int ks_column(const KsHost& h, int d, int m) { return m < h.lo(d) ? m : m - (h.hi(d) - h.lo(d)); }

        size_t ks_up_words(int L, int M, int D)
        {
            const size_t MP = static_cast<size_t>(bc_padded(M));
            return 5 * static_cast<size_t>(L) + static_cast<size_t>(L) * MP + 6 * MP + static_cast<size_t>(D) * MP;
        }

        template <typename T> std::vector<T> ks_up_image(const KsHost& h, kern::KsOffsets& off)
        {
            const int L = h.L, M = h.M, D = h.D, MP = bc_padded(M);
            std::vector<T> img(ks_up_words(L, M, D), T(0));
            size_t at = 0;
            auto take = [&](size_t words) {
                const size_t first = at;
                at += words;
                return first;
            };
            const size_t o_q = take(L), o_w = take(L), o_wp = take(L), o_r = take(L), o_sh = take(L),
                         o_m = take(static_cast<size_t>(L) * MP), o_mod = take(MP), o_t1 = take(MP), o_t1p = take(MP),
                         o_t2 = take(MP), o_t2p = take(MP), o_one = take(MP), o_nq = take(static_cast<size_t>(D) * MP);
            for (int d = 0; d < D; d++)
            {
                const host::BcHostConsts& u = h.up[d];
                for (int i = h.lo(d); i < h.hi(d); i++)
                {
                    const int li = i - h.lo(d);
                    img[o_q + i] = static_cast<T>(u.q[li]), img[o_w + i] = static_cast<T>(u.w[li]);
                    img[o_wp + i] = static_cast<T>(u.wp[li]), img[o_r + i] = static_cast<T>(u.recip[li]);
                    img[o_sh + i] = static_cast<T>(u.blen[li] - 1);
                    for (int m = 0; m < M; m++)
                        if (m < h.lo(d) || m >= h.hi(d))
                            img[o_m + static_cast<size_t>(i) * MP + m] =
                                static_cast<T>(u.matrix[static_cast<size_t>(li) * u.K + ks_column(h, d, m)]);
                }
                for (int m = 0; m < M; m++)
                    if (m < h.lo(d) || m >= h.hi(d))
                        img[o_nq + static_cast<size_t>(d) * MP + m] = static_cast<T>(u.negq[ks_column(h, d, m)]);
            }
            for (int m = 0; m < M; m++)
            {
                img[o_mod + m] = static_cast<T>(h.mod[m]), img[o_t1 + m] = static_cast<T>(h.t1[m]);
                img[o_t1p + m] = static_cast<T>(h.t1p[m]), img[o_t2 + m] = static_cast<T>(h.t2[m]);
                img[o_t2p + m] = static_cast<T>(h.t2p[m]), img[o_one + m] = static_cast<T>(h.onep[m]);
            }
            auto u32 = [](size_t v) { return static_cast<unsigned>(v); };
            off = kern::KsOffsets{u32(o_q),  u32(o_w),   u32(o_wp), u32(o_r),   u32(o_sh),  u32(o_m), u32(o_mod),
                                  u32(o_t1), u32(o_t1p), u32(o_t2), u32(o_t2p), u32(o_one), u32(o_nq)};
            return img;
        }

        // the argument checks of mod_up / mod_down (device or host arrays alike)
        template <typename T>
        void ks_check_mod_up(int L, int M, int D, const T* in, const T* a, int n_power, int count, BaseConvMode mode)
        {
            rns_check_n_power(n_power);
            if (mode != BaseConvMode::approximate && mode != BaseConvMode::centred)
                throw std::invalid_argument("Invalid mode!");
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (in == nullptr || a == nullptr)
                throw std::invalid_argument("null pointer argument");
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n_power;
            if (rns_overlap(in, cols * L * sizeof(T), a, cols * M * D * sizeof(T)) && count > 0)
                throw std::invalid_argument("ModUp input and output overlap!");
        }
        template <typename T>
        void ks_check_mod_down(int L, int M, const T* x, const T* out, int n_power, int stacks) // L out of M limbs
        {
            rns_check_n_power(n_power);
            if (stacks < 0)
                throw std::invalid_argument("Invalid stacks!");
            if (x == nullptr || out == nullptr)
                throw std::invalid_argument("null pointer argument");
            const std::uint64_t cols = static_cast<std::uint64_t>(stacks) << n_power;
            if (rns_overlap(x, cols * M * sizeof(T), out, cols * L * sizeof(T)) && stacks > 0)
                throw std::invalid_argument("ModDown input and output overlap!");
        }

        struct KsLayout // the workspace, in bytes
        {
            size_t up, down, inner, ntt_full_f, ntt_full_i, ntt_q_i, ntt_q_f;
            size_t down_rs, rs, ntt_keep_f, ntt_drop_i; // R > 0 only: they follow the rest, so R = 0 is the old layout
            size_t total;
        };
        void ks_check_rescale_limbs(int L, int R, int least)
        {
            if (R < least || R > L - 1)
                throw std::invalid_argument("Invalid rescale_limbs!");
        }
        template <typename T> KsLayout ks_layout(int L, int K, int alpha, int n_power, int R)
        {
            ks_check_counts(L, K, alpha);
            rns_check_n_power(n_power);
            ks_check_rescale_limbs(L, R, 0);
            const int M = L + K, D = ks_digits(L, alpha > L ? L : alpha);
            KsLayout w{};
            size_t at = 0;
            auto take = [&](size_t bytes) {
                const size_t first = at;
                at += rns_align(bytes);
                return first;
            };
            w.up = take(ks_up_words(L, M, D) * sizeof(T));
            w.down = take(host::bc_image_words(K, L) * sizeof(T));
            w.inner = take(InnerProductPlan<T>::workspace_bytes(M));
            w.ntt_full_f = take(NTTPlan<T>::workspace_bytes(n_power, M));
            w.ntt_full_i = take(NTTPlan<T>::workspace_bytes(n_power, M));
            w.ntt_q_i = take(NTTPlan<T>::workspace_bytes(n_power, L));
            w.ntt_q_f = take(NTTPlan<T>::workspace_bytes(n_power, L));
            if (R > 0)
            {
                w.down_rs = take(host::bc_image_words(K + R, L - R) * sizeof(T));
                w.rs = take(host::bc_image_words(R, L - R) * sizeof(T));
                w.ntt_keep_f = take(NTTPlan<T>::workspace_bytes(n_power, L - R));
                w.ntt_drop_i = take(NTTPlan<T>::workspace_bytes(n_power, R));
            }
            w.total = at;
            return w;
        }

        struct KsScratch // the caller's scratch, in bytes
        {
            size_t a, c_coeff, inner_out, total; // c_coeff does not move with `components`: decompose needs no C
        };
        template <typename T> KsScratch ks_scratch(int L, int M, int D, int n_power, int count, int components)
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (components < 1 || components > INNERPROD_MAX_COMPONENTS)
                throw std::invalid_argument("Invalid components!");
            const size_t poly = (static_cast<size_t>(count) << n_power) * sizeof(T);
            KsScratch s{};
            s.a = 0;
            s.c_coeff = s.a + rns_align(poly * M * D);
            s.inner_out = s.c_coeff + rns_align(poly * L);
            s.total = s.inner_out + rns_align(poly * M * components);
            return s;
        }

        // the scratch of rotate_hoisted, in bytes: the accumulators T[G][2][count][M][N]
        template <typename T> size_t ks_hoisted_scratch(int M, int n_power, int count, int elements)
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (elements < 1 || elements > GALOIS_MAX_COUNT)
                throw std::invalid_argument("Invalid galois_count!");
            return rns_align((static_cast<size_t>(count) << n_power) * sizeof(T) * M * 2 * elements);
        }

        // the scratch of rotate_hoisted_sum, in bytes: the accumulators T[2][count][M][N], whatever G is
        template <typename T> size_t ks_hoisted_sum_scratch(int M, int n_power, int count)
        {
            return ks_hoisted_scratch<T>(M, n_power, count, 1);
        }

        // the scratch of linear_transform_bsgs, in bytes.  u: T[n1][2][count][M][N], the baby accumulators -- dead after
        // bsgs_weighted_sum, so acc T[2][count][M][N] lives at its start; v: T[2][n2][count][M][N], the weighted sums,
        // component-major with the keyed giant steps first; t: T[n2 * count][L][N], the second components after mod_down;
        // a2: T[D][n2 * count][M][N], their digits.  t and a2 are sized for n2 keyed giant steps
        struct KsBsgsScratch
        {
            size_t u, v, t, a2, total;
        };
        template <typename T> KsBsgsScratch ks_bsgs_scratch(int L, int M, int D, int n_power, int count, int n1, int n2)
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (n1 < 1 || n1 > KEYSWITCH_MAX_STEPS || n2 < 1 || n2 > KEYSWITCH_MAX_STEPS ||
                n1 * n2 > KEYSWITCH_MAX_DIAGONALS)
                throw std::invalid_argument("Invalid baby or giant step count!");
            const size_t poly = (static_cast<size_t>(count) << n_power) * sizeof(T);
            KsBsgsScratch s{};
            s.u = 0;
            s.v = s.u + rns_align(poly * M * 2 * n1);
            s.t = s.v + rns_align(poly * M * 2 * n2);
            s.a2 = s.t + rns_align(poly * L * n2);
            s.total = s.a2 + rns_align(poly * M * D * n2);
            return s;
        }
    } // namespace

    template <typename T> struct KeySwitchPlan<T>::Impl
    {
        int L = 0, K = 0, M = 0, alpha = 0, D = 0, n = 0, KM = 0;
        bool negacyclic = true;
        std::vector<Modulus<T>> moduli; // [M] the full base as the caller gave it: modulus(m)
        std::vector<int> limbs;
        std::vector<T> p_mod_q, p_mod_q_shoup; // [L] P mod q_j and its Shoup companion: the c0 term of rotate_hoisted
        char* ws = nullptr;
        bool owns = false;
        KsLayout lay{};
        kern::KsOffsets up_off{};
        kern::BcOffsets down_off{};
        std::unique_ptr<InnerProductPlan<T>> inner;
        std::unique_ptr<NTTPlan<T>> ntt_full_f, ntt_full_i, ntt_q_i, ntt_q_f;
        // rescaling, R > 0 only: Lk = L - R kept limbs; the images {dropped q, p} -> {kept q} and {dropped q} -> {kept q};
        // the forward transform over the kept moduli and the inverse transform over the dropped ones
        int R = 0, Lk = 0;
        kern::BcOffsets down_rs_off{}, rs_off{};
        kern::RsDropped<T> dropped_mods{}; // the dropped moduli and their companions of 1: rescale_gather reduces with them
        std::unique_ptr<NTTPlan<T>> ntt_keep_f, ntt_drop_i;

        void mod_up(const T* in, T* a, int count, BaseConvMode mode, hipStream_t stream) const
        {
            ks_check_mod_up<T>(L, M, D, in, a, n, count, mode);
            if (count == 0)
                return;
            const unsigned long long total = static_cast<unsigned long long>(count) << n;
            unsigned nt = kern::KS_NT;
            while (nt > 64 && 2 * static_cast<size_t>(L) * nt * sizeof(T) > kern::KS_LDS)
                nt /= 2;
            const unsigned long long tiles = column_tiles(total, nt, "Invalid count!");
            const int MP = bc_padded(M), pairs = D * (MP / kern::BC_KB);
            // workgroups per column tile over the (digit, block) pairs: DESIGN.md 3.12
            const int split = host::rns_split(tiles, pairs, host::g_ks_split.load(std::memory_order_relaxed));
            const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(split));
            const size_t lds = 2 * static_cast<size_t>(L) * nt * sizeof(T);
            const T* consts = reinterpret_cast<const T*>(ws + lay.up);
            const unsigned long long digit_stride = total * static_cast<unsigned>(M);
            if (mode == BaseConvMode::centred)
                GPUNTT_LAUNCH((kern::ks_mod_up<T, true>), grid, dim3(nt), lds, stream, in, a, consts, up_off, L, M, MP,
                              alpha, D, n, total, digit_stride);
            else
                GPUNTT_LAUNCH((kern::ks_mod_up<T, false>), grid, dim3(nt), lds, stream, in, a, consts, up_off, L, M, MP,
                              alpha, D, n, total, digit_stride);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        void mod_down(const T* x, T* out, int stacks, hipStream_t stream) const
        {
            ks_check_mod_down<T>(L, M, x, out, n, stacks);
            if (stacks == 0)
                return;
            // the input base is {p_k} (K limbs, parked in LDS), the output base {q_j} (L limbs)
            divide_in_stack(x, out, stacks, M, K, L, lay.down, down_off, stream);
        }

        // ONE launch of the strided base_convert (centred, divide): stacks of `limbs` limbs at x, the last `in_count` of the
        // first out_count + in_count are the input base, read in place, the first out_count are c; out is dense,
        // T[stacks][out_count][N].  The constants image lies `image` bytes into the workspace
        // addend != nullptr (dense like out): ONE launch of mod_down_add instead, the same kernel with the addend epilogue
        void divide_in_stack(const T* x, T* out, int stacks, int limbs, int in_count, int out_count, size_t image,
                             const kern::BcOffsets& off, hipStream_t stream, const T* addend = nullptr) const
        {
            const unsigned long long poly = 1ull << n, full = static_cast<unsigned long long>(limbs) << n;
            const unsigned long long total = static_cast<unsigned long long>(stacks) << n;
            const unsigned long long tiles = column_tiles(total, kern::BC_NT, "Invalid stacks!");
            const int KP = bc_padded(out_count);
            const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(host::bc_ksplit(tiles, out_count)));
            const size_t lds = static_cast<size_t>(in_count) * kern::BC_NT * sizeof(T);
            const kern::BcStrides<true> strides{full, full, static_cast<unsigned long long>(out_count) << n};
            if (addend != nullptr)
                GPUNTT_LAUNCH((kern::mod_down_add<T>), grid, dim3(kern::BC_NT), lds, stream, x + out_count * poly, x, addend,
                              out, reinterpret_cast<const T*>(ws + image), off, in_count, out_count, KP, n, total, strides);
            else
                GPUNTT_LAUNCH((kern::base_convert<T, true, true, true>), grid, dim3(kern::BC_NT), lds, stream,
                              x + out_count * poly, x, out, reinterpret_cast<const T*>(ws + image), off, in_count,
                              out_count, KP, n, total, strides);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        // x: T[stacks][M][N], addend and out: T[stacks][L][N]; addend may be exactly out
        void mod_down_add(const T* x, const T* addend, T* out, int stacks, hipStream_t stream) const
        {
            ks_check_mod_down<T>(L, M, x, out, n, stacks);
            need_pointers(addend);
            if (stacks == 0)
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(stacks) << n;
            const std::uint64_t low_bytes = cols * L * sizeof(T);
            refuse_overlap({{addend, low_bytes}}, {{x, cols * M * sizeof(T)}, {out, low_bytes, true}},
                           "The addend overlaps an operand!");
            divide_in_stack(x, out, stacks, M, K, L, lay.down, down_off, stream, addend);
        }

        void need_rescale() const
        {
            if (R == 0)
                throw std::invalid_argument("The plan was built without rescale_limbs!");
        }

        // x: T[stacks][M][N], out: T[stacks][Lk][N]: the R dropped q-limbs and the K special limbs are the input base
        void mod_down_rescale(const T* x, T* out, int stacks, hipStream_t stream) const
        {
            need_rescale();
            ks_check_mod_down<T>(Lk, M, x, out, n, stacks);
            if (stacks == 0)
                return;
            divide_in_stack(x, out, stacks, M, K + R, Lk, lay.down_rs, down_rs_off, stream);
        }

        size_t rescale_scratch(int stacks) const
        {
            need_rescale();
            if (stacks < 0)
                throw std::invalid_argument("Invalid stacks!");
            return rns_align((static_cast<size_t>(stacks) << n) * R * sizeof(T));
        }

        // x: T[stacks][L][N], out: T[stacks][Lk][N]; the scratch (ntt_form only): T[stacks][R][N]
        void rescale(const T* x, T* out, int stacks, bool ntt_form, void* scratch, hipStream_t stream) const
        {
            need_rescale();
            if (ntt_form)
                need_transforms();
            ks_check_mod_down<T>(Lk, L, x, out, n, stacks);
            if (!ntt_form)
            {
                if (stacks > 0)
                    divide_in_stack(x, out, stacks, L, R, Lk, lay.rs, rs_off, stream);
                return;
            }
            const size_t scratch_bytes = rescale_scratch(stacks);
            need_pointers(scratch);
            need_aligned_scratch(scratch);
            if (stacks == 0)
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(stacks) << n;
            refuse_overlap({{scratch, scratch_bytes}}, {{x, cols * L * sizeof(T)}}, "The scratch overlaps an operand!");
            refuse_overlap({{scratch, scratch_bytes}}, {{out, cols * Lk * sizeof(T)}}, "The scratch overlaps out!");
            // every limit before the first launch: the batches of the transforms are ints, the grids as their launches check
            need_int_batch(static_cast<unsigned long long>(stacks) * static_cast<unsigned>(L), "Invalid stacks!");
            const unsigned long long tiles = column_tiles(cols, kern::BC_NT, "Invalid stacks!");
            T* dropped = static_cast<T*>(scratch);
            const T* image = reinterpret_cast<const T*>(ws + lay.rs);
            const kern::RsOffsets sub{rs_off.p, rs_off.onep, rs_off.qinv, rs_off.qinvp};
            host::rescale_gather_launch<T>(x, dropped, dropped_mods, stacks, L, R, n, false, stream);
            host::rescale_sub_scale_launch<T>(x, out, image, sub, stacks, L, Lk, n, false, stream);

            host::rescale_gather_launch<T>(x, dropped, dropped_mods, stacks, L, R, n, true, stream);
            ntt_drop_i->execute(dropped, dropped, stacks * R, stream);
            // the dense centred conversion {dropped q} -> {kept q}, no division: conv_j in coefficient form
            const int KP = bc_padded(Lk);
            const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(host::bc_ksplit(tiles, Lk)));
            GPUNTT_LAUNCH((kern::base_convert<T, true, false, false>), grid, dim3(kern::BC_NT),
                          static_cast<size_t>(R) * kern::BC_NT * sizeof(T), stream, dropped, out, out, image, rs_off, R, Lk,
                          KP, n, cols, kern::BcStrides<false>{});
            GPUNTT_HIP_CHECK(hipGetLastError());
            ntt_keep_f->execute(out, out, stacks * Lk, stream);
            host::rescale_sub_scale_launch<T>(x, out, image, sub, stacks, L, Lk, n, true, stream);
        }

        void need_transforms() const
        {
            if (!ntt_full_f)
                throw std::invalid_argument("The plan was built without transform tables!");
        }

        void decompose(const T* c_in, T* a, int count, bool input_ntt, void* scratch, hipStream_t stream) const
        {
            need_transforms();
            const KsScratch s = ks_scratch<T>(L, M, D, n, count, 1);
            need_pointers(c_in, a);
            if (input_ntt)
                need_pointers(scratch);
            if (count == 0)
                return;
            const T* coeff = c_in;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t c_bytes = cols * L * sizeof(T), a_bytes = cols * M * D * sizeof(T);
            // every refusal comes before the first launch
            refuse_overlap({{a, a_bytes}}, {{c_in, c_bytes}}, "ModUp input and output overlap!");
            if (input_ntt)
            {
                T* tmp = words_at<T>(scratch, s.c_coeff);
                refuse_overlap({{tmp, s.inner_out - s.c_coeff}}, {{a, a_bytes}, {c_in, c_bytes}},
                               "The scratch overlaps an operand!");
                ntt_q_i->execute(c_in, tmp, count * L, stream);
                coeff = tmp;
            }
            mod_up(coeff, a, count, BaseConvMode::centred, stream);
            ntt_full_f->execute(a, a, D * count * M, stream);
        }

        void switch_digits(const T* a, const T* key, T* out, int count, int C, bool output_ntt, void* scratch,
                           hipStream_t stream) const
        {
            need_transforms();
            const KsScratch s = ks_scratch<T>(L, M, D, n, count, C);
            need_pointers(a, key, out, scratch);
            if (count == 0)
                return;
            T* acc = words_at<T>(scratch, s.inner_out);
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            refuse_overlap({{acc, cols * M * C * sizeof(T)}}, {{out, cols * L * C * sizeof(T)}}, "The scratch overlaps out!");
            // a or key overlapping the accumulators in the scratch: refused by the inner product's own check of its
            // output against its inputs, before its launch -- the first of this call
            inner->multiply_accumulate(a, key, acc, n, D, C, count, false, KM, limbs.data(), stream);
            finish(acc, out, C * count, output_ntt, false, stream);
        }

        // the tail of every switch: acc T[stacks][M][N] in the NTT domain -> out T[stacks][L][N]
        // rescale: -> out T[stacks][Lk][N], divided by P q_{L-R} ... q_{L-1} in the one ModDown
        void finish(T* acc, T* out, int stacks, bool output_ntt, bool rescale, hipStream_t stream) const
        {
            ntt_full_i->execute(acc, acc, stacks * M, stream);
            if (rescale)
                mod_down_rescale(acc, out, stacks, stream);
            else
                mod_down(acc, out, stacks, stream);
            if (output_ntt)
                (rescale ? ntt_keep_f : ntt_q_f)->execute(out, out, stacks * (rescale ? Lk : L), stream);
        }

        // a Galois element reduced as GPU_Automorphism_NTT reduces it (odd, or refused) and its inverse
        std::uint32_t galois_checked(std::uint32_t element, std::uint32_t& inverse) const
        {
            const std::uint32_t mask = negacyclic ? (2u << n) - 1u : (1u << n) - 1u;
            const std::uint32_t k = element & mask;
            if ((k & 1u) == 0u)
                throw std::invalid_argument("Invalid Galois element (must be odd)!");
            inverse = galois_inverse(k) & mask;
            return k;
        }

        // what the kernel arguments of the pipeline calls carry of the base: the key limb of every modulus, P mod q_j
        // and its Shoup companion
        void fill_base(unsigned char* limb, T* p_mod_q_out, T* p_mod_q_shoup_out) const
        {
            for (int m = 0; m < M; m++)
                limb[m] = static_cast<unsigned char>(limbs[m]);
            std::copy(p_mod_q.begin(), p_mod_q.end(), p_mod_q_out);
            std::copy(p_mod_q_shoup.begin(), p_mod_q_shoup.end(), p_mod_q_shoup_out);
        }

        // What rotate_hoisted (groups = G, no weights) and rotate_hoisted_sum (groups = 1) share up to the launch: every
        // refusal of the call, in one order, and the kernel arguments.  out: T[groups][2][count][L][N], the scratch:
        // T[groups][2][count][M][N]; weights: G device pointers (each may be null) or null.  Returns the stacks the tail
        // runs over, 2 * groups * count; 0: count is 0 and nothing is to be launched.  rescale: out has Lk limbs per stack
        int hoist_prepare(const T* a, const T* c0, const T* const* keys, const std::uint32_t* elts,
                          const T* const* weights, int G, int groups, const T* out, int count, const void* scratch,
                          kern::HoistArgs<T>& args, bool rescale = false) const
        {
            need_transforms();
            if (rescale)
                need_rescale();
            const size_t acc_bytes = ks_hoisted_scratch<T>(M, n, count, groups); // checks count (and G = groups)
            if (G < 1 || G > GALOIS_MAX_COUNT)
                throw std::invalid_argument("Invalid galois_count!");
            need_pointers(a, keys, elts, out, scratch);
            need_aligned_scratch(scratch);
            args.count = G;
            for (int g = 0; g < G; g++)
            {
                args.elt[g] = galois_checked(elts[g], args.inv[g]);
                need_pointers(keys[g]);
                args.key[g] = keys[g];
            }
            fill_base(args.limb, args.p_mod_q, args.p_mod_q_shoup);
            if (count == 0)
                return 0;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t out_bytes = cols * (rescale ? Lk : L) * 2 * groups * sizeof(T);
            const std::uint64_t key_bytes = ((static_cast<std::uint64_t>(D) * 2 * KM) << n) * sizeof(T);
            const std::uint64_t weight_bytes = (static_cast<std::uint64_t>(M) << n) * sizeof(T);
            const char* operand = "out or the scratch overlaps an operand!";
            const std::initializer_list<host::RnsRange> written = {{out, out_bytes}, {scratch, acc_bytes}};
            refuse_overlap(written, {{a, cols * M * D * sizeof(T)}, {c0, cols * L * sizeof(T)}}, operand);
            for (int g = 0; g < G; g++)
                refuse_overlap(written, {{keys[g], key_bytes}, {weights != nullptr ? weights[g] : nullptr, weight_bytes}},
                               operand);
            refuse_overlap({{out, out_bytes}}, {{scratch, acc_bytes}}, "The scratch overlaps out!");
            const unsigned long long stacks = 2ull * static_cast<unsigned>(groups) * static_cast<unsigned>(count);
            need_int_batch(stacks * static_cast<unsigned>(M), "Invalid count!"); // the batch of the transforms
            // mod_down's own grid limit, checked before the first launch
            (void) column_tiles(stacks << n, kern::BC_NT, "Invalid count!");
            return static_cast<int>(stacks);
        }

        void rotate_hoisted(const T* a, const T* c0, const T* const* keys, const std::uint32_t* elts, int G, T* out,
                            int count, bool output_ntt, void* scratch, hipStream_t stream) const
        {
            kern::HoistArgs<T> args{};
            const int stacks = hoist_prepare(a, c0, keys, elts, nullptr, G, G, out, count, scratch, args);
            if (stacks == 0)
                return;
            T* acc = static_cast<T*>(scratch);
            // the first launch of the call: its own grid check throws before it
            host::hoist_launch<T>(a, c0, acc, reinterpret_cast<const T*>(ws + lay.inner), args, D, count, L, M, KM, n,
                                  negacyclic, stream);
            finish(acc, out, stacks, output_ntt, false, stream);
        }

        void rotate_hoisted_sum(const T* a, const T* c0, const T* const* keys, const std::uint32_t* elts,
                                const T* const* weights, int G, T* out, int count, bool output_ntt, bool rescale,
                                void* scratch, hipStream_t stream) const
        {
            kern::HoistSumArgs<T> args{};
            const int stacks = hoist_prepare(a, c0, keys, elts, weights, G, 1, out, count, scratch, args.h, rescale);
            if (stacks == 0)
                return;
            for (int g = 0; g < G && weights != nullptr; g++)
                args.weight[g] = weights[g];
            T* acc = static_cast<T*>(scratch);
            // the first launch of the call: its own grid check throws before it
            host::hoist_sum_launch<T>(a, c0, acc, reinterpret_cast<const T*>(ws + lay.inner), args, D, count, L, M, KM, n,
                                      negacyclic, stream);
            finish(acc, out, stacks, output_ntt, rescale, stream);
        }

        // One axis of linear_transform_bsgs: the steps with a key first (into `args`, in their order), then the others;
        // order[i] = the caller's index of step i of the scratch.  Returns the number of keyed steps
        int bsgs_axis(const T* const* keys, const std::uint32_t* elts, int steps, kern::HoistArgs<T>& args,
                      int* order) const
        {
            int keyed = 0;
            for (int i = 0; i < steps; i++)
            {
                std::uint32_t inverse;
                const std::uint32_t k = galois_checked(elts[i], inverse);
                if (keys[i] == nullptr && k != 1u)
                    throw std::invalid_argument("A null key is accepted only where the element is 1!");
                if (keys[i] != nullptr)
                {
                    args.elt[keyed] = k, args.inv[keyed] = inverse, args.key[keyed] = keys[i];
                    order[keyed++] = i;
                }
            }
            args.count = keyed;
            for (int i = 0, at = keyed; i < steps; i++)
                if (keys[i] == nullptr)
                    order[at++] = i;
            fill_base(args.limb, args.p_mod_q, args.p_mod_q_shoup);
            return keyed;
        }

        void linear_transform_bsgs(const T* a, const T* c0, const T* c1, const T* const* bkeys,
                                   const std::uint32_t* belts, int n1, const T* const* gkeys,
                                   const std::uint32_t* gelts, int n2, const T* const* weights, T* out, int count,
                                   bool output_ntt, bool rescale, void* scratch, hipStream_t stream) const
        {
            need_transforms();
            if (rescale)
                need_rescale();
            const KsBsgsScratch s = ks_bsgs_scratch<T>(L, M, D, n, count, n1, n2); // checks count, n1 and n2
            need_pointers(a, bkeys, belts, gkeys, gelts, weights, out, scratch);
            need_aligned_scratch(scratch);
            kern::HoistArgs<T> bargs{}, gargs{};
            int border[KEYSWITCH_MAX_STEPS], gorder[KEYSWITCH_MAX_STEPS];
            const int n1k = bsgs_axis(bkeys, belts, n1, bargs, border);
            const int n2k = bsgs_axis(gkeys, gelts, n2, gargs, gorder);
            if (n1k < n1)
                need_pointers(c1); // a baby step without a key reads c1
            kern::BsgsWeights<T> wa{};
            wa.n1 = n1, wa.n2 = n2;
            for (int g = 0; g < n2; g++)
            {
                bool any = false;
                for (int b = 0; b < n1; b++)
                {
                    wa.w[g * n1 + b] = weights[gorder[g] * n1 + border[b]];
                    any = any || wa.w[g * n1 + b] != nullptr;
                }
                if (!any)
                    throw std::invalid_argument("A giant step has no present weight!");
            }
            if (count == 0)
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t c_bytes = cols * L * sizeof(T);
            const std::uint64_t out_bytes = cols * (rescale ? Lk : L) * 2 * sizeof(T);
            const std::uint64_t key_bytes = ((static_cast<std::uint64_t>(D) * 2 * KM) << n) * sizeof(T);
            const std::uint64_t weight_bytes = (static_cast<std::uint64_t>(M) << n) * sizeof(T);
            const char* operand = "out or the scratch overlaps an operand!";
            const std::initializer_list<host::RnsRange> written = {{out, out_bytes}, {scratch, s.total}};
            refuse_overlap(written, {{a, cols * M * D * sizeof(T)}, {c0, c_bytes}, {c1, c_bytes}}, operand);
            for (int i = 0; i < n1k; i++)
                refuse_overlap(written, {{bargs.key[i], key_bytes}}, operand);
            for (int i = 0; i < n2k; i++)
                refuse_overlap(written, {{gargs.key[i], key_bytes}}, operand);
            for (int i = 0; i < n1 * n2; i++)
                refuse_overlap(written, {{wa.w[i], weight_bytes}}, operand);
            refuse_overlap({{out, out_bytes}}, {{scratch, s.total}}, "The scratch overlaps out!");
            // every limit before the first launch, at n2 keyed giant steps whatever their number is: the batches of the
            // transforms are ints; the grids of mod_up, mod_down and the five kernels of hoisted_rotation.hip launch at
            // most stacks * max(N, 256) work-items
            const unsigned long long stacks = static_cast<unsigned long long>(n2 > 2 ? n2 : 2) * static_cast<unsigned>(count);
            need_int_batch(stacks * static_cast<unsigned>(D) * static_cast<unsigned>(M), "Invalid count!");
            if (stacks * ((1ull << n) > 256ull ? (1ull << n) : 256ull) > 0xFFFFFFFFull)
                throw std::invalid_argument("Invalid count!");

            T* u = words_at<T>(scratch, s.u);
            T* v = words_at<T>(scratch, s.v);
            T* t = words_at<T>(scratch, s.t);
            T* a2 = words_at<T>(scratch, s.a2);
            T* acc = u; // u is dead once v is formed
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            // 1. the baby steps: u[b] for the keyed b < n1k, then the others
            if (n1k > 0)
                host::hoist_launch<T>(a, c0, u, consts, bargs, D, count, L, M, KM, n, negacyclic, stream);
            if (n1k < n1)
                host::bsgs_scale_launch<T>(c0, c1, u, consts, bargs, n1k, n1, count, L, M, n, stream);
            // 2. all n2 weighted sums
            host::bsgs_sum_launch<T>(u, v, consts, wa, count, M, n, stream);
            // 3. the second components of the keyed giant steps, one contiguous T[n2k * count][M][N]: to coefficient
            //    form, down to the q-base and into digits again
            if (n2k > 0)
            {
                T* v1 = v + static_cast<size_t>(n2) * cols * M;
                ntt_full_i->execute(v1, v1, n2k * count * M, stream);
                mod_down(v1, t, n2k * count, stream);
                mod_up(t, a2, n2k * count, BaseConvMode::centred, stream);
                ntt_full_f->execute(a2, a2, D * n2k * count * M, stream);
            }
            // 4. the giant steps, summed
            host::bsgs_giant_launch<T>(a2, v, acc, consts, gargs, n2, D, count, M, KM, n, negacyclic, stream);
            // 5. ONE ModDown
            finish(acc, out, 2 * count, output_ntt, rescale, stream);
        }

        // the limits of the relinearizing calls, before their first launch: the batches of the transforms are ints; the
        // grids of mod_up and mod_down: as their own launches check
        void relin_limits(std::uint64_t cols, int count) const
        {
            need_int_batch(static_cast<unsigned long long>(D) * static_cast<unsigned>(count) * static_cast<unsigned>(M),
                           "Invalid count!");
            (void) column_tiles(cols, kern::KS_NT, "Invalid count!");
            (void) column_tiles(2 * cols, kern::BC_NT, "Invalid count!");
        }

        struct RelinScratch // the regions of ks_scratch(count, 2): the digits, the top term, the accumulators
        {
            T *a, *d2, *acc;
        };

        // What multiply_relinearize (one term: xs = &x, ys = &y) and multiply_relinearize_sum share up to the first
        // launch: every refusal of the call, in one order, the kernel arguments of the base and the regions of the
        // scratch.  Returns false when count is 0 and nothing is to be launched
        bool relin_prepare(const T* const* xs, const T* const* ys, int terms, const T* key, const T* out, int count,
                           bool rescale, void* scratch, kern::RelinArgs<T>& args, RelinScratch& r) const
        {
            need_transforms();
            if (rescale)
                need_rescale();
            const KsScratch s = ks_scratch<T>(L, M, D, n, count, 2); // checks count
            if (terms < 1 || terms > KEYSWITCH_MAX_TERMS)
                throw std::invalid_argument("Invalid terms!");
            need_pointers(xs, ys, key, out, scratch);
            for (int t = 0; t < terms; t++)
                need_pointers(xs[t], ys[t]);
            need_aligned_scratch(scratch);
            if (count == 0)
                return false;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t ct_bytes = cols * L * 2 * sizeof(T);
            const std::uint64_t out_bytes = cols * (rescale ? Lk : L) * 2 * sizeof(T);
            const std::uint64_t key_bytes = ((static_cast<std::uint64_t>(D) * 2 * KM) << n) * sizeof(T);
            const char* operand = "out or the scratch overlaps an operand!";
            // out may be exactly any x[t] or y[t]: the last read of them (inner_product_tensor[_sum]) precedes mod_down's
            // first write on the stream.  Any other overlap is refused
            refuse_overlap({{scratch, s.total}, {out, out_bytes}}, {{key, key_bytes}}, operand);
            for (int t = 0; t < terms; t++)
            {
                refuse_overlap({{scratch, s.total}}, {{xs[t], ct_bytes}, {ys[t], ct_bytes}}, operand);
                refuse_overlap({{out, out_bytes}}, {{xs[t], ct_bytes, true}, {ys[t], ct_bytes, true}}, operand);
            }
            refuse_overlap({{out, out_bytes}}, {{scratch, s.total}}, "The scratch overlaps out!");
            relin_limits(cols, count);
            fill_base(args.limbs.v, args.p_mod_q, args.p_mod_q_shoup);
            r = RelinScratch{words_at<T>(scratch, s.a), words_at<T>(scratch, s.c_coeff), words_at<T>(scratch, s.inner_out)};
            return true;
        }

        // x, y: T[2][count][L][N]; out: T[2][count][L][N], rescale: T[2][count][Lk][N]; key: T[D_key][2][KM][N]; the
        // scratch: ks_scratch(count, 2)
        void multiply_relinearize(const T* x, const T* y, const T* key, T* out, int count, bool output_ntt, bool rescale,
                                  void* scratch, hipStream_t stream) const
        {
            kern::RelinArgs<T> args{};
            RelinScratch r{};
            if (!relin_prepare(&x, &y, 1, key, out, count, rescale, scratch, args, r))
                return;
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const T* x1 = x + cols * L;
            const T* y1 = y + cols * L;
            // the grid limits of both kernels, before the first launch
            host::relin_top_launch<T>(x1, y1, r.d2, consts, count, L, M, n, false, stream);
            host::relin_inner_launch<T>(r.a, key, r.acc, consts, x, y, args, D, count, L, M, KM, n, false, stream);

            host::relin_top_launch<T>(x1, y1, r.d2, consts, count, L, M, n, true, stream);
            ntt_q_i->execute(r.d2, r.d2, count * L, stream);
            mod_up(r.d2, r.a, count, BaseConvMode::centred, stream);
            ntt_full_f->execute(r.a, r.a, D * count * M, stream);
            host::relin_inner_launch<T>(r.a, key, r.acc, consts, x, y, args, D, count, L, M, KM, n, true, stream);
            finish(r.acc, out, 2 * count, output_ntt, rescale, stream);
        }

        // xs, ys: host arrays of `terms` pointers to T[2][count][L][N]; everything else as multiply_relinearize
        void multiply_relinearize_sum(const T* const* xs, const T* const* ys, int terms, const T* key, T* out, int count,
                                      bool output_ntt, bool rescale, void* scratch, hipStream_t stream) const
        {
            kern::RelinSumArgs<T> args{};
            RelinScratch r{};
            if (!relin_prepare(xs, ys, terms, key, out, count, rescale, scratch, args.r, r))
                return;
            args.terms = terms;
            for (int t = 0; t < terms; t++)
                args.x[t] = xs[t], args.y[t] = ys[t];
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            // the grid limits of both kernels, before the first launch
            host::relin_sum_top_launch<T>(r.d2, consts, args, count, L, M, n, false, stream);
            host::relin_sum_inner_launch<T>(r.a, key, r.acc, consts, args, D, count, L, M, KM, n, false, stream);

            host::relin_sum_top_launch<T>(r.d2, consts, args, count, L, M, n, true, stream);
            ntt_q_i->execute(r.d2, r.d2, count * L, stream);
            mod_up(r.d2, r.a, count, BaseConvMode::centred, stream);
            ntt_full_f->execute(r.a, r.a, D * count * M, stream);
            host::relin_sum_inner_launch<T>(r.a, key, r.acc, consts, args, D, count, L, M, KM, n, true, stream);
            finish(r.acc, out, 2 * count, output_ntt, rescale, stream);
        }

        // c01: T[2][count][L][N], c2: T[count][L][N], out: T[2][count][L][N]; key: T[D_key][2][KM][N]; the scratch:
        // ks_scratch(count, 2)
        void relinearize(const T* c01, const T* c2, const T* key, T* out, int count, bool input_ntt, bool output_ntt,
                         void* scratch, hipStream_t stream) const
        {
            need_transforms();
            const KsScratch s = ks_scratch<T>(L, M, D, n, count, 2); // checks count
            need_pointers(c01, c2, key, out, scratch);
            need_aligned_scratch(scratch);
            if (count == 0)
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t low_bytes = cols * L * 2 * sizeof(T), top_bytes = cols * L * sizeof(T);
            const std::uint64_t key_bytes = ((static_cast<std::uint64_t>(D) * 2 * KM) << n) * sizeof(T);
            const char* operand = "out or the scratch overlaps an operand!";
            refuse_overlap({{scratch, s.total}}, {{c01, low_bytes}, {c2, top_bytes}, {key, key_bytes}}, operand);
            // out may be exactly c01: every word of c01 is read by the lane that later writes it (mod_down_add), or all of
            // it is read before mod_down's first write on the stream (inner_product_seeded).  Any other overlap is refused
            refuse_overlap({{out, low_bytes}}, {{c2, top_bytes}, {key, key_bytes}, {c01, low_bytes, true}}, operand);
            refuse_overlap({{c01, low_bytes}}, {{c2, top_bytes}, {key, key_bytes}}, operand);
            refuse_overlap({{c2, top_bytes}}, {{key, key_bytes}}, operand);
            refuse_overlap({{out, low_bytes}}, {{scratch, s.total}}, "The scratch overlaps out!");
            relin_limits(cols, count);
            T* a = words_at<T>(scratch, s.a);
            T* acc = words_at<T>(scratch, s.inner_out);
            if (!input_ntt)
            {
                // c01 is in coefficient form: it joins after the division, in mod_down's own epilogue
                mod_up(c2, a, count, BaseConvMode::centred, stream);
                ntt_full_f->execute(a, a, D * count * M, stream);
                inner->multiply_accumulate(a, key, acc, n, D, 2, count, false, KM, limbs.data(), stream);
                ntt_full_i->execute(acc, acc, 2 * count * M, stream);
                mod_down_add(acc, c01, out, 2 * count, stream);
                if (output_ntt)
                    ntt_q_f->execute(out, out, 2 * count * L, stream);
                return;
            }
            kern::RelinArgs<T> args{};
            fill_base(args.limbs.v, args.p_mod_q, args.p_mod_q_shoup);
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            // the grid limit of the kernel, before the first launch
            host::relin_seeded_launch<T>(a, key, acc, consts, c01, args, D, count, L, M, KM, n, false, stream);
            decompose(c2, a, count, true, scratch, stream);
            host::relin_seeded_launch<T>(a, key, acc, consts, c01, args, D, count, L, M, KM, n, true, stream);
            finish(acc, out, 2 * count, output_ntt, false, stream);
        }

        // Key material (keygen.hip)

        // What lift_small and lift_centred share between their own refusals and their launches; in: [polys][N] words of
        // in_word bytes, out: T[polys][B][N].  Returns false when polys is 0 and nothing is to be launched
        bool lift_prepare(const void* in, std::uint64_t in_word, const T* out, int polys, int B) const
        {
            if (polys < 0)
                throw std::invalid_argument("Invalid polys!");
            need_pointers(in, out);
            need_int_batch(static_cast<unsigned long long>(polys) * static_cast<unsigned>(B), "Invalid polys!");
            if (polys == 0)
                return false;
            const std::uint64_t cols = static_cast<std::uint64_t>(polys) << n;
            refuse_overlap({{out, cols * B * sizeof(T)}}, {{in, cols * in_word}}, "The lift's input and output overlap!");
            return true;
        }

        // small: int32[polys][N] -> out: T[polys][B][N], B = M (full_base) or L
        void lift_small(const std::int32_t* small, T* out, int polys, bool full_base, bool to_ntt, hipStream_t stream) const
        {
            if (to_ntt)
                need_transforms();
            const int B = full_base ? M : L;
            if (!lift_prepare(small, sizeof(std::int32_t), out, polys, B))
                return;
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            host::keygen_lift_launch<T>(small, out, consts, polys, B, M, n, false, stream);
            host::keygen_lift_launch<T>(small, out, consts, polys, B, M, n, true, stream);
            if (to_ntt)
                (full_base ? ntt_full_f : ntt_q_f)->execute(out, out, polys * B, stream);
        }

        // Plaintext operands (keygen.hip)

        // words: T[polys][N], read modulo t and centred -> out: T[polys][B][N], B = M (full_base) or L
        void lift_centred(const T* words, T t, T* out, int polys, bool full_base, bool to_ntt, hipStream_t stream) const
        {
            if (to_ntt)
                need_transforms();
            if (t < 2 || (t >> (8 * sizeof(T) - 1)) != 0) // (Modulus<T> leaves mu = 0 from 2^(W-1) on and does not throw)
                throw std::invalid_argument("Invalid plaintext modulus!");
            try
            {
                (void) Modulus<T>(t); // what Modulus<T> accepts: below 2^(W-1), all the Shoup product by 1 needs
            }
            catch (const std::invalid_argument&)
            {
                throw std::invalid_argument("Invalid plaintext modulus!");
            }
            const int B = full_base ? M : L;
            if (!lift_prepare(words, sizeof(T), out, polys, B))
                return;
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            host::lift_centred_launch<T>(words, out, consts, t, polys, B, M, n, false, stream);
            host::lift_centred_launch<T>(words, out, consts, t, polys, B, M, n, true, stream);
            if (to_ntt)
                (full_base ? ntt_full_f : ntt_q_f)->execute(out, out, polys * B, stream);
        }

        // ct, out: T[2][count][L][N], pt: T[plain_count][L][N], all in NTT form
        void multiply_plain(const T* ct, const T* pt, T* out, int count, int plain_count, hipStream_t stream) const
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (plain_count != 1 && plain_count != count)
                throw std::invalid_argument("Invalid plain_count!");
            need_pointers(ct, pt, out);
            if (count == 0)
                return;
            const std::uint64_t stack = (static_cast<std::uint64_t>(L) << n) * sizeof(T);
            const std::uint64_t ct_bytes = 2 * stack * count, pt_bytes = stack * plain_count;
            // out may be exactly ct: every word is written by the lane that read it, after its loads
            refuse_overlap({{out, ct_bytes}}, {{ct, ct_bytes, true}, {pt, pt_bytes}}, "out overlaps an operand!");
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            host::multiply_plain_launch<T>(ct, pt, out, consts, count, plain_count, L, M, n, false, stream);
            host::multiply_plain_launch<T>(ct, pt, out, consts, count, plain_count, L, M, n, true, stream);
        }

        size_t keygen_scratch(int keys) const // E: T[keys][D][M][N]
        {
            if (keys < 0 || keys > KEYGEN_MAX_KEYS)
                throw std::invalid_argument("Invalid keys!");
            return rns_align(((static_cast<size_t>(keys) * D * M) << n) * sizeof(T));
        }
        size_t lifted_scratch(int count, int polys) const // what lift_small makes of int32[polys][count][N] over the q-base
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            return rns_align(((static_cast<size_t>(polys) * count * L) << n) * sizeof(T));
        }
        size_t encrypt_scratch(int count) const { return lifted_scratch(count, 1); }        // E: T[count][L][N]
        size_t encrypt_public_scratch(int count) const { return lifted_scratch(count, 3); } // (U, E0, E1): T[3][count][L][N]

        // What encrypt_symmetric (polys = 1, key = s, L limbs read) and encrypt_public (polys = 3, key = pk, 2 L limbs)
        // share up to the first launch: every refusal of the call, in one order.  small: int32[polys][count][N].  Returns
        // false when count is 0 and nothing is to be launched
        bool encrypt_prepare(const T* key, int key_limbs, const std::int32_t* small, int polys, const T* message,
                             const T* out, int count, const void* scratch) const
        {
            need_transforms();
            const size_t e_bytes = lifted_scratch(count, polys); // checks count
            need_pointers(key, small, out, scratch);
            need_aligned_scratch(scratch);
            need_int_batch(static_cast<unsigned long long>(polys) * static_cast<unsigned>(count) * static_cast<unsigned>(L),
                           "Invalid count!");
            if (count == 0)
                return false;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t ct_bytes = cols * L * 2 * sizeof(T);
            refuse_overlap({{scratch, e_bytes}, {out, ct_bytes}},
                           {{key, (static_cast<std::uint64_t>(key_limbs) << n) * sizeof(T)},
                            {small, polys * cols * sizeof(std::int32_t)},
                            {message, cols * L * sizeof(T)}},
                           "out or the scratch overlaps an operand!");
            refuse_overlap({{out, ct_bytes}}, {{scratch, e_bytes}}, "The scratch overlaps out!");
            return true;
        }

        // s: T[M][N], s_from: T[keys][M][N], errors: int32[keys][D][N], key_ptrs: a host array of `keys` device
        // pointers to T[D][2][M][N]; the scratch: keygen_scratch(keys)
        void generate_keys(const T* s, const T* s_from, const std::int32_t* errors, T* const* key_ptrs, int keys,
                           void* scratch, hipStream_t stream) const
        {
            need_transforms();
            const size_t e_bytes = keygen_scratch(keys); // checks keys
            if (KM != M)
                throw std::invalid_argument("Keys are generated by the plan of the level they are laid out for!");
            for (int m = 0; m < M; m++)
                if (limbs[m] != m)
                    throw std::invalid_argument("Keys are generated by the plan of the level they are laid out for!");
            need_pointers(s, s_from, errors, key_ptrs, scratch);
            for (int g = 0; g < keys; g++)
                need_pointers(key_ptrs[g]);
            need_aligned_scratch(scratch);
            if (keys == 0)
                return;
            const std::uint64_t stack = (static_cast<std::uint64_t>(M) << n) * sizeof(T);
            const std::uint64_t key_bytes = stack * 2 * D, from_bytes = stack * keys;
            const std::uint64_t err_bytes = ((static_cast<std::uint64_t>(keys) * D) << n) * sizeof(std::int32_t);
            for (const host::RnsRange& op : {host::RnsRange{s, stack}, {s_from, from_bytes}, {errors, err_bytes}})
            {
                refuse_overlap({{scratch, e_bytes}}, {op}, "The scratch overlaps an operand!");
                for (int g = 0; g < keys; g++)
                    refuse_overlap({{key_ptrs[g], key_bytes}}, {op}, "A key overlaps an operand!");
            }
            for (int g = 0; g < keys; g++)
            {
                refuse_overlap({{key_ptrs[g], key_bytes}}, {{scratch, e_bytes}}, "The scratch overlaps a key!");
                for (int o = g + 1; o < keys; o++)
                    refuse_overlap({{key_ptrs[g], key_bytes}}, {{key_ptrs[o], key_bytes}}, "Two keys overlap!");
            }
            kern::KeygenArgs<T> args{};
            for (int g = 0; g < keys; g++)
                args.group[g] = key_ptrs[g];
            for (int j = 0; j < L; j++)
                args.mult[j] = p_mod_q[j];
            const unsigned long long poly = 1ull << n;
            const kern::KeygenShape shape{2 * M * poly, M * poly, M * poly, 0, D, M, L, alpha};
            T* e = static_cast<T*>(scratch);
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            // the grid limits of both kernels, before the first launch
            host::keygen_lift_launch<T>(errors, e, consts, keys * D, M, M, n, false, stream);
            host::keygen_combine_launch<T>(e, s, s_from, args, shape, keys, consts, M, n, false, stream);
            host::keygen_lift_launch<T>(errors, e, consts, keys * D, M, M, n, true, stream);
            ntt_full_f->execute(e, e, keys * D * M, stream);
            host::keygen_combine_launch<T>(e, s, s_from, args, shape, keys, consts, M, n, true, stream);
        }

        // s: T[M][N] (the first L limbs are read), errors: int32[count][N], message: T[count][L][N] or nullptr,
        // out: T[2][count][L][N] with out[1] = a; the scratch: encrypt_scratch(count)
        void encrypt_symmetric(const T* s, const std::int32_t* errors, const T* message, T* out, int count, void* scratch,
                               hipStream_t stream) const
        {
            if (!encrypt_prepare(s, L, errors, 1, message, out, count, scratch))
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            kern::KeygenArgs<T> args{};
            args.group[0] = out;
            for (int j = 0; j < L; j++)
                args.mult[j] = T(1);
            const unsigned long long poly = 1ull << n;
            const kern::KeygenShape shape{L * poly, cols * L, 0, L * poly, count, L, L, 0};
            T* e = static_cast<T*>(scratch);
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            host::keygen_lift_launch<T>(errors, e, consts, count, L, M, n, false, stream);
            host::keygen_combine_launch<T>(e, s, message, args, shape, 1, consts, M, n, false, stream);
            host::keygen_lift_launch<T>(errors, e, consts, count, L, M, n, true, stream);
            ntt_q_f->execute(e, e, count * L, stream);
            host::keygen_combine_launch<T>(e, s, message, args, shape, 1, consts, M, n, true, stream);
        }

        // Decryption and public-key encryption (decrypt.hip)

        static void phase_components(int components)
        {
            if (components != 2 && components != 3)
                throw std::invalid_argument("Invalid components!");
        }
        size_t phase_scratch(int count, int components, bool input_ntt) const // the NTT of ct: T[components][count][L][N]
        {
            phase_components(components);
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (input_ntt)
                return 0;
            return rns_align(((static_cast<size_t>(components) * count * L) << n) * sizeof(T));
        }

        // ct: T[components][count][L][N], s: T[M][N] (the first L limbs are read), out: T[count][L][N]; the scratch:
        // phase_scratch(count, components, input_ntt)
        void phase(const T* ct, const T* s, T* out, int count, int components, bool input_ntt, bool output_ntt,
                   void* scratch, hipStream_t stream) const
        {
            if (!input_ntt || !output_ntt)
                need_transforms();
            const size_t s_bytes = phase_scratch(count, components, input_ntt); // checks components and count
            need_pointers(ct, s, out);
            if (!input_ntt)
            {
                need_pointers(scratch);
                need_aligned_scratch(scratch);
            }
            need_int_batch(static_cast<unsigned long long>(components) * static_cast<unsigned>(count) * static_cast<unsigned>(L),
                           "Invalid count!"); // the transforms' batch
            if (count == 0)
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t out_bytes = cols * L * sizeof(T), ct_bytes = out_bytes * components;
            const std::uint64_t sec_bytes = (static_cast<std::uint64_t>(L) << n) * sizeof(T);
            // out may be exactly ct in NTT form: every word of component 0 is written by the lane that read it
            refuse_overlap({{out, out_bytes}}, {{ct, ct_bytes, input_ntt}, {s, sec_bytes}}, "out overlaps an operand!");
            if (!input_ntt)
            {
                refuse_overlap({{scratch, s_bytes}}, {{ct, ct_bytes}, {s, sec_bytes}}, "out or the scratch overlaps an operand!");
                refuse_overlap({{scratch, s_bytes}}, {{out, out_bytes}}, "The scratch overlaps out!");
            }
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            const T* c = input_ntt ? ct : static_cast<const T*>(scratch);
            host::decrypt_phase_launch<T>(c, s, out, consts, count, components, L, M, n, false, stream);
            if (!input_ntt)
                ntt_q_f->execute(ct, static_cast<T*>(scratch), components * count * L, stream);
            host::decrypt_phase_launch<T>(c, s, out, consts, count, components, L, M, n, true, stream);
            if (!output_ntt)
                ntt_q_i->execute(out, out, count * L, stream);
        }

        // pk: T[2][L][N], small: int32[3][count][N] = (u, e0, e1), message: T[count][L][N] or nullptr,
        // out: T[2][count][L][N]; the scratch: encrypt_public_scratch(count)
        void encrypt_public(const T* pk, const std::int32_t* small, const T* message, T* out, int count, void* scratch,
                            hipStream_t stream) const
        {
            if (!encrypt_prepare(pk, 2 * L, small, 3, message, out, count, scratch))
                return;
            T* e = static_cast<T*>(scratch);
            const T* consts = reinterpret_cast<const T*>(ws + lay.inner);
            host::keygen_lift_launch<T>(small, e, consts, 3 * count, L, M, n, false, stream);
            host::encrypt_public_combine_launch<T>(pk, e, message, out, consts, count, L, M, n, false, stream);
            host::keygen_lift_launch<T>(small, e, consts, 3 * count, L, M, n, true, stream);
            ntt_q_f->execute(e, e, 3 * count * L, stream);
            host::encrypt_public_combine_launch<T>(pk, e, message, out, consts, count, L, M, n, true, stream);
        }
    };

    template <typename T>
    size_t KeySwitchPlan<T>::phase_scratch_bytes(int count, int components, bool input_ntt) const
    {
        return p_->phase_scratch(count, components, input_ntt);
    }
    template <typename T>
    void KeySwitchPlan<T>::phase(const T* device_ct, const T* device_s_ntt, T* device_out, int count, int components,
                                 bool input_ntt, bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->phase(device_ct, device_s_ntt, device_out, count, components, input_ntt, output_ntt, scratch_device, stream);
    }
    template <typename T> size_t KeySwitchPlan<T>::encrypt_public_scratch_bytes(int count) const
    {
        return p_->encrypt_public_scratch(count);
    }
    template <typename T>
    void KeySwitchPlan<T>::encrypt_public(const T* device_pk, const std::int32_t* device_small,
                                          const T* device_message_ntt, T* device_out, int count, void* scratch_device,
                                          stream_t stream) const
    {
        p_->encrypt_public(device_pk, device_small, device_message_ntt, device_out, count, scratch_device, stream);
    }

    template <typename T>
    void KeySwitchPlan<T>::lift_small(const std::int32_t* device_small, T* device_out, int polys, bool full_base,
                                      bool to_ntt, stream_t stream) const
    {
        p_->lift_small(device_small, device_out, polys, full_base, to_ntt, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::lift_centred(const T* device_words, T plain_modulus, T* device_out, int polys, bool full_base,
                                        bool to_ntt, stream_t stream) const
    {
        p_->lift_centred(device_words, plain_modulus, device_out, polys, full_base, to_ntt, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::multiply_plain(const T* device_ct, const T* device_pt_ntt, T* device_out, int count,
                                          int plain_count, stream_t stream) const
    {
        p_->multiply_plain(device_ct, device_pt_ntt, device_out, count, plain_count, stream);
    }
    template <typename T> size_t KeySwitchPlan<T>::keygen_scratch_bytes(int keys) const
    {
        return p_->keygen_scratch(keys);
    }
    template <typename T> size_t KeySwitchPlan<T>::encrypt_scratch_bytes(int count) const
    {
        return p_->encrypt_scratch(count);
    }
    template <typename T>
    void KeySwitchPlan<T>::generate_keys(const T* device_s_ntt, const T* device_s_from_ntt,
                                         const std::int32_t* device_errors, T* const* device_keys_host, int keys,
                                         void* scratch_device, stream_t stream) const
    {
        p_->generate_keys(device_s_ntt, device_s_from_ntt, device_errors, device_keys_host, keys, scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::encrypt_symmetric(const T* device_s_ntt, const std::int32_t* device_errors,
                                             const T* device_message_ntt, T* device_out, int count, void* scratch_device,
                                             stream_t stream) const
    {
        p_->encrypt_symmetric(device_s_ntt, device_errors, device_message_ntt, device_out, count, scratch_device, stream);
    }

    template <typename T> int KeySwitchPlan<T>::digits(int q_count, int alpha)
    {
        if (q_count < 1 || alpha < 1)
            throw std::invalid_argument("Invalid alpha!");
        return ks_digits(q_count, alpha);
    }

    template <typename T>
    size_t KeySwitchPlan<T>::workspace_bytes(int q_count, int p_count, int alpha, int n_power, int rescale_limbs)
    {
        return ks_layout<T>(q_count, p_count, alpha, n_power, rescale_limbs).total;
    }

    template <typename T>
    size_t KeySwitchPlan<T>::scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count, int components)
    {
        ks_check_counts(q_count, p_count, alpha);
        rns_check_n_power(n_power);
        return ks_scratch<T>(q_count, q_count + p_count, ks_digits(q_count, alpha), n_power, count, components).total;
    }

    template <typename T>
    size_t KeySwitchPlan<T>::hoisted_scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count,
                                                   int elements)
    {
        ks_check_counts(q_count, p_count, alpha);
        rns_check_n_power(n_power);
        return ks_hoisted_scratch<T>(q_count + p_count, n_power, count, elements);
    }

    template <typename T>
    size_t KeySwitchPlan<T>::hoisted_sum_scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count)
    {
        ks_check_counts(q_count, p_count, alpha);
        rns_check_n_power(n_power);
        return ks_hoisted_sum_scratch<T>(q_count + p_count, n_power, count);
    }

    template <typename T>
    size_t KeySwitchPlan<T>::bsgs_scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count, int n1,
                                                int n2)
    {
        ks_check_counts(q_count, p_count, alpha);
        rns_check_n_power(n_power);
        return ks_bsgs_scratch<T>(q_count, q_count + p_count, ks_digits(q_count, alpha > q_count ? q_count : alpha),
                                  n_power, count, n1, n2)
            .total;
    }

    template <typename T>
    KeySwitchPlan<T>::KeySwitchPlan(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host,
                                    int p_count, int alpha, int n_power, const Root<T>* forward_table_device,
                                    const Root<T>* inverse_table_device, const Ninverse<T>* mod_inverse_host,
                                    ReductionPolynomial reduction_poly, int batch_hint, int key_mod_count,
                                    const int* key_limbs_host, stream_t stream, void* workspace_device,
                                    int rescale_limbs)
        : p_(nullptr)
    {
        const KsHost h = ks_derive<T>(q_moduli_host, q_count, p_moduli_host, p_count, alpha);
        const KsLayout lay = ks_layout<T>(h.L, h.K, h.alpha, n_power, rescale_limbs);
        const int R = rescale_limbs, Lk = h.L - R;
        const bool transforms = forward_table_device != nullptr || inverse_table_device != nullptr;
        if (transforms && (forward_table_device == nullptr || inverse_table_device == nullptr || mod_inverse_host == nullptr))
            throw std::invalid_argument("null pointer argument");
        if (key_mod_count < h.M || key_mod_count > INNERPROD_MAX_KEY_MODULI)
            throw std::invalid_argument("Invalid key_mod_count!");
        std::unique_ptr<Impl> p(new Impl);
        p->L = h.L, p->K = h.K, p->M = h.M, p->alpha = h.alpha, p->D = h.D, p->n = n_power, p->KM = key_mod_count;
        p->lay = lay;
        p->negacyclic = reduction_poly == ReductionPolynomial::X_N_plus;
        for (int j = 0; j < h.L; j++)
        {
            const std::uint64_t pq = h.down.qmod[j]; // P mod q_j, what constants() returns as down_p_mod_q
            p->p_mod_q.push_back(static_cast<T>(pq));
            p->p_mod_q_shoup.push_back(
                static_cast<T>((static_cast<U128>(pq) << (8 * sizeof(T))) / h.mod[j]));
        }
        for (int m = 0; m < h.M; m++)
        {
            const int l = key_limbs_host != nullptr ? key_limbs_host[m] : m;
            if (l < 0 || l >= key_mod_count)
                throw std::invalid_argument("Invalid key_limbs!");
            p->limbs.push_back(l);
        }
        const std::vector<T> up_img = ks_up_image<T>(h, p->up_off);
        const std::vector<T> down_img = host::bc_image<T>(h.down, p->down_off);
        std::vector<Modulus<T>> full(q_moduli_host, q_moduli_host + h.L);
        full.insert(full.end(), p_moduli_host, p_moduli_host + h.K);
        p->R = R, p->Lk = Lk, p->moduli = full;
        std::vector<T> down_rs_img, rs_img;
        if (R > 0)
        {
            // limbs Lk .. M - 1 of the full base -> the kept q-limbs, and the dropped q-limbs alone -> the kept ones
            down_rs_img = host::bc_image<T>(host::bc_derive<T>(full.data() + Lk, R + h.K, full.data(), Lk), p->down_rs_off);
            rs_img = host::bc_image<T>(host::bc_derive<T>(full.data() + Lk, R, full.data(), Lk), p->rs_off);
            for (int i = 0; i < R; i++)
            {
                p->dropped_mods.q[i] = static_cast<T>(h.mod[Lk + i]);
                p->dropped_mods.onep[i] = static_cast<T>(h.onep[Lk + i]);
            }
        }

        void* raw = workspace_device;
        if (raw == nullptr)
        {
            GPUNTT_HIP_CHECK(hipMalloc(&raw, lay.total));
            p->owns = true;
        }
        p->ws = static_cast<char*>(raw);
        try
        {
            GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws + lay.up, up_img.data(), up_img.size() * sizeof(T), hipMemcpyHostToDevice,
                                            stream));
            GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws + lay.down, down_img.data(), down_img.size() * sizeof(T),
                                            hipMemcpyHostToDevice, stream));
            if (R > 0)
            {
                GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws + lay.down_rs, down_rs_img.data(), down_rs_img.size() * sizeof(T),
                                                hipMemcpyHostToDevice, stream));
                GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws + lay.rs, rs_img.data(), rs_img.size() * sizeof(T),
                                                hipMemcpyHostToDevice, stream));
            }
            GPUNTT_HIP_CHECK(hipStreamSynchronize(stream)); // the images die with this scope
            p->inner.reset(new InnerProductPlan<T>(full.data(), h.M, stream, p->ws + lay.inner));
            if (transforms)
            {
                p->ntt_full_f.reset(new NTTPlan<T>(forward_table_device, full.data(), h.M, n_power, reduction_poly,
                                                   FORWARD, nullptr, batch_hint, stream, p->ws + lay.ntt_full_f));
                p->ntt_full_i.reset(new NTTPlan<T>(inverse_table_device, full.data(), h.M, n_power, reduction_poly,
                                                   INVERSE, mod_inverse_host, batch_hint, stream,
                                                   p->ws + lay.ntt_full_i));
                p->ntt_q_i.reset(new NTTPlan<T>(inverse_table_device, full.data(), h.L, n_power, reduction_poly, INVERSE,
                                                mod_inverse_host, batch_hint, stream, p->ws + lay.ntt_q_i));
                p->ntt_q_f.reset(new NTTPlan<T>(forward_table_device, full.data(), h.L, n_power, reduction_poly, FORWARD,
                                                nullptr, batch_hint, stream, p->ws + lay.ntt_q_f));
                if (R > 0)
                {
                    // forward over the first Lk moduli: the same table pointer; inverse over the R dropped moduli: the
                    // table, the moduli and the n^-1 values Lk slots on
                    p->ntt_keep_f.reset(new NTTPlan<T>(forward_table_device, full.data(), Lk, n_power, reduction_poly,
                                                       FORWARD, nullptr, batch_hint, stream, p->ws + lay.ntt_keep_f));
                    p->ntt_drop_i.reset(new NTTPlan<T>(inverse_table_device + (static_cast<size_t>(Lk) << n_power),
                                                       full.data() + Lk, R, n_power, reduction_poly, INVERSE,
                                                       mod_inverse_host + Lk, batch_hint, stream,
                                                       p->ws + lay.ntt_drop_i));
                }
            }
        }
        catch (...)
        {
            p->ntt_keep_f.reset(), p->ntt_drop_i.reset();
            p->inner.reset(), p->ntt_full_f.reset(), p->ntt_full_i.reset(), p->ntt_q_i.reset(), p->ntt_q_f.reset();
            if (p->owns)
                (void) hipFree(p->ws);
            throw;
        }
        p_ = p.release();
    }

    template <typename T> KeySwitchPlan<T>::~KeySwitchPlan()
    {
        if (p_ == nullptr)
            return;
        p_->ntt_keep_f.reset(), p_->ntt_drop_i.reset();
        p_->inner.reset(), p_->ntt_full_f.reset(), p_->ntt_full_i.reset(), p_->ntt_q_i.reset(), p_->ntt_q_f.reset();
        if (p_->owns)
            (void) hipFree(p_->ws);
        delete p_;
    }

    template <typename T>
    void KeySwitchPlan<T>::mod_up(const T* device_in, T* device_a, int count, BaseConvMode mode, stream_t stream) const
    {
        p_->mod_up(device_in, device_a, count, mode, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::mod_down(const T* device_x, T* device_out, int stacks, stream_t stream) const
    {
        p_->mod_down(device_x, device_out, stacks, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::decompose(const T* device_c_in, T* device_a, int count, bool input_ntt, void* scratch_device,
                                     stream_t stream) const
    {
        p_->decompose(device_c_in, device_a, count, input_ntt, scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::switch_digits(const T* device_a, const T* device_key, T* device_out, int count,
                                         int components, bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->switch_digits(device_a, device_key, device_out, count, components, output_ntt, scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::rotate_hoisted(const T* device_a, const T* device_c0, const T* const* device_keys_host,
                                          const std::uint32_t* galois_elements_host, int elements, T* device_out,
                                          int count, bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->rotate_hoisted(device_a, device_c0, device_keys_host, galois_elements_host, elements, device_out, count,
                           output_ntt, scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::rotate_hoisted_sum(const T* device_a, const T* device_c0, const T* const* device_keys_host,
                                              const std::uint32_t* galois_elements_host,
                                              const T* const* device_weights_host, int elements, T* device_out, int count,
                                              bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->rotate_hoisted_sum(device_a, device_c0, device_keys_host, galois_elements_host, device_weights_host, elements,
                               device_out, count, output_ntt, false, scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::rotate_hoisted_sum_rescale(const T* device_a, const T* device_c0,
                                                      const T* const* device_keys_host,
                                                      const std::uint32_t* galois_elements_host,
                                                      const T* const* device_weights_host, int elements, T* device_out,
                                                      int count, bool output_ntt, void* scratch_device,
                                                      stream_t stream) const
    {
        p_->rotate_hoisted_sum(device_a, device_c0, device_keys_host, galois_elements_host, device_weights_host, elements,
                               device_out, count, output_ntt, true, scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::linear_transform_bsgs(const T* device_a, const T* device_c0, const T* device_c1,
                                                 const T* const* baby_keys_host,
                                                 const std::uint32_t* baby_elements_host, int n1,
                                                 const T* const* giant_keys_host,
                                                 const std::uint32_t* giant_elements_host, int n2,
                                                 const T* const* weights_host, T* device_out, int count, bool output_ntt,
                                                 void* scratch_device, stream_t stream) const
    {
        p_->linear_transform_bsgs(device_a, device_c0, device_c1, baby_keys_host, baby_elements_host, n1, giant_keys_host,
                                  giant_elements_host, n2, weights_host, device_out, count, output_ntt, false,
                                  scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::linear_transform_bsgs_rescale(const T* device_a, const T* device_c0, const T* device_c1,
                                                         const T* const* baby_keys_host,
                                                         const std::uint32_t* baby_elements_host, int n1,
                                                         const T* const* giant_keys_host,
                                                         const std::uint32_t* giant_elements_host, int n2,
                                                         const T* const* weights_host, T* device_out, int count,
                                                         bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->linear_transform_bsgs(device_a, device_c0, device_c1, baby_keys_host, baby_elements_host, n1, giant_keys_host,
                                  giant_elements_host, n2, weights_host, device_out, count, output_ntt, true,
                                  scratch_device, stream);
    }
    template <typename T> size_t KeySwitchPlan<T>::bsgs_scratch_bytes(int count, int n1, int n2) const
    {
        return ks_bsgs_scratch<T>(p_->L, p_->M, p_->D, p_->n, count, n1, n2).total;
    }
    template <typename T>
    void KeySwitchPlan<T>::multiply_relinearize(const T* device_x, const T* device_y, const T* device_key, T* device_out,
                                                int count, bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->multiply_relinearize(device_x, device_y, device_key, device_out, count, output_ntt, false, scratch_device,
                                 stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::multiply_relinearize_rescale(const T* device_x, const T* device_y, const T* device_key,
                                                        T* device_out, int count, bool output_ntt, void* scratch_device,
                                                        stream_t stream) const
    {
        p_->multiply_relinearize(device_x, device_y, device_key, device_out, count, output_ntt, true, scratch_device,
                                 stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::multiply_relinearize_sum_rescale(const T* const* device_x_host, const T* const* device_y_host,
                                                            int terms, const T* device_key, T* device_out, int count,
                                                            bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->multiply_relinearize_sum(device_x_host, device_y_host, terms, device_key, device_out, count, output_ntt, true,
                                     scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::mod_down_rescale(const T* device_x, T* device_out, int stacks, stream_t stream) const
    {
        p_->mod_down_rescale(device_x, device_out, stacks, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::rescale(const T* device_x, T* device_out, int stacks, bool ntt_form, void* scratch_device,
                                   stream_t stream) const
    {
        p_->rescale(device_x, device_out, stacks, ntt_form, scratch_device, stream);
    }
    template <typename T> size_t KeySwitchPlan<T>::rescale_scratch_bytes(int stacks) const
    {
        return p_->rescale_scratch(stacks);
    }
    template <typename T> int KeySwitchPlan<T>::rescale_limbs() const { return p_->R; }

    template <typename T>
    void KeySwitchPlan<T>::multiply_relinearize_sum(const T* const* device_x_host, const T* const* device_y_host, int terms,
                                                    const T* device_key, T* device_out, int count, bool output_ntt,
                                                    void* scratch_device, stream_t stream) const
    {
        p_->multiply_relinearize_sum(device_x_host, device_y_host, terms, device_key, device_out, count, output_ntt, false,
                                     scratch_device, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::apply(const T* device_c_in, const T* device_key, T* device_out, int count, int components,
                                 bool input_ntt, bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->need_transforms();
        const KsScratch s = ks_scratch<T>(p_->L, p_->M, p_->D, p_->n, count, components);
        need_pointers(scratch_device);
        T* a = words_at<T>(scratch_device, s.a);
        if (device_c_in != nullptr && device_out != nullptr && count > 0) // (decompose and switch_digits refuse the rest)
        {
            const std::uint64_t c_bytes = (static_cast<std::uint64_t>(count) << p_->n) * p_->L * sizeof(T);
            refuse_overlap({{scratch_device, s.total}}, {{device_c_in, c_bytes}, {device_out, c_bytes * components}},
                           "The scratch overlaps an operand!");
        }
        p_->decompose(device_c_in, a, count, input_ntt, scratch_device, stream);
        p_->switch_digits(a, device_key, device_out, count, components, output_ntt, scratch_device, stream);
    }

    template <typename T>
    void KeySwitchPlan<T>::mod_down_add(const T* device_x, const T* device_addend, T* device_out, int stacks,
                                        stream_t stream) const
    {
        p_->mod_down_add(device_x, device_addend, device_out, stacks, stream);
    }
    template <typename T>
    void KeySwitchPlan<T>::relinearize(const T* device_c01, const T* device_c2, const T* device_key, T* device_out,
                                       int count, bool input_ntt, bool output_ntt, void* scratch_device,
                                       stream_t stream) const
    {
        p_->relinearize(device_c01, device_c2, device_key, device_out, count, input_ntt, output_ntt, scratch_device,
                        stream);
    }
    template <typename T> Modulus<T> KeySwitchPlan<T>::modulus(int m) const
    {
        if (m < 0 || m >= p_->M)
            throw std::invalid_argument("Invalid modulus index!");
        return p_->moduli[m];
    }
    template <typename T> ReductionPolynomial KeySwitchPlan<T>::reduction_poly() const
    {
        return p_->negacyclic ? ReductionPolynomial::X_N_plus : ReductionPolynomial::X_N_minus;
    }

    template <typename T> int KeySwitchPlan<T>::q_count() const { return p_->L; }
    template <typename T> int KeySwitchPlan<T>::p_count() const { return p_->K; }
    template <typename T> int KeySwitchPlan<T>::key_mod_count() const { return p_->KM; }
    template <typename T> int KeySwitchPlan<T>::alpha() const { return p_->alpha; }
    template <typename T> int KeySwitchPlan<T>::digits() const { return p_->D; }
    template <typename T> int KeySwitchPlan<T>::n_power() const { return p_->n; }
    template <typename T> bool KeySwitchPlan<T>::has_transforms() const { return static_cast<bool>(p_->ntt_full_f); }
    template <typename T> bool KeySwitchPlan<T>::owns_workspace() const { return p_->owns; }
    template <typename T> size_t KeySwitchPlan<T>::scratch_bytes(int count, int components) const
    {
        return ks_scratch<T>(p_->L, p_->M, p_->D, p_->n, count, components).total;
    }
    template <typename T> size_t KeySwitchPlan<T>::hoisted_scratch_bytes(int count, int elements) const
    {
        return ks_hoisted_scratch<T>(p_->M, p_->n, count, elements);
    }
    template <typename T> size_t KeySwitchPlan<T>::hoisted_sum_scratch_bytes(int count) const
    {
        return ks_hoisted_sum_scratch<T>(p_->M, p_->n, count);
    }

    template <typename T>
    void KeySwitchPlan<T>::constants(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host,
                                     int p_count, int alpha, const KeySwitchConstants<T>& out)
    {
        const KsHost h = ks_derive<T>(q_moduli_host, q_count, p_moduli_host, p_count, alpha);
        for (const T* ptr : {out.up_qhat_inv, out.up_qhat_inv_shoup, out.up_matrix, out.up_q_mod, out.up_recip,
                             out.up_bit_length, out.down_qhat_inv, out.down_qhat_inv_shoup, out.down_matrix,
                             out.down_p_mod_q, out.down_p_inv_mod_q, out.down_recip, out.down_bit_length, out.pow_w,
                             out.pow_w_shoup, out.pow_2w, out.pow_2w_shoup, out.one_shoup})
            if (ptr == nullptr)
                throw std::invalid_argument("null pointer argument");
        const int M = h.M;
        for (int d = 0; d < h.D; d++)
        {
            const host::BcHostConsts& u = h.up[d];
            for (int i = h.lo(d); i < h.hi(d); i++)
            {
                const int li = i - h.lo(d);
                out.up_qhat_inv[i] = static_cast<T>(u.w[li]), out.up_qhat_inv_shoup[i] = static_cast<T>(u.wp[li]);
                out.up_recip[i] = static_cast<T>(u.recip[li]), out.up_bit_length[i] = static_cast<T>(u.blen[li]);
            }
            for (int m = 0; m < M; m++)
            {
                const bool own = m >= h.lo(d) && m < h.hi(d);
                out.up_q_mod[static_cast<size_t>(d) * M + m] = own ? T(0) : static_cast<T>(u.qmod[ks_column(h, d, m)]);
                for (int i = h.lo(d); i < h.hi(d); i++)
                    out.up_matrix[static_cast<size_t>(i) * M + m] =
                        own ? T(0)
                            : static_cast<T>(u.matrix[static_cast<size_t>(i - h.lo(d)) * u.K + ks_column(h, d, m)]);
            }
        }
        auto copy = [](const std::vector<std::uint64_t>& v, T* dst) {
            for (size_t i = 0; i < v.size(); i++)
                dst[i] = static_cast<T>(v[i]);
        };
        copy(h.down.w, out.down_qhat_inv), copy(h.down.wp, out.down_qhat_inv_shoup), copy(h.down.matrix, out.down_matrix);
        copy(h.down.qmod, out.down_p_mod_q), copy(h.down.qinv, out.down_p_inv_mod_q), copy(h.down.recip, out.down_recip);
        copy(h.down.blen, out.down_bit_length);
        copy(h.t1, out.pow_w), copy(h.t1p, out.pow_w_shoup), copy(h.t2, out.pow_2w), copy(h.t2p, out.pow_2w_shoup);
        copy(h.onep, out.one_shoup);
    }

    namespace
    {
        // convert_and_divide (centred) inside stacks of `limbs` limbs: the input base of `c` is limbs c.K .. c.K + c.L - 1
        // of every stack, its output base limbs 0 .. c.K - 1; out: T[stacks][c.K][N]
        template <typename T>
        void ks_ref_divide(const host::BcHostConsts& c, const T* x_host, T* out_host, int n_power, int stacks, int limbs)
        {
            const size_t n = size_t(1) << n_power;
            std::uint64_t x[BASECONV_MAX_COUNT], conv[BASECONV_MAX_COUNT];
            for (int s = 0; s < stacks; s++)
                for (size_t j = 0; j < n; j++)
                {
                    const T* src = x_host + static_cast<size_t>(s) * limbs * n + j;
                    for (int k = 0; k < c.L; k++)
                        x[k] = src[(c.K + k) * n];
                    host::bc_ref_convert<T>(c, x, true, conv);
                    for (int i = 0; i < c.K; i++)
                    {
                        const std::uint64_t q = c.p[i];
                        const std::uint64_t w = src[i * n] % q;
                        const std::uint64_t diff = w >= conv[i] ? w - conv[i] : w + (q - conv[i]);
                        out_host[(static_cast<size_t>(s) * c.K + i) * n + j] =
                            static_cast<T>(static_cast<U128>(diff) * c.qinv[i] % q);
                    }
                }
        }
    } // namespace

    template <typename T>
    void KeySwitchPlan<T>::reference_mod_up(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host,
                                            int p_count, int alpha, const T* in_host, T* a_host, int n_power, int count,
                                            BaseConvMode mode)
    {
        const KsHost h = ks_derive<T>(q_moduli_host, q_count, p_moduli_host, p_count, alpha);
        ks_check_mod_up<T>(h.L, h.M, h.D, in_host, a_host, n_power, count, mode);
        const size_t n = size_t(1) << n_power;
        const int L = h.L, M = h.M;
        std::uint64_t x[BASECONV_MAX_COUNT], conv[BASECONV_MAX_COUNT];
        for (int d = 0; d < h.D; d++)
            for (int r = 0; r < count; r++)
                for (size_t j = 0; j < n; j++)
                {
                    const T* src = in_host + static_cast<size_t>(r) * L * n + j;
                    T* dst = a_host + (static_cast<size_t>(d) * count + r) * M * n + j;
                    for (int i = h.lo(d); i < h.hi(d); i++)
                        x[i - h.lo(d)] = src[i * n];
                    host::bc_ref_convert<T>(h.up[d], x, mode == BaseConvMode::centred, conv);
                    for (int m = 0; m < M; m++)
                        dst[m * n] = (m >= h.lo(d) && m < h.hi(d)) ? static_cast<T>(src[m * n] % h.mod[m])
                                                                   : static_cast<T>(conv[ks_column(h, d, m)]);
                }
    }

    template <typename T>
    void KeySwitchPlan<T>::reference_mod_down(const Modulus<T>* q_moduli_host, int q_count,
                                              const Modulus<T>* p_moduli_host, int p_count, const T* x_host, T* out_host,
                                              int n_power, int stacks)
    {
        const KsHost h = ks_derive<T>(q_moduli_host, q_count, p_moduli_host, p_count, 1, false); // {p} -> {q} only
        ks_check_mod_down<T>(h.L, h.M, x_host, out_host, n_power, stacks);
        ks_ref_divide<T>(h.down, x_host, out_host, n_power, stacks, h.M);
    }

    template <typename T>
    void KeySwitchPlan<T>::reference_mod_down_rescale(const Modulus<T>* q_moduli_host, int q_count,
                                                      const Modulus<T>* p_moduli_host, int p_count, int rescale_limbs,
                                                      const T* x_host, T* out_host, int n_power, int stacks)
    {
        const KsHost h = ks_derive<T>(q_moduli_host, q_count, p_moduli_host, p_count, 1, false); // every pair is checked
        ks_check_rescale_limbs(h.L, rescale_limbs, 1);
        const int Lk = h.L - rescale_limbs;
        ks_check_mod_down<T>(Lk, h.M, x_host, out_host, n_power, stacks);
        std::vector<Modulus<T>> full(q_moduli_host, q_moduli_host + h.L);
        full.insert(full.end(), p_moduli_host, p_moduli_host + h.K);
        const host::BcHostConsts c = host::bc_derive<T>(full.data() + Lk, rescale_limbs + h.K, full.data(), Lk);
        ks_ref_divide<T>(c, x_host, out_host, n_power, stacks, h.M);
    }

    template <typename T>
    void KeySwitchPlan<T>::reference_rescale(const Modulus<T>* q_moduli_host, int q_count, int rescale_limbs,
                                             const T* x_host, T* out_host, int n_power, int stacks)
    {
        if (q_count < 1 || q_count > INNERPROD_MAX_MODULI)
            throw std::invalid_argument("Invalid q_count!");
        if (q_moduli_host == nullptr)
            throw std::invalid_argument("null pointer argument");
        ks_check_rescale_limbs(q_count, rescale_limbs, 1);
        const int Lk = q_count - rescale_limbs;
        // {dropped} -> {kept} checks the dropped pairwise and against every kept modulus; the kept among themselves here
        const host::BcHostConsts c = host::bc_derive<T>(q_moduli_host + Lk, rescale_limbs, q_moduli_host, Lk);
        for (int i = 0; i < Lk; i++)
            for (int o = i + 1; o < Lk; o++)
                if (std::__gcd(c.p[i], c.p[o]) != 1)
                    throw std::invalid_argument("Input base moduli are not pairwise coprime!");
        ks_check_mod_down<T>(Lk, q_count, x_host, out_host, n_power, stacks);
        ks_ref_divide<T>(c, x_host, out_host, n_power, stacks, q_count);
    }

    template class KeySwitchPlan<Data32>;
    template class KeySwitchPlan<Data64>;
} // namespace gpuntt
