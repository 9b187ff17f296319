// bfv_multiply.hip -- scale-invariant ciphertext multiplication (extension, include/gpuntt/rns/bfv_multiply.cuh): the
// three kernels of BfvMultiplyPlan<T> and the plan itself.
//
//   bfv_extend:       full[s][m] = in[s][m] mod q_m for m < L, and the centred conversion {q} -> {b} of the stack's L words
//                     into limbs L .. M-1 -- KeySwitchPlan::mod_up at a single digit, as a sibling of its kernel
//   bfv_tensor:       d0 = x0 y0, d1 = x0 y1 + x1 y0, d2 = x1 y1 modulo every modulus of the full base
//   bfv_scale_round:  out = round(t X / Q) in the base q from the M words of X: t X, the centred conversion {q} -> {b} with
//                     its division by Q, and the centred conversion {b} -> {q} of the result, in ONE pass over the stack
//
// The two conversion kernels keep the conventions of base_conversion.hip -- one lane owns one coefficient
// column, the y_i are parked in LDS at [i][lane], every constant is indexed by wave-uniform values only and is read through
// the constant address space -- and are made of its conversion unit: bc_z, bc_block_mac and bc_fold of
// base_conversion_internal.hpp, where the bounds are proved.
//
// bfv_scale_round.  The lane reads the M words of its column once.  First conversion: y_i = full_i * [t qhat_i^-1 mod q_i]
// -- t folded into the Shoup constant: the same canonical residue as ((t mod q_i) full_i mod q_i) * qhat_i^-1 mod q_i -- goes
// to LDS row i, v is formed as base_convert forms it, and the K outputs come BC_KB at a time: conv_j, then c_j = full_{L+j}
// scaled by t mod b_j, the difference as a congruent word, the product with Q^-1 mod b_j: r_j, step 2 of the definition.
// Each r_j becomes y'_j = r_j * [Bhat_j^-1 mod b_j] on the spot and goes to LDS row L + j, with its z' term summed
// for v'.  Second conversion: the L outputs of {b} -> {q} are accumulated over rows L .. M-1 and stored.  The K words r_j
// never reach memory.  LDS: M x 128 words per workgroup, 64 KiB at M = 64 with u64 -- mod_down's ceiling.
// A column tile is never split over workgroups: the second conversion needs every y'_j, so a split would recompute the
// whole first conversion in each part (whether small calls would gain from it is not measured).
//
// bfv_tensor is tensor_top's arithmetic (relinearize.hip) for three terms: IpAcc::mac and IpFold of
// inner_product_internal.hpp, the ONE copy of that arithmetic -- d1 is one exact two-term sum, folded once.  It may write
// d over x: every word is written by the lane that read it, after its loads.
//
// multiply_sum / multiply_relinearize_sum: the host side is here (sum_check, sum_product: the distinct operands by pointer
// equality, one slot of the operand region each); their kernel, bfv_tensor_sum, is in bfv_multiply_sum.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

#include "bfv_multiply_internal.hpp"
#include "bfv_multiply_sum_internal.hpp"
#include "decrypt_internal.hpp"
#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/bfv_multiply.cuh"
#include "launch.hpp"
#include "relinearize_internal.hpp"
#include "rns_call.hpp"

namespace gpuntt
{
    namespace kern
    {
        extern __shared__ __align__(16) unsigned char bfv_smem[]; // M (bfv_extend: L) rows of BC_NT words

        // in: T[stacks][L][N], full: T[stacks][M][N], M = L + K; total = stacks N columns.  grid: x = column tile
        template <typename T>
        __global__ __launch_bounds__(BC_NT) void bfv_extend(const T* __restrict__ in, T* __restrict__ full,
                                                            const T* __restrict__ consts, BcOffsets up, BfvOffsets ex,
                                                            int L, int K, int KP, int n_power, unsigned long long total)
        {
            const BcConsts<T> k(consts, up);
            const typename BcConsts<T>::CP onepq = (typename BcConsts<T>::CP) (consts) + ex.onepq;
            using W2 = typename RnsWide<T>::type;
            constexpr int W = static_cast<int>(8 * sizeof(T));
            T* ys = reinterpret_cast<T*>(bfv_smem) + threadIdx.x;

            const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * BC_NT + threadIdx.x;
            if (t >= total)
                return; // (no barrier below)
            const unsigned long long e = t >> n_power, col = t & ((1ull << n_power) - 1ull);
            const T* src = in + ((e * static_cast<unsigned>(L)) << n_power) + col;
            T* dst = full + ((e * static_cast<unsigned>(L + K)) << n_power) + col;

            W2 zsum = static_cast<W2>(1) << (W - 1);
#pragma unroll 4
            for (int i = 0; i < L; i++)
            {
                const T q = k.q[i];
                const T x = src[static_cast<unsigned long long>(i) << n_power];
                const T y = rns_shoup<T>(x, k.w[i], k.wp[i], q);
                ys[i * BC_NT] = y;
                // the canonical word: a conditional subtraction does not reduce a 64-bit word modulo a 20-bit q
                dst[static_cast<unsigned long long>(i) << n_power] = rns_shoup<T>(x, T(1), onepq[i], q);
                zsum += bc_z<T>(y, k.recip[i], k.shift[i]);
            }
            const T v = static_cast<T>(zsum >> W);

            dst += static_cast<unsigned long long>(L) << n_power;
            for (int j0 = 0; j0 < K; j0 += BC_KB)
            {
                W2 acc[BC_KB];
                T carry[BC_KB];
                bc_block_mac<T, true>(ys, BC_NT, k.matrix + j0, KP, L, v, k.negq + j0, acc, carry);
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    const int j = j0 + b;
                    if (j < K)
                        dst[static_cast<unsigned long long>(j) << n_power] = bc_fold<T>(acc[b], carry[b], k, j, k.p[j]);
                }
            }
        }

        // full: T[stacks][M][N], out: T[stacks][L][N]; total = stacks N columns.  grid: x = column tile.  up: the image of
        // {q} -> {b} (KP = K padded), down: the image of {b} -> {q} (LP = L padded)
        template <typename T>
        __global__ __launch_bounds__(BC_NT) void bfv_scale_round(const T* __restrict__ full, T* __restrict__ out,
                                                                 const T* __restrict__ consts, BcOffsets up,
                                                                 BcOffsets down, BfvOffsets ex, int L, int K, int KP,
                                                                 int LP, int n_power, unsigned long long total)
        {
            using CP = typename BcConsts<T>::CP;
            using W2 = typename RnsWide<T>::type;
            constexpr int W = static_cast<int>(8 * sizeof(T));
            const BcConsts<T> ku(consts, up), kd(consts, down);
            const CP wt = (CP) (consts) + ex.wt, wtp = (CP) (consts) + ex.wtp;
            const CP tb = (CP) (consts) + ex.tb, tbp = (CP) (consts) + ex.tbp;
            T* ys = reinterpret_cast<T*>(bfv_smem) + threadIdx.x; // y_i at row i < L, y'_j at row L + j
            T* y2s = ys + L * BC_NT;

            const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * BC_NT + threadIdx.x;
            if (t >= total)
                return; // (no barrier below)
            const unsigned long long e = t >> n_power, col = t & ((1ull << n_power) - 1ull);
            const T* src = full + ((e * static_cast<unsigned>(L + K)) << n_power) + col;

            // {q} -> {b} of t X: y_i with t folded into the constant
            W2 zsum = static_cast<W2>(1) << (W - 1);
#pragma unroll 4
            for (int i = 0; i < L; i++)
            {
                const T y = rns_shoup<T>(src[static_cast<unsigned long long>(i) << n_power], wt[i], wtp[i], ku.q[i]);
                ys[i * BC_NT] = y;
                zsum += bc_z<T>(y, ku.recip[i], ku.shift[i]);
            }
            const T v = static_cast<T>(zsum >> W);

            src += static_cast<unsigned long long>(L) << n_power;
            W2 zsum2 = static_cast<W2>(1) << (W - 1);
            for (int j0 = 0; j0 < K; j0 += BC_KB)
            {
                W2 acc[BC_KB];
                T carry[BC_KB];
                bc_block_mac<T, true>(ys, BC_NT, ku.matrix + j0, KP, L, v, ku.negq + j0, acc, carry);
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    const int j = j0 + b;
                    if (j < K)
                    {
                        const T p = ku.p[j];
                        const T conv = bc_fold<T>(acc[b], carry[b], ku, j, p);
                        // c_j = (t mod b_j) full_{L+j} mod b_j; c - conv as a word that is congruent to it
                        const T c = rns_shoup<T>(src[static_cast<unsigned long long>(j) << n_power], tb[j], tbp[j], p);
                        const T d = c >= conv ? c - conv : c + (p - conv);
                        const T r = rns_shoup<T>(d, ku.qinv[j], ku.qinvp[j], p); // step 2's word
                        const T y2 = rns_shoup<T>(r, kd.w[j], kd.wp[j], p);
                        y2s[j * BC_NT] = y2;
                        zsum2 += bc_z<T>(y2, kd.recip[j], kd.shift[j]);
                    }
                }
            }
            const T v2 = static_cast<T>(zsum2 >> W);

            // {b} -> {q} of r
            T* dst = out + ((e * static_cast<unsigned>(L)) << n_power) + col;
            for (int i0 = 0; i0 < L; i0 += BC_KB)
            {
                W2 acc[BC_KB];
                T carry[BC_KB];
                bc_block_mac<T, true>(y2s, BC_NT, kd.matrix + i0, LP, K, v2, kd.negq + i0, acc, carry);
#pragma unroll
                for (int b = 0; b < BC_KB; b++)
                {
                    const int i = i0 + b;
                    if (i < L)
                        dst[static_cast<unsigned long long>(i) << n_power] = bc_fold<T>(acc[b], carry[b], kd, i, kd.p[i]);
                }
            }
        }

        // grid: x = r * tiles + tile, y = m < M; xe, ye: T[2][count][M][N], d: T[3][count][M][N]; fold: the six arrays of M
        // words IpFold reads.  d may be xe's memory; ye may be xe (a squaring: two loads instead of four)
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void bfv_tensor(const T* xe, const T* ye, T* d, const T* __restrict__ fold_consts,
                                                            int count, int M, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, r = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long at =
                ((static_cast<unsigned long long>(r) * static_cast<unsigned>(M) + m) << n_power) + col;
            const unsigned long long comp = (static_cast<unsigned long long>(count) * static_cast<unsigned>(M)) << n_power;
            const Vec x0 = *reinterpret_cast<const Vec*>(xe + at);
            const Vec x1 = *reinterpret_cast<const Vec*>(xe + comp + at);
            Vec y0 = x0, y1 = x1;
            if (ye != xe) // uniform over the grid
            {
                y0 = *reinterpret_cast<const Vec*>(ye + at);
                y1 = *reinterpret_cast<const Vec*>(ye + comp + at);
            }
            const IpFold<T> fold(fold_consts, M, m);
            Vec o0, o1, o2;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                IpAcc<T> s0{T(0), T(0), 0u}, s1{T(0), T(0), 0u}, s2{T(0), T(0), 0u};
                s0.mac(x0.x[v], y0.x[v]);
                s1.mac(x0.x[v], y1.x[v]);
                s1.mac(x1.x[v], y0.x[v]);
                s2.mac(x1.x[v], y1.x[v]);
                o0.x[v] = fold.reduce(fold.sum(s0)); // each sum is below 3 q < 2^W
                o1.x[v] = fold.reduce(fold.sum(s1));
                o2.x[v] = fold.reduce(fold.sum(s2));
            }
            *reinterpret_cast<Vec*>(d + at) = o0;
            *reinterpret_cast<Vec*>(d + comp + at) = o1;
            *reinterpret_cast<Vec*>(d + 2 * comp + at) = o2;
        }
    } // namespace kern

    namespace
    {
        using U128 = unsigned __int128;

        // rns_host.hpp and, for bc_padded, base_conversion_internal.hpp
        using host::bc_padded;
        using host::column_tiles;
        using host::need_aligned_scratch;
        using host::need_int_batch;
        using host::need_pointers;
        using host::refuse_overlap;
        using host::rns_align;
        using host::rns_check_n_power;
        using host::words_at;

        void bfv_check_counts(int L, int K)
        {
            if (L < 1 || L > BASECONV_MAX_COUNT)
                throw std::invalid_argument("Invalid q_count!");
            if (K < 1 || K > BASECONV_MAX_COUNT || L + K > BASECONV_MAX_COUNT)
                throw std::invalid_argument("Invalid b_count!");
        }

        // a product of words in exact integers, little-endian 64-bit limbs: the size check B >= 2 t N Q
        using Big = std::vector<std::uint64_t>;
        void big_mul(Big& a, std::uint64_t f)
        {
            std::uint64_t carry = 0;
            for (std::uint64_t& w : a)
            {
                const U128 p = static_cast<U128>(w) * f + carry;
                w = static_cast<std::uint64_t>(p);
                carry = static_cast<std::uint64_t>(p >> 64);
            }
            if (carry != 0)
                a.push_back(carry);
        }
        bool big_less(const Big& a, const Big& b) // no leading zero limbs on either side
        {
            if (a.size() != b.size())
                return a.size() < b.size();
            for (size_t i = a.size(); i-- > 0;)
                if (a[i] != b[i])
                    return a[i] < b[i];
            return false;
        }

        // everything the host derives for one (q-base, auxiliary base, t), in exact integers
        struct BfvHost
        {
            int L = 0, K = 0, M = 0;
            int max_terms = 1;                                 // min(BFV_MAX_TERMS, floor(B / (2 t N Q)))
            std::vector<std::uint64_t> mod;                    // [M] the full base
            host::BcHostConsts up, down;                       // {q} -> {b}, {b} -> {q}
            std::vector<std::uint64_t> tm, tmp;                // [M] t mod m_m and its Shoup companion
            std::vector<std::uint64_t> wt, wtp;                // [L] (t qhat_i^-1) mod q_i and its companion
            std::vector<std::uint64_t> t1, t1p, t2, t2p, onep; // [M] the fold constants of bfv_tensor
        };

        // n_power < 0: without the size check (the host references are defined for any bases)
        template <typename T>
        BfvHost bfv_derive(const Modulus<T>* qm, int L, const Modulus<T>* bm, int K, std::uint64_t t, int n_power)
        {
            constexpr int W = static_cast<int>(8 * sizeof(T));
            bfv_check_counts(L, K);
            if (qm == nullptr || bm == nullptr)
                throw std::invalid_argument("null pointer argument");
            if (t < 2)
                throw std::invalid_argument("Invalid plaintext modulus!");
            BfvHost h;
            h.L = L, h.K = K, h.M = L + K;
            // {q} -> {b} checks the q pairwise and every q against every b, {b} -> {q} the b pairwise; both check every
            // modulus ("Invalid modulus!")
            h.up = host::bc_derive<T>(qm, L, bm, K);
            h.down = host::bc_derive<T>(bm, K, qm, L);
            h.mod = h.up.q;
            h.mod.insert(h.mod.end(), h.up.p.begin(), h.up.p.end());
            if (n_power >= 0)
            {
                rns_check_n_power(n_power);
                Big B{1}, need{2};
                for (int j = 0; j < K; j++)
                    big_mul(B, h.mod[L + j]);
                big_mul(need, t);
                big_mul(need, std::uint64_t(1) << n_power);
                for (int i = 0; i < L; i++)
                    big_mul(need, h.mod[i]);
                if (big_less(B, need))
                    throw std::invalid_argument("Auxiliary base too small!");
                // the largest terms <= BFV_MAX_TERMS with B >= 2 terms t N Q: what multiply_sum may add up
                for (int terms = 2; terms <= BFV_MAX_TERMS; terms++)
                {
                    Big scaled = need;
                    big_mul(scaled, static_cast<std::uint64_t>(terms));
                    if (big_less(B, scaled))
                        break;
                    h.max_terms = terms;
                }
            }
            for (int m = 0; m < h.M; m++)
            {
                const std::uint64_t q = h.mod[m];
                auto shoup = [&](std::uint64_t v) { return static_cast<std::uint64_t>((static_cast<U128>(v) << W) / q); };
                const std::uint64_t tq = t % q;
                const host::RnsFoldConsts f = host::rns_fold_consts(q, W);
                h.tm.push_back(tq), h.tmp.push_back(shoup(tq));
                h.t1.push_back(f.t1), h.t1p.push_back(f.t1p), h.t2.push_back(f.t2), h.t2p.push_back(f.t2p);
                h.onep.push_back(f.onep);
                if (m < L)
                {
                    const std::uint64_t w = static_cast<std::uint64_t>(static_cast<U128>(tq) * h.up.w[m] % q);
                    h.wt.push_back(w), h.wtp.push_back(shoup(w));
                }
            }
            return h;
        }

        struct BfvLayout // the workspace, in bytes; the constants are the run [up, ntt_q_i)
        {
            size_t up, down, extra, fold, ntt_q_i, ntt_q_f, ntt_full_f, ntt_full_i, total;
        };
        template <typename T> BfvLayout bfv_layout(int L, int K, int n_power)
        {
            bfv_check_counts(L, K);
            rns_check_n_power(n_power);
            const int M = L + K;
            BfvLayout w{};
            size_t at = 0;
            auto take = [&](size_t bytes) {
                const size_t first = at;
                at += rns_align(bytes);
                return first;
            };
            w.up = take(host::bc_image_words(L, K) * sizeof(T));
            w.down = take(host::bc_image_words(K, L) * sizeof(T));
            w.extra = take((3 * static_cast<size_t>(L) + 2 * static_cast<size_t>(bc_padded(K))) * sizeof(T));
            w.fold = take(6 * static_cast<size_t>(M) * sizeof(T));
            w.ntt_q_i = take(NTTPlan<T>::workspace_bytes(n_power, L));
            w.ntt_q_f = take(NTTPlan<T>::workspace_bytes(n_power, L));
            w.ntt_full_f = take(NTTPlan<T>::workspace_bytes(n_power, M));
            w.ntt_full_i = take(NTTPlan<T>::workspace_bytes(n_power, M));
            w.total = at;
            return w;
        }

        // BcOffsets of an image that starts `words` words into the run of constants
        kern::BcOffsets bfv_shift(kern::BcOffsets o, size_t words)
        {
            const unsigned s = static_cast<unsigned>(words);
            return kern::BcOffsets{o.q + s,     o.w + s,  o.wp + s,  o.recip + s, o.shift + s,
                                   o.matrix + s, o.p + s,  o.negq + s, o.qinv + s,  o.qinvp + s,
                                   o.t1 + s,    o.t1p + s, o.t2 + s,  o.t2p + s,   o.onep + s};
        }

        struct BfvScratch // the caller's scratch, in bytes
        {
            size_t e, coeff, total; // e: T[4][count][M][N]; coeff: T[2][count][L][N]
        };
        template <typename T> BfvScratch bfv_scratch(int L, int M, int n_power, int count)
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            const size_t poly = (static_cast<size_t>(count) << n_power) * sizeof(T);
            BfvScratch s{};
            s.e = 0;
            s.coeff = s.e + rns_align(poly * M * 4);
            s.total = s.coeff + rns_align(poly * L * 2);
            return s;
        }

        // multiply_sum's scratch: the operand region grows to max(operands, 2) slots of T[2][count][M][N]; operands = 2
        // is multiply's layout
        template <typename T> BfvScratch bfv_sum_scratch(int L, int M, int n_power, int count, int operands)
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (operands < 1 || operands > 2 * BFV_MAX_TERMS)
                throw std::invalid_argument("Invalid operands!");
            const size_t poly = (static_cast<size_t>(count) << n_power) * sizeof(T);
            BfvScratch s{};
            s.e = 0;
            s.coeff = s.e + rns_align(poly * M * 2 * static_cast<size_t>(std::max(operands, 2)));
            s.total = s.coeff + rns_align(poly * L * 2);
            return s;
        }

        // the argument checks of extend / scale_round (device or host arrays alike): `narrow` limbs per stack at a,
        // `wide` at b
        template <typename T>
        void bfv_check_stacks(int narrow, int wide, const T* a, const T* b, int n_power, int stacks, const char* what)
        {
            rns_check_n_power(n_power);
            if (stacks < 0)
                throw std::invalid_argument("Invalid stacks!");
            need_pointers(a, b);
            const std::uint64_t cols = static_cast<std::uint64_t>(stacks) << n_power;
            if (stacks > 0)
                refuse_overlap({{a, cols * narrow * sizeof(T)}}, {{b, cols * wide * sizeof(T)}}, what);
        }

        template <typename T, int V>
        void bfv_tensor_as(const T* xe, const T* ye, T* d, const T* fold, int count, int M, int n_power, bool enqueue,
                           hipStream_t stream)
        {
            const host::RelinGrid g = host::relin_grid(n_power, V, static_cast<unsigned long long>(count));
            if (!enqueue)
                return;
            GPUNTT_LAUNCH((kern::bfv_tensor<T, V>), dim3(g.blocks, static_cast<unsigned>(M)), dim3(g.nt), 0, stream, xe,
                          ye, d, fold, count, M, n_power, g.tiles);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }
        // enqueue false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void bfv_tensor_launch(const T* xe, const T* ye, T* d, const T* fold, int count, int M, int n_power, bool enqueue,
                               hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (host::relin_wide<T>(n_power, {xe, ye, d}))
                bfv_tensor_as<T, VW>(xe, ye, d, fold, count, M, n_power, enqueue, stream);
            else
                bfv_tensor_as<T, 1>(xe, ye, d, fold, count, M, n_power, enqueue, stream);
        }
    } // namespace

    template <typename T> struct BfvMultiplyPlan<T>::Impl
    {
        int L = 0, K = 0, M = 0, n = 0, max_terms = 1;
        T t = 0;
        std::vector<Modulus<T>> moduli; // [M] the full base as the caller gave it: modulus(m)
        ReductionPolynomial poly = ReductionPolynomial::X_N_plus;
        char* ws = nullptr;
        bool owns = false;
        BfvLayout lay{};
        kern::BcOffsets up_off{}, down_off{};
        kern::BfvOffsets ex_off{};
        std::unique_ptr<NTTPlan<T>> ntt_q_i, ntt_q_f, ntt_full_f, ntt_full_i;
        // scale_message / decode / decrypt (decrypt.hip): the constants of t travel as kernel arguments, derived on the
        // host at construction -- no word of the workspace, no launch
        bool decode_ok = false, scale_ok = false; // is t usable by decode / by scale_message ("Plaintext modulus ...")
        kern::BfvDecodeArgs<T> decode_args{};
        kern::BfvScaleArgs<T> scale_args{};

        const T* consts() const { return reinterpret_cast<const T*>(ws + lay.up); }
        const T* fold() const { return reinterpret_cast<const T*>(ws + lay.fold); }

        void extend(const T* in, T* full, int stacks, hipStream_t stream) const
        {
            bfv_check_stacks<T>(L, M, in, full, n, stacks, "extend input and output overlap!");
            if (stacks == 0)
                return;
            const unsigned long long total = static_cast<unsigned long long>(stacks) << n;
            const unsigned tiles = static_cast<unsigned>(column_tiles(total, kern::BC_NT, "Invalid stacks!"));
            GPUNTT_LAUNCH((kern::bfv_extend<T>), dim3(tiles), dim3(kern::BC_NT),
                          static_cast<size_t>(L) * kern::BC_NT * sizeof(T), stream, in, full, consts(), up_off, ex_off, L,
                          K, bc_padded(K), n, total);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        void scale_round(const T* full, T* out, int stacks, hipStream_t stream) const
        {
            bfv_check_stacks<T>(L, M, out, full, n, stacks, "scale_round input and output overlap!");
            if (stacks == 0)
                return;
            const unsigned long long total = static_cast<unsigned long long>(stacks) << n;
            const unsigned tiles = static_cast<unsigned>(column_tiles(total, kern::BC_NT, "Invalid stacks!"));
            GPUNTT_LAUNCH((kern::bfv_scale_round<T>), dim3(tiles), dim3(kern::BC_NT),
                          static_cast<size_t>(M) * kern::BC_NT * sizeof(T), stream, full, out, consts(), up_off, down_off,
                          ex_off, L, K, bc_padded(K), bc_padded(L), n, total);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        // message: T[count][N] -> out: T[count][L][N], round(Q m / t) in the q-base
        void scale_message(const T* message, T* out, int count, bool to_ntt, hipStream_t stream) const
        {
            if (!scale_ok)
                throw std::invalid_argument("Plaintext modulus not usable here!");
            if (to_ntt && !ntt_q_f)
                throw std::invalid_argument("The plan was built without transform tables!");
            if (count < 0 || static_cast<unsigned long long>(count) * static_cast<unsigned>(L) > 0x7FFFFFFFull)
                throw std::invalid_argument("Invalid count!");
            need_pointers(message, out);
            if (count == 0)
                return;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            refuse_overlap({{out, cols * L * sizeof(T)}}, {{message, cols * sizeof(T)}},
                           "scale_message input and output overlap!");
            host::bfv_scale_message_launch<T>(message, out, fold(), scale_args, count, L, n, false, stream);
            host::bfv_scale_message_launch<T>(message, out, fold(), scale_args, count, L, n, true, stream);
            if (to_ntt)
                ntt_q_f->execute(out, out, count * L, stream);
        }

        // every refusal of decode; returns false when stacks is 0 and nothing is to be launched
        size_t decode_partials(int stacks) const // the partial maxima of the two-launch decode: T[stacks][tiles]
        {
            if (stacks < 0)
                throw std::invalid_argument("Invalid stacks!");
            return rns_align(host::decode_partial_words(stacks, n) * sizeof(T));
        }

        bool decode_check(const T* x, const T* message, const T* noise_max, int stacks, const void* partials = nullptr) const
        {
            if (!decode_ok)
                throw std::invalid_argument("Plaintext modulus not usable here!");
            if (stacks < 0)
                throw std::invalid_argument("Invalid stacks!");
            need_pointers(x, message);
            if (stacks == 0)
                return false;
            const std::uint64_t cols = static_cast<std::uint64_t>(stacks) << n;
            const std::uint64_t x_bytes = cols * L * sizeof(T), m_bytes = cols * sizeof(T);
            const std::uint64_t n_bytes = static_cast<std::uint64_t>(stacks) * sizeof(T);
            const char* overlap = "decode input and output overlap!";
            refuse_overlap({{message, m_bytes}, {noise_max, n_bytes}}, {{x, x_bytes}}, overlap);
            refuse_overlap({{message, m_bytes}}, {{noise_max, n_bytes}}, overlap);
            if (partials != nullptr && noise_max != nullptr)
            {
                if (reinterpret_cast<uintptr_t>(partials) % sizeof(T) != 0)
                    throw std::invalid_argument(overlap);
                refuse_overlap({{partials, host::decode_partial_words(stacks, n) * sizeof(T)}},
                               {{x, x_bytes}, {message, m_bytes}, {noise_max, n_bytes}}, overlap);
            }
            // the grid limit, with the loader the launch will choose
            try
            {
                host::bfv_decode_launch<T>(x, const_cast<T*>(message), nullptr, nullptr, consts(), up_off, decode_args,
                                           stacks, L, n, false, nullptr);
            }
            catch (const std::invalid_argument&)
            {
                throw std::invalid_argument("Invalid stacks!"); // the grid's own words name a count
            }
            return true;
        }
        // partials == nullptr: the memset of noise_max and ONE launch with the atomic merge; otherwise two launches
        void decode_run(const T* x, T* message, T* noise_max, int stacks, hipStream_t stream, void* partials = nullptr) const
        {
            if (noise_max != nullptr && partials == nullptr)
                GPUNTT_HIP_CHECK(hipMemsetAsync(noise_max, 0, static_cast<size_t>(stacks) * sizeof(T), stream));
            host::bfv_decode_launch<T>(x, message, noise_max, static_cast<T*>(partials), consts(), up_off, decode_args,
                                       stacks, L, n, true, stream);
        }
        // x: T[stacks][L][N] in coefficient form -> message: T[stacks][N], noise_max: T[stacks] or nullptr
        void decode(const T* x, T* message, T* noise_max, int stacks, hipStream_t stream, void* partials) const
        {
            if (decode_check(x, message, noise_max, stacks, partials))
                decode_run(x, message, noise_max, stacks, stream, partials);
        }

        size_t decrypt_scratch(int count) const // the phase in coefficient form: T[count][L][N]
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            return rns_align(((static_cast<size_t>(count) * L) << n) * sizeof(T));
        }

        // the calls that hand their q-base to a key-switching plan: both plans have their transforms and agree in the
        // q-base, the ring and the reduction polynomial
        void need_matching(const KeySwitchPlan<T>& ks) const
        {
            bool match = ntt_full_f && ks.has_transforms() && ks.q_count() == L && ks.n_power() == n &&
                         ks.reduction_poly() == poly;
            for (int m = 0; match && m < L; m++)
                match = ks.modulus(m).value == moduli[m].value;
            if (!match)
                throw std::invalid_argument("The key-switching plan does not match!");
        }

        void decrypt(const T* ct, const KeySwitchPlan<T>& ks, const T* s, T* message, T* noise_max, int count,
                     int components, bool input_ntt, void* scratch, void* ks_scratch, hipStream_t stream) const
        {
            need_matching(ks);
            (void) decrypt_scratch(count); // checks count
            need_pointers(scratch);
            need_aligned_scratch(scratch);
            T* x = static_cast<T*>(scratch);
            const bool work = decode_check(x, message, noise_max, count);
            const size_t ks_bytes = ks.phase_scratch_bytes(count, components, input_ntt); // checks components
            if (work && ct != nullptr && s != nullptr)
            {
                const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
                const std::uint64_t ct_bytes = cols * L * components * sizeof(T), m_bytes = cols * sizeof(T);
                const std::uint64_t s_bytes = (static_cast<std::uint64_t>(L) << n) * sizeof(T);
                const std::uint64_t n_bytes = static_cast<std::uint64_t>(count) * sizeof(T);
                refuse_overlap({{message, m_bytes}, {noise_max, n_bytes}},
                               {{ct, ct_bytes}, {s, s_bytes}, {ks_bytes != 0 ? ks_scratch : nullptr, ks_bytes}},
                               "out or the scratch overlaps an operand!");
            }
            // the phase refuses the rest before its first launch: null ct or s, its own scratch, the overlaps of the
            // coefficient region with ct, s and its scratch
            ks.phase(ct, s, x, count, components, input_ntt, false, ks_scratch, stream);
            if (work)
                decode_run(x, message, noise_max, count, stream);
        }

        // The tail product_check and sum_check share: the scratch (of `total` bytes) and out (`comps` components) against
        // the U operands at ops, and the limits of the calls -- `widest` count M is the widest batch of a transform.
        // Returns false when count is 0 and nothing is to be launched
        bool operands_check(const T* const* ops, int U, const T* out, int comps, int count, const void* scratch,
                            size_t total, unsigned long long widest) const
        {
            need_aligned_scratch(scratch);
            if (count == 0)
                return false;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t ct_bytes = cols * L * 2 * sizeof(T), out_bytes = cols * L * comps * sizeof(T);
            for (int u = 0; u < U; u++)
            {
                const char* operand = "out or the scratch overlaps an operand!";
                refuse_overlap({{scratch, total}}, {{ops[u], ct_bytes}}, operand);
                // out may be exactly one operand: the last read of every operand (bfv_extend, or the INTT before it)
                // precedes bfv_scale_round's first write on the stream.  Any other overlap is refused
                refuse_overlap({{out, out_bytes}}, {{ops[u], ct_bytes, true}}, operand);
            }
            refuse_overlap({{out, out_bytes}}, {{scratch, total}}, "The scratch overlaps out!");
            // every limit before the first launch: the batches of the transforms are ints, the grids as the launches check
            need_int_batch(widest * static_cast<unsigned>(count) * static_cast<unsigned>(M), "Invalid count!");
            (void) column_tiles((3ull * static_cast<unsigned>(count)) << n, kern::BC_NT, "Invalid stacks!");
            return true;
        }

        // What multiply and multiply_relinearize share up to the first launch: every refusal of multiply, with `comps`
        // components at out.  Returns false when count is 0 and nothing is to be launched
        bool product_check(const T* x, const T* y, const T* out, int comps, int count, void* scratch) const
        {
            if (!ntt_full_f)
                throw std::invalid_argument("The plan was built without transform tables!");
            const BfvScratch s = bfv_scratch<T>(L, M, n, count); // checks count
            need_pointers(x, y, out, scratch);
            const T* const ops[] = {x, y};
            if (!operands_check(ops, 2, out, comps, count, scratch, s.total, 4))
                return false;
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const bool square = x == y;
            T* e = words_at<T>(scratch, s.e);
            bfv_tensor_launch<T>(e, square ? e : e + cols * M * 2, e, fold(), count, M, n, false, nullptr);
            return true;
        }

        // steps 1 to 5 of multiply: the three tensor components in coefficient form over the full base, T[3][count][M][N]
        // at the start of the scratch
        T* product(const T* x, const T* y, int count, bool input_ntt, void* scratch, hipStream_t stream) const
        {
            const BfvScratch s = bfv_scratch<T>(L, M, n, count);
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const bool square = x == y;
            T* e = words_at<T>(scratch, s.e);
            T* coeff = words_at<T>(scratch, s.coeff);
            T* xe = e;
            T* ye = square ? e : e + cols * M * 2;
            auto bring = [&](const T* op, T* full) { // steps 1 and 2 for one operand
                if (input_ntt)
                    ntt_q_i->execute(op, coeff, 2 * count * L, stream);
                extend(input_ntt ? coeff : op, full, 2 * count, stream);
            };
            bring(x, xe);
            if (!square) // a squaring: y is x, extended once
                bring(y, ye);
            ntt_full_f->execute(e, e, (square ? 2 : 4) * count * M, stream);
            bfv_tensor_launch<T>(xe, ye, e, fold(), count, M, n, true, stream);
            ntt_full_i->execute(e, e, 3 * count * M, stream);
            return e;
        }

        void multiply(const T* x, const T* y, T* out, int count, bool input_ntt, bool output_ntt, void* scratch,
                      hipStream_t stream) const
        {
            if (!product_check(x, y, out, 3, count, scratch))
                return;
            const T* e = product(x, y, count, input_ntt, scratch, stream);
            scale_round(e, out, 3 * count, stream);
            if (output_ntt)
                ntt_q_f->execute(out, out, 3 * count * L, stream);
        }

        // What multiply_relinearize and multiply_relinearize_sum refuse before the product's own checks; returns the
        // bytes of the key-switching plan's scratch
        size_t relin_head(const KeySwitchPlan<T>& ks, const T* key, int count, const void* ks_scratch) const
        {
            need_matching(ks);
            need_pointers(key, ks_scratch);
            const size_t ks_bytes = ks.scratch_bytes(count, 2); // checks count
            need_aligned_scratch(ks_scratch);
            return ks_bytes;
        }

        // ... and after them: the key and the key-switching plan's scratch against the U operands at ops, out and the
        // scratch, and the limits of relinearize's coefficient path, before the first launch: the batch of its widest
        // transform is an int, and its grids (mod_up, the inner product, mod_down_add) launch at most
        // 2 * count * max(N, 256) work-items
        void relin_check(const T* const* ops, int U, const KeySwitchPlan<T>& ks, const T* key, const T* out, int count,
                         const void* scratch, size_t total, const void* ks_scratch, size_t ks_bytes) const
        {
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            const std::uint64_t ct_bytes = cols * L * 2 * sizeof(T);
            const std::uint64_t key_bytes =
                ((static_cast<std::uint64_t>(ks.digits()) * 2 * ks.key_mod_count()) << n) * sizeof(T);
            const char* operand = "out or the scratch overlaps an operand!";
            refuse_overlap({{ks_scratch, ks_bytes}, {scratch, total}, {out, ct_bytes}}, {{key, key_bytes}}, operand);
            for (int u = 0; u < U; u++)
                refuse_overlap({{ks_scratch, ks_bytes}, {key, key_bytes}}, {{ops[u], ct_bytes}}, operand);
            refuse_overlap({{ks_scratch, ks_bytes}}, {{out, ct_bytes}, {scratch, total}}, "The scratch overlaps out!");
            const unsigned long long ks_m = static_cast<unsigned>(L + ks.p_count());
            need_int_batch(static_cast<unsigned long long>(ks.digits()) * static_cast<unsigned>(count) * ks_m,
                           "Invalid count!");
            if (2ull * static_cast<unsigned>(count) * ((1ull << n) > 256ull ? (1ull << n) : 256ull) > 0xFFFFFFFFull)
                throw std::invalid_argument("Invalid count!");
        }

        // the three tensor components at e, divided and rounded: the low ones straight into out, the top one into the
        // coeff region of the scratch (dead since bfv_extend, and T[count][L][N] fits its T[2][count][L][N]); then the
        // key switch of the top one
        void relin_tail(const T* e, const KeySwitchPlan<T>& ks, const T* key, T* out, int count, bool output_ntt, T* top,
                        void* ks_scratch, hipStream_t stream) const
        {
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            scale_round(e, out, 2 * count, stream);
            scale_round(e + 2 * cols * M, top, count, stream);
            ks.relinearize(out, top, key, out, count, false, output_ntt, ks_scratch, stream);
        }

        void multiply_relinearize(const T* x, const T* y, const KeySwitchPlan<T>& ks, const T* key, T* out, int count,
                                  bool input_ntt, bool output_ntt, void* scratch, void* ks_scratch,
                                  hipStream_t stream) const
        {
            const size_t ks_bytes = relin_head(ks, key, count, ks_scratch);
            if (!product_check(x, y, out, 2, count, scratch))
                return;
            const BfvScratch s = bfv_scratch<T>(L, M, n, count);
            const T* const ops[] = {x, y};
            relin_check(ops, 2, ks, key, out, count, scratch, s.total, ks_scratch, ks_bytes);
            const T* e = product(x, y, count, input_ntt, scratch, stream);
            relin_tail(e, ks, key, out, count, output_ntt, words_at<T>(scratch, s.coeff), ks_scratch, stream);
        }

        // one multiply_sum call as the host sees it: the U distinct operand pointers in order of first appearance (x_0
        // is slot 0) and the two slots of every term
        struct SumCall
        {
            int U = 0;
            const T* op[2 * BFV_MAX_TERMS];
            kern::BfvSumArgs args;
        };

        // What multiply_sum and multiply_relinearize_sum share up to the first launch: every refusal of multiply_sum,
        // with `comps` components at out.  Returns false when count is 0 and nothing is to be launched
        bool sum_check(const T* const* xs, const T* const* ys, int terms, const T* out, int comps, int count,
                       void* scratch, SumCall& call) const
        {
            if (!ntt_full_f)
                throw std::invalid_argument("The plan was built without transform tables!");
            if (terms < 1 || terms > BFV_MAX_TERMS)
                throw std::invalid_argument("Invalid terms!");
            if (terms > max_terms)
                throw std::invalid_argument("Auxiliary base too small for these terms!");
            need_pointers(xs, ys, out, scratch);
            call.U = 0;
            call.args = kern::BfvSumArgs{};
            call.args.terms = terms;
            auto slot_of = [&](const T* p) {
                need_pointers(p);
                for (int s = 0; s < call.U; s++)
                    if (call.op[s] == p)
                        return static_cast<unsigned char>(s);
                call.op[call.U] = p;
                return static_cast<unsigned char>(call.U++);
            };
            for (int i = 0; i < terms; i++)
            {
                call.args.x_slot[i] = slot_of(xs[i]);
                call.args.y_slot[i] = slot_of(ys[i]);
            }
            const BfvScratch s = bfv_sum_scratch<T>(L, M, n, count, call.U); // checks count
            // the widest transform batch is 2 U count M (3 count M for U = 1)
            if (!operands_check(call.op, call.U, out, comps, count, scratch, s.total, std::max(2 * call.U, 3)))
                return false;
            T* e = words_at<T>(scratch, s.e);
            host::bfv_tensor_sum_launch<T>(e, fold(), call.args, count, M, n, false, nullptr);
            return true;
        }

        // steps 1 and 2 of multiply_sum and the one inverse transform: T[3][count][M][N] in coefficient form at the start
        // of the scratch
        T* sum_product(const SumCall& call, int count, bool input_ntt, void* scratch, hipStream_t stream) const
        {
            const BfvScratch s = bfv_sum_scratch<T>(L, M, n, count, call.U);
            const std::uint64_t cols = static_cast<std::uint64_t>(count) << n;
            T* e = words_at<T>(scratch, s.e);
            T* coeff = words_at<T>(scratch, s.coeff);
            for (int u = 0; u < call.U; u++) // the coefficient region is reused in stream order
            {
                if (input_ntt)
                    ntt_q_i->execute(call.op[u], coeff, 2 * count * L, stream);
                extend(input_ntt ? coeff : call.op[u], e + cols * M * 2 * static_cast<unsigned>(u), 2 * count, stream);
            }
            ntt_full_f->execute(e, e, 2 * call.U * count * M, stream);
            host::bfv_tensor_sum_launch<T>(e, fold(), call.args, count, M, n, true, stream);
            ntt_full_i->execute(e, e, 3 * count * M, stream);
            return e;
        }

        void multiply_sum(const T* const* xs, const T* const* ys, int terms, T* out, int count, bool input_ntt,
                          bool output_ntt, void* scratch, hipStream_t stream) const
        {
            SumCall call;
            if (!sum_check(xs, ys, terms, out, 3, count, scratch, call))
                return;
            const T* e = sum_product(call, count, input_ntt, scratch, stream);
            scale_round(e, out, 3 * count, stream);
            if (output_ntt)
                ntt_q_f->execute(out, out, 3 * count * L, stream);
        }

        void multiply_relinearize_sum(const T* const* xs, const T* const* ys, int terms, const KeySwitchPlan<T>& ks,
                                      const T* key, T* out, int count, bool input_ntt, bool output_ntt, void* scratch,
                                      void* ks_scratch, hipStream_t stream) const
        {
            const size_t ks_bytes = relin_head(ks, key, count, ks_scratch);
            SumCall call;
            if (!sum_check(xs, ys, terms, out, 2, count, scratch, call))
                return;
            const BfvScratch s = bfv_sum_scratch<T>(L, M, n, count, call.U);
            relin_check(call.op, call.U, ks, key, out, count, scratch, s.total, ks_scratch, ks_bytes);
            const T* e = sum_product(call, count, input_ntt, scratch, stream);
            relin_tail(e, ks, key, out, count, output_ntt, words_at<T>(scratch, s.coeff), ks_scratch, stream);
        }
    };

    template <typename T> size_t BfvMultiplyPlan<T>::workspace_bytes(int q_count, int b_count, int n_power)
    {
        return bfv_layout<T>(q_count, b_count, n_power).total;
    }

    template <typename T> size_t BfvMultiplyPlan<T>::scratch_bytes(int q_count, int b_count, int n_power, int count)
    {
        bfv_check_counts(q_count, b_count);
        rns_check_n_power(n_power);
        return bfv_scratch<T>(q_count, q_count + b_count, n_power, count).total;
    }

    template <typename T>
    BfvMultiplyPlan<T>::BfvMultiplyPlan(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host,
                                        int b_count, T plain_modulus, int n_power, const Root<T>* forward_table_device,
                                        const Root<T>* inverse_table_device, const Ninverse<T>* mod_inverse_host,
                                        ReductionPolynomial reduction_poly, int batch_hint, stream_t stream,
                                        void* workspace_device)
        : p_(nullptr)
    {
        bfv_check_counts(q_count, b_count);
        rns_check_n_power(n_power);
        const BfvHost h = bfv_derive<T>(q_moduli_host, q_count, b_moduli_host, b_count, plain_modulus, n_power);
        const BfvLayout lay = bfv_layout<T>(h.L, h.K, n_power);
        const bool transforms = forward_table_device != nullptr || inverse_table_device != nullptr;
        if (transforms && (forward_table_device == nullptr || inverse_table_device == nullptr || mod_inverse_host == nullptr))
            throw std::invalid_argument("null pointer argument");
        std::unique_ptr<Impl> p(new Impl);
        p->L = h.L, p->K = h.K, p->M = h.M, p->n = n_power, p->t = plain_modulus, p->lay = lay;
        p->poly = reduction_poly, p->max_terms = h.max_terms;

        // the run of constants: the two images, the plan's own arrays, the fold image -- one host buffer, one copy
        const int L = h.L, KP = bc_padded(h.K);
        std::vector<T> run((lay.ntt_q_i - lay.up) / sizeof(T), T(0));
        kern::BcOffsets up_rel{}, down_rel{};
        const std::vector<T> up_img = host::bc_image<T>(h.up, up_rel), down_img = host::bc_image<T>(h.down, down_rel);
        const size_t o_down = (lay.down - lay.up) / sizeof(T), o_extra = (lay.extra - lay.up) / sizeof(T);
        const size_t o_fold = (lay.fold - lay.up) / sizeof(T);
        std::copy(up_img.begin(), up_img.end(), run.begin());
        std::copy(down_img.begin(), down_img.end(), run.begin() + o_down);
        p->up_off = up_rel, p->down_off = bfv_shift(down_rel, o_down);
        auto u = [](size_t v) { return static_cast<unsigned>(v); };
        p->ex_off = kern::BfvOffsets{u(o_extra), u(o_extra + L), u(o_extra + 2 * L), u(o_extra + 3 * L),
                                     u(o_extra + 3 * L + KP)};
        for (int i = 0; i < L; i++)
        {
            run[p->ex_off.wt + i] = static_cast<T>(h.wt[i]), run[p->ex_off.wtp + i] = static_cast<T>(h.wtp[i]);
            run[p->ex_off.onepq + i] = static_cast<T>(h.onep[i]);
        }
        for (int j = 0; j < h.K; j++)
        {
            run[p->ex_off.tb + j] = static_cast<T>(h.tm[L + j]), run[p->ex_off.tbp + j] = static_cast<T>(h.tmp[L + j]);
        }
        {
            size_t at = o_fold;
            for (const std::vector<std::uint64_t>* v : {&h.mod, &h.t1, &h.t1p, &h.t2, &h.t2p, &h.onep})
                for (std::uint64_t w : *v)
                    run[at++] = static_cast<T>(w);
        }
        std::vector<Modulus<T>> full(q_moduli_host, q_moduli_host + h.L);
        full.insert(full.end(), b_moduli_host, b_moduli_host + h.K);
        p->moduli = full;
        {
            // the constants of scale_message and decode, in exact integers.  decode: 2 <= t < 2^(W-2) and t < every q_i;
            // scale_message: also gcd(t, q_i) = 1
            constexpr int W = static_cast<int>(8 * sizeof(T));
            const std::uint64_t t = plain_modulus;
            bool ok = t >= 2 && t < (std::uint64_t(1) << (W - 2));
            for (int i = 0; ok && i < L; i++)
                ok = t < h.mod[i];
            p->decode_ok = ok;
            if (ok)
            {
                auto shoup = [&](std::uint64_t v, std::uint64_t m) {
                    return static_cast<T>((static_cast<U128>(v) << W) / m);
                };
                p->decode_args.t = p->scale_args.t = static_cast<T>(t);
                p->decode_args.one_shoup_t = p->scale_args.one_shoup_t = shoup(1, t);
                std::uint64_t q_mod_t = 1 % t;
                bool coprime = true;
                for (int i = 0; i < L; i++)
                {
                    const std::uint64_t q = h.mod[i];
                    p->decode_args.t_shoup[i] = shoup(t, q);
                    q_mod_t = static_cast<std::uint64_t>(static_cast<U128>(q_mod_t) * (q % t) % t);
                    // t^-1 mod q by the extended Euclidean algorithm (q need not be prime)
                    __int128 r0 = static_cast<__int128>(q), r1 = static_cast<__int128>(t), c0 = 0, c1 = 1;
                    while (r1 != 0)
                    {
                        const __int128 quo = r0 / r1, r2 = r0 - quo * r1, c2 = c0 - quo * c1;
                        r0 = r1, r1 = r2, c0 = c1, c1 = c2;
                    }
                    if (r0 != 1)
                    {
                        coprime = false;
                        continue;
                    }
                    const std::uint64_t inv = static_cast<std::uint64_t>(c0 < 0 ? c0 + static_cast<__int128>(q) : c0);
                    p->scale_args.t_inv[i] = static_cast<T>(inv), p->scale_args.t_inv_shoup[i] = shoup(inv, q);
                }
                p->scale_args.q_mod_t = static_cast<T>(q_mod_t), p->scale_args.q_mod_t_shoup = shoup(q_mod_t, t);
                p->scale_args.half = static_cast<T>(t / 2);
                p->scale_ok = coprime;
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
            GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws + lay.up, run.data(), run.size() * sizeof(T), hipMemcpyHostToDevice,
                                            stream));
            GPUNTT_HIP_CHECK(hipStreamSynchronize(stream)); // `run` dies with this scope
            if (transforms)
            {
                p->ntt_q_i.reset(new NTTPlan<T>(inverse_table_device, full.data(), h.L, n_power, reduction_poly, INVERSE,
                                                mod_inverse_host, batch_hint, stream, p->ws + lay.ntt_q_i));
                p->ntt_q_f.reset(new NTTPlan<T>(forward_table_device, full.data(), h.L, n_power, reduction_poly, FORWARD,
                                                nullptr, batch_hint, stream, p->ws + lay.ntt_q_f));
                p->ntt_full_f.reset(new NTTPlan<T>(forward_table_device, full.data(), h.M, n_power, reduction_poly,
                                                   FORWARD, nullptr, batch_hint, stream, p->ws + lay.ntt_full_f));
                p->ntt_full_i.reset(new NTTPlan<T>(inverse_table_device, full.data(), h.M, n_power, reduction_poly,
                                                   INVERSE, mod_inverse_host, batch_hint, stream,
                                                   p->ws + lay.ntt_full_i));
            }
        }
        catch (...)
        {
            p->ntt_q_i.reset(), p->ntt_q_f.reset(), p->ntt_full_f.reset(), p->ntt_full_i.reset();
            if (p->owns)
                (void) hipFree(p->ws);
            throw;
        }
        p_ = p.release();
    }

    template <typename T> BfvMultiplyPlan<T>::~BfvMultiplyPlan()
    {
        if (p_ == nullptr)
            return;
        p_->ntt_q_i.reset(), p_->ntt_q_f.reset(), p_->ntt_full_f.reset(), p_->ntt_full_i.reset();
        if (p_->owns)
            (void) hipFree(p_->ws);
        delete p_;
    }

    template <typename T> void BfvMultiplyPlan<T>::extend(const T* device_in, T* device_full, int stacks, stream_t stream) const
    {
        p_->extend(device_in, device_full, stacks, stream);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::scale_round(const T* device_full, T* device_out, int stacks, stream_t stream) const
    {
        p_->scale_round(device_full, device_out, stacks, stream);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::multiply(const T* device_x, const T* device_y, T* device_out, int count, bool input_ntt,
                                      bool output_ntt, void* scratch_device, stream_t stream) const
    {
        p_->multiply(device_x, device_y, device_out, count, input_ntt, output_ntt, scratch_device, stream);
    }

    template <typename T>
    void BfvMultiplyPlan<T>::multiply_relinearize(const T* device_x, const T* device_y, const KeySwitchPlan<T>& key_switch,
                                                  const T* device_key, T* device_out, int count, bool input_ntt,
                                                  bool output_ntt, void* scratch_device, void* key_switch_scratch_device,
                                                  stream_t stream) const
    {
        p_->multiply_relinearize(device_x, device_y, key_switch, device_key, device_out, count, input_ntt, output_ntt,
                                 scratch_device, key_switch_scratch_device, stream);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::multiply_sum(const T* const* device_x_host, const T* const* device_y_host, int terms,
                                          T* device_out, int count, bool input_ntt, bool output_ntt, void* scratch_device,
                                          stream_t stream) const
    {
        p_->multiply_sum(device_x_host, device_y_host, terms, device_out, count, input_ntt, output_ntt, scratch_device,
                         stream);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::multiply_relinearize_sum(const T* const* device_x_host, const T* const* device_y_host,
                                                      int terms, const KeySwitchPlan<T>& key_switch, const T* device_key,
                                                      T* device_out, int count, bool input_ntt, bool output_ntt,
                                                      void* scratch_device, void* key_switch_scratch_device,
                                                      stream_t stream) const
    {
        p_->multiply_relinearize_sum(device_x_host, device_y_host, terms, key_switch, device_key, device_out, count,
                                     input_ntt, output_ntt, scratch_device, key_switch_scratch_device, stream);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::scale_message(const T* device_message, T* device_out, int count, bool to_ntt,
                                           stream_t stream) const
    {
        p_->scale_message(device_message, device_out, count, to_ntt, stream);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::decode(const T* device_x, T* device_message_out, T* device_noise_max, int stacks,
                                    stream_t stream, void* partials_device) const
    {
        p_->decode(device_x, device_message_out, device_noise_max, stacks, stream, partials_device);
    }
    template <typename T> size_t BfvMultiplyPlan<T>::decode_partials_bytes(int stacks) const
    {
        return p_->decode_partials(stacks);
    }
    template <typename T> size_t BfvMultiplyPlan<T>::decrypt_scratch_bytes(int count) const
    {
        return p_->decrypt_scratch(count);
    }
    template <typename T>
    void BfvMultiplyPlan<T>::decrypt(const T* device_ct, const KeySwitchPlan<T>& key_switch, const T* device_s_ntt,
                                     T* device_message_out, T* device_noise_max, int count, int components,
                                     bool input_ntt, void* scratch_device, void* key_switch_scratch_device,
                                     stream_t stream) const
    {
        p_->decrypt(device_ct, key_switch, device_s_ntt, device_message_out, device_noise_max, count, components,
                    input_ntt, scratch_device, key_switch_scratch_device, stream);
    }
    template <typename T> int BfvMultiplyPlan<T>::max_terms() const { return p_->max_terms; }
    template <typename T>
    int BfvMultiplyPlan<T>::max_terms(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host,
                                      int b_count, T plain_modulus, int n_power)
    {
        rns_check_n_power(n_power);
        return bfv_derive<T>(q_moduli_host, q_count, b_moduli_host, b_count, plain_modulus, n_power).max_terms;
    }
    template <typename T>
    size_t BfvMultiplyPlan<T>::sum_scratch_bytes(int q_count, int b_count, int n_power, int count, int operands)
    {
        bfv_check_counts(q_count, b_count);
        rns_check_n_power(n_power);
        return bfv_sum_scratch<T>(q_count, q_count + b_count, n_power, count, operands).total;
    }
    template <typename T> size_t BfvMultiplyPlan<T>::sum_scratch_bytes(int count, int operands) const
    {
        return bfv_sum_scratch<T>(p_->L, p_->M, p_->n, count, operands).total;
    }
    template <typename T> Modulus<T> BfvMultiplyPlan<T>::modulus(int m) const
    {
        if (m < 0 || m >= p_->M)
            throw std::invalid_argument("Invalid modulus index!");
        return p_->moduli[m];
    }
    template <typename T> ReductionPolynomial BfvMultiplyPlan<T>::reduction_poly() const { return p_->poly; }

    template <typename T> int BfvMultiplyPlan<T>::q_count() const { return p_->L; }
    template <typename T> int BfvMultiplyPlan<T>::b_count() const { return p_->K; }
    template <typename T> int BfvMultiplyPlan<T>::n_power() const { return p_->n; }
    template <typename T> T BfvMultiplyPlan<T>::plain_modulus() const { return p_->t; }
    template <typename T> bool BfvMultiplyPlan<T>::has_transforms() const { return static_cast<bool>(p_->ntt_full_f); }
    template <typename T> bool BfvMultiplyPlan<T>::owns_workspace() const { return p_->owns; }
    template <typename T> size_t BfvMultiplyPlan<T>::scratch_bytes(int count) const
    {
        return bfv_scratch<T>(p_->L, p_->M, p_->n, count).total;
    }

    template <typename T>
    void BfvMultiplyPlan<T>::constants(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host,
                                       int b_count, T plain_modulus, int n_power, const BfvConstants<T>& out)
    {
        rns_check_n_power(n_power);
        const BfvHost h = bfv_derive<T>(q_moduli_host, q_count, b_moduli_host, b_count, plain_modulus, n_power);
        for (const T* ptr : {out.t_mod, out.t_mod_shoup, out.t_qhat_inv, out.t_qhat_inv_shoup})
            if (ptr == nullptr)
                throw std::invalid_argument("null pointer argument");
        auto copy = [](const std::vector<std::uint64_t>& v, T* dst) {
            if (dst == nullptr)
                throw std::invalid_argument("null pointer argument");
            for (size_t i = 0; i < v.size(); i++)
                dst[i] = static_cast<T>(v[i]);
        };
        for (const auto& side : {std::pair<const host::BcHostConsts*, const BaseConvConstants<T>*>{&h.up, &out.up},
                                 {&h.down, &out.down}})
        {
            const host::BcHostConsts& c = *side.first;
            const BaseConvConstants<T>& o = *side.second;
            copy(c.w, o.qhat_inv), copy(c.wp, o.qhat_inv_shoup), copy(c.matrix, o.matrix), copy(c.qmod, o.q_mod_p);
            copy(c.qinv, o.q_inv_mod_p), copy(c.recip, o.recip), copy(c.blen, o.bit_length);
        }
        copy(h.tm, out.t_mod), copy(h.tmp, out.t_mod_shoup), copy(h.wt, out.t_qhat_inv), copy(h.wtp, out.t_qhat_inv_shoup);
    }

    template <typename T>
    void BfvMultiplyPlan<T>::reference_extend(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host,
                                              int b_count, const T* in_host, T* full_host, int n_power, int stacks)
    {
        const BfvHost h = bfv_derive<T>(q_moduli_host, q_count, b_moduli_host, b_count, 2, -1);
        bfv_check_stacks<T>(h.L, h.M, in_host, full_host, n_power, stacks, "extend input and output overlap!");
        const size_t n = size_t(1) << n_power;
        std::uint64_t x[BASECONV_MAX_COUNT], conv[BASECONV_MAX_COUNT];
        for (int s = 0; s < stacks; s++)
            for (size_t j = 0; j < n; j++)
            {
                const T* src = in_host + static_cast<size_t>(s) * h.L * n + j;
                T* dst = full_host + static_cast<size_t>(s) * h.M * n + j;
                for (int i = 0; i < h.L; i++)
                {
                    x[i] = src[i * n] % h.mod[i];
                    dst[i * n] = static_cast<T>(x[i]);
                }
                host::bc_ref_convert<T>(h.up, x, true, conv);
                for (int k = 0; k < h.K; k++)
                    dst[(h.L + k) * n] = static_cast<T>(conv[k]);
            }
    }

    template <typename T>
    void BfvMultiplyPlan<T>::reference_scale_round(const Modulus<T>* q_moduli_host, int q_count,
                                                   const Modulus<T>* b_moduli_host, int b_count, T plain_modulus,
                                                   const T* full_host, T* out_host, int n_power, int stacks)
    {
        const BfvHost h = bfv_derive<T>(q_moduli_host, q_count, b_moduli_host, b_count, plain_modulus, -1);
        bfv_check_stacks<T>(h.L, h.M, out_host, full_host, n_power, stacks, "scale_round input and output overlap!");
        const size_t n = size_t(1) << n_power;
        std::uint64_t s[BASECONV_MAX_COUNT], conv[BASECONV_MAX_COUNT], r[BASECONV_MAX_COUNT];
        for (int st = 0; st < stacks; st++)
            for (size_t j = 0; j < n; j++)
            {
                const T* src = full_host + static_cast<size_t>(st) * h.M * n + j;
                for (int m = 0; m < h.M; m++) // step 1
                    s[m] = static_cast<std::uint64_t>(static_cast<U128>(h.tm[m]) * (src[m * n] % h.mod[m]) % h.mod[m]);
                host::bc_ref_convert<T>(h.up, s, true, conv); // step 2
                for (int k = 0; k < h.K; k++)
                {
                    const std::uint64_t b = h.mod[h.L + k], c = s[h.L + k];
                    const std::uint64_t diff = c >= conv[k] ? c - conv[k] : c + (b - conv[k]);
                    r[k] = static_cast<std::uint64_t>(static_cast<U128>(diff) * h.up.qinv[k] % b);
                }
                host::bc_ref_convert<T>(h.down, r, true, conv); // step 3
                for (int i = 0; i < h.L; i++)
                    out_host[(static_cast<size_t>(st) * h.L + i) * n + j] = static_cast<T>(conv[i]);
            }
    }

    template class BfvMultiplyPlan<Data32>;
    template class BfvMultiplyPlan<Data64>;
} // namespace gpuntt
