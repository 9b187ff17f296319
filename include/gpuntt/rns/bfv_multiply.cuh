// gpuntt/rns/bfv_multiply.cuh -- scale-invariant ciphertext multiplication (extension: no counterpart in the reference).
//
// The product the BFV family needs, round(t (x (x) y) / Q) over the integers, as ONE plan that owns the constants, the
// order of steps, the scratch layout and the size proof of the auxiliary base -- the third operation
// rns/base_conversion.cuh was built for, beside ModUp / ModDown (rns/key_switch.cuh) and rescaling.  All integers,
// W = 8 * sizeof(T).
//
// Bases.  q-primes q_0 .. q_{L-1}, Q = prod q_i; auxiliary primes b_0 .. b_{K-1}, B = prod b_j; the FULL base is
// {q_0 .. q_{L-1}, b_0 .. b_{K-1}} in that order, M = L + K <= 64 limbs, modulus m_m of the full base is q_m for m < L and
// b_{m-L} otherwise.  The plaintext modulus t is a word, t >= 2; it is reduced per limb on the host.  N = 2^n_power,
// n_power in [1, 28].  The constructor requires
//       B >= 2 t N Q,
// checked in exact integers on the host: std::invalid_argument("Auxiliary base too small!") otherwise.
//   Why that is enough.  extend chooses |x~| <= Q (1/2 + eps), eps = 3 L / 2^W, so every coefficient of a tensor
//   component obeys |d_c| <= 2 N Q^2 (1/2 + eps)^2 (d_1 is a sum of two negacyclic or cyclic products of N terms each).
//   Divide by Q and multiply by t: |round(t d_c / Q)| <= 2 t N Q (1/2 + eps)^2 + 1/2 <= (B / 4) (1 + 2 eps)^2 + 1/2, half of
//   what the centred representation modulo B holds.  So t d_c is an integer whose quotient fits B / 2 (scale_round below),
//   and the last conversion, from {b} back to {q}, never comes near its band [B / 2, B / 2 + eps B): it is exact.
//
//   extend(in, full, stacks):  in = T[stacks][L][N] in coefficient form, ANY word is accepted (read modulo q_i);
//     full = T[stacks][M][N]:
//       m < L:      full[s][m] = in[s][m] mod q_m                                   canonical
//       m = L + j:  full[s][m] = WORD FOR WORD what BaseConvPlan({q} -> {b})::convert gives in centred mode for stack s
//     -- the residues of the representative of x in [-Q/2, Q/2 + eps Q) (base_conversion.cuh).  ONE launch of bfv_extend
//     (KeySwitchPlan::mod_up at a single digit; a sibling of its kernel).  `in` must not overlap `full`
//   scale_round(full, out, stacks):  full = T[stacks][M][N] in coefficient form, ANY word; out = T[stacks][L][N].
//     DEFINITION, word for word, through the calls that exist beside it:
//       1. s_m = ((t mod m_m) * full_m) mod m_m for every limb            -- what operator_gpu's multiplication gives
//       2. r = BaseConvPlan({q} -> {b})::convert_and_divide, centred, with in = the q-limbs of s and c = the b-limbs of
//          s: T[K] per column
//       3. out = BaseConvPlan({b} -> {q})::convert, centred, of r
//     Outside step 2's rounding band this is round(t X / Q) mod q_i for ANY integer X with those residues whose quotient
//     fits B / 2; inside the band it is that value +- 1, exactly as mod_down documents.  ONE launch of bfv_scale_round:
//     the K intermediate words never reach memory.  out must not overlap full (stacks of full are M N words apart, those
//     of out L N)
//   multiply(x, y, out, count, input_ntt, output_ntt, scratch):  x, y = T[2][count][L][N], the component-major layout every
//     plan call writes; y may be exactly x (a squaring).  In coefficient form (input_ntt false) every word may hold any
//     value: extend reads it modulo q_m.  In NTT form the first step is a transform, which is defined on residues: the
//     words are canonical, as GPU_INTT takes them.  out = T[3][count][L][N]: out[2] is directly the c_in of
//     KeySwitchPlan::apply for relinearization (components = 2; add its two outputs to out[0], out[1] modulo q_m) --
//     multiply_relinearize below does all of that in one call, KeySwitchPlan::relinearize the second half.
//     DEFINITION, word for word:
//       1. [input_ntt: GPU_INTT over the q-base, 2 * count * L polynomials per operand]
//       2. extend over the 2 * count stacks of each operand
//       3. the full-base GPU_NTT
//       4. per limb m < M the canonical residues d0 = x0 y0, d1 = x0 y1 + x1 y0, d2 = x1 y1 modulo m_m -- each what
//          InnerProductPlan::multiply_accumulate gives (D = 1 for d0 and d2, D = 2 for d1, C = 1), as in
//          multiply_relinearize's step 1
//       5. the full-base GPU_INTT over 3 * count * M polynomials
//       6. scale_round over 3 * count stacks
//       7. [output_ntt: the q-base GPU_NTT over 3 * count * L polynomials]
//     What runs: [the q-base INTT and] bfv_extend once per operand (once in all for a squaring), ONE full-base NTT over
//     both operands, ONE bfv_tensor, ONE full-base INTT, ONE bfv_scale_round, [ONE q-base NTT].  No step's launch count
//     grows with count.  multiply allocates nothing and never synchronises: one stream, capturable into a hipGraph as it
//     is.  count = 0 launches nothing.
//   multiply_relinearize(x, y, key_switch, key, out, count, input_ntt, output_ntt, scratch, key_switch_scratch):  the
//     product, relinearized: BFV ct x ct in one call.  key_switch is a KeySwitchPlan<T> over the same q-base (its special
//     base, digits and key layout are its own), key the relinearization key it reads (s^2 -> s), out = T[2][count][L][N].
//     DEFINITION, word for word:
//       m = multiply(x, y, count, input_ntt, output_ntt = false)
//       out = key_switch.relinearize(m[0..1], m[2], key, count, input_ntt = false, output_ntt)
//     What runs: steps 1 to 5 of multiply; bfv_scale_round over stacks 0 .. 2 count - 1 INTO out; bfv_scale_round over
//     stacks 2 count .. 3 count - 1 into the scratch's coefficient region (dead since bfv_extend; T[count][L][N] fits its
//     T[2][count][L][N]); relinearize's coefficient path with mod_down_add in place on out.  No T[3][count][L][N]
//     temporary, no add pass, no transform of the low components on their own.  scratch_bytes(count) is unchanged;
//     key_switch_scratch is key_switch.scratch_bytes(count, 2) bytes, 256-byte aligned.  out may be exactly x or exactly
//     y, as for multiply; the two scratches must not overlap each other, out, an operand or the key.  Allocates nothing,
//     never synchronises, capturable as it is; count = 0 launches nothing.
//     std::invalid_argument("The key-switching plan does not match!"), before anything is launched: a q-modulus differs in
//     value, q_count, n_power or the reduction polynomial differs, or one of the two plans has no transforms.  Then
//     multiply's refusals, a null key or key_switch_scratch, a misaligned key_switch_scratch, and a count beyond
//     relinearize's limits
//   multiply_sum(x, y, terms, out, count, input_ntt, output_ntt, scratch):  the sum of `terms` products with ONE division
//     by Q: round(t * sum_t (x~_t (x) y~_t) / Q).  The tensor is bilinear and the division comes after it, so the sum is
//     taken in the full base, in NTT form, in exact accumulators, and every later step of multiply runs once whatever
//     `terms` is.  x, y: HOST arrays of `terms` device pointers (as KeySwitchPlan::multiply_relinearize_sum takes them),
//     each a batch T[2][count][L][N] with multiply's rules for the words; y[t] may be x[t], and the same pointer may
//     appear in any number of terms on either side.  out = T[3][count][L][N].  1 <= terms <= BFV_MAX_TERMS
//     ("Invalid terms!") and terms <= max_terms() ("Auxiliary base too small for these terms!"), both before any launch.
//     DEFINITION, word for word, through multiply's steps:
//       1. steps 1 to 3 for every DISTINCT operand pointer
//       2. step 4 summed: per limb m < M the canonical residues d0 = (sum_t x0_t y0_t) mod m_m,
//          d1 = (sum_t x0_t y1_t + x1_t y0_t) mod m_m, d2 = (sum_t x1_t y1_t) mod m_m -- each what
//          InnerProductPlan::multiply_accumulate gives with D = terms for d0 and d2, D = 2 * terms for d1, and C = 1
//          (BFV_MAX_TERMS keeps 2 * terms inside INNERPROD_MAX_DIGITS)
//       3. steps 5 to 7 unchanged: ONE full-base GPU_INTT over 3 * count * M polynomials, scale_round over 3 * count
//          stacks, [the q-base GPU_NTT]
//     With terms = 1 these are the words of multiply.
//     Size.  Every extended operand obeys |x~| <= Q (1/2 + eps), so |sum_t d_c| <= terms * 2 N Q^2 (1/2 + eps)^2 and the
//     argument above needs B >= 2 * terms * t N Q and nothing else.  max_terms() = min(BFV_MAX_TERMS,
//     floor(B / (2 t N Q))) >= 1 is fixed at construction in exact integers; the constructor's check is its terms = 1 case.
//     Rounding.  With more terms the result is NOT word for word the sum of `terms` multiply calls: this call rounds
//     S = t * sum D / Q once, they round `terms` times.  |round(S) - S| <= 1/2 and |sum_t round(a_t) - S| <= terms / 2, so
//     outside the conversion bands the centred difference per coefficient is at most (terms + 1) / 2; every band hit
//     (mod_down's documented +- 1) adds at most 1 per rounding, so it is unconditionally at most
//     (terms + 1) / 2 + terms + 1.
//     What runs: the DISTINCT operand pointers are collected on the host by pointer equality, U <= 2 * terms of them, so a
//     squaring or a vector shared by several terms is extended and transformed once.  Per distinct operand [the q-base
//     INTT and] bfv_extend; ONE full-base NTT over 2 * U * count * M polynomials; ONE bfv_tensor_sum; ONE full-base INTT
//     over 3 * count * M; ONE bfv_scale_round; [ONE q-base NTT].  Apart from the per-operand step no launch count grows
//     with terms or count.  Allocates nothing, never synchronises, one stream, capturable as it is; count = 0 launches
//     nothing.
//     scratch: sum_scratch_bytes(count, operands) bytes with operands >= U (the call lays it out for exactly U and
//     uses the first sum_scratch_bytes(count, U) bytes; a wrapper that knows the size of the buffer -- the Python one --
//     refuses a smaller one; operands outside [1, 2 * BFV_MAX_TERMS]: "Invalid operands!"), 256-byte aligned:
//     T[max(operands, 2)][2][count][M][N] for the extended
//     operands, contiguous (bfv_tensor_sum writes d0, d1, d2 over its first three planes, each word by the lane that read
//     it), and the T[2][count][L][N] coefficient region of multiply, reused operand by operand in stream order.  It
//     grows linearly with the distinct operands: a caller who cannot afford it splits the sum and adds the parts, at
//     one rounding per part.
//     Refusals: multiply's, applied to every operand pointer -- a null pointer (or a null array), overlap with out other
//     than being exactly out, overlap with the scratch, a misaligned scratch, and the count limits with the widest
//     transform batch 2 * U * count * M as an int
//   multiply_relinearize_sum(x, y, terms, key_switch, key, out, count, input_ntt, output_ntt, scratch,
//     key_switch_scratch):  the summed product, relinearized: an encrypted BFV dot product with ONE t/Q rounding, ONE key
//     switch and ONE ModDown.  out = T[2][count][L][N].
//     DEFINITION, word for word:
//       m = multiply_sum(x, y, terms, count, input_ntt, output_ntt = false)
//       out = key_switch.relinearize(m[0..1], m[2], key, count, input_ntt = false, output_ntt)
//     exactly as multiply_relinearize is defined from multiply, and run in the same way: bfv_scale_round over the first
//     2 * count stacks INTO out, the top component into the coefficient region (dead by then), mod_down_add in place.
//     With terms = 1 these are the words of multiply_relinearize; with more terms the rounding bounds above hold for
//     m.  They do not carry over to out word by word: a top component that differs by one is decomposed into other
//     digits, and the switched words differ by a multiple of the key.  What is close is the decryption, where this call
//     carries one t/Q rounding and one ModDown rounding and the separate calls `terms` of each.
//     Refusals: multiply_relinearize's, applied to every operand pointer
//   scratch: scratch_bytes(count) bytes owned by the CALLER, 256-byte aligned: the operands in the full base
//     T[4][count][M][N] (x0, x1, y0, y1 -- bfv_tensor writes d0, d1, d2 over the first three, each word by the lane that
//     read it) and T[2][count][L][N] for the coefficient form of one operand.
//   overlap: out may be exactly x or exactly y -- their last read (bfv_extend, or the INTT before it) precedes the first
//     write of out (bfv_scale_round) on the stream.  Any other overlap of out or the scratch with an operand or with each
//     other: std::invalid_argument before anything is launched.  The same for a null pointer, a scratch that is not
//     256-byte aligned, count < 0, a count beyond the grid and int limits of the transforms and kernels, and a multiply on
//     a plan without transforms
//
// Reading a result back (the kernels are in decrypt.hip).  The three calls below need a plaintext modulus
// with 2 <= t < 2^(W-2) and t < every q_i -- and, for scale_message, gcd(t, q_i) = 1 --:
// std::invalid_argument("Plaintext modulus not usable here!") otherwise, from these calls only (multiply* take any t >= 2).
// Their constants (Q mod t, t^-1 mod q_i, floor(t 2^W / q_i), with Shoup companions) are derived on the host at
// construction in exact integers and travel as kernel arguments: workspace_bytes and every launch above are unchanged.
//   scale_message(message, out, count, to_ntt):  round(Q m / t) in the q-base, what KeySwitchPlan::encrypt_symmetric /
//     encrypt_public take as message_ntt.  message = T[count][N], any word, read modulo t; out = T[count][L][N].
//     DEFINITION, with m = word mod t, h = floor(t / 2) and r = ((Q mod t) m + h) mod t:
//       out[c][i][j] = floor((Q m + h) / t) mod q_i = ((h - r) [t^-1 mod q_i]) mod q_i, canonical
//     (Q m vanishes modulo q_i: no wide arithmetic).  ONE launch of bfv_scale_message, then with to_ntt the q-base
//     GPU_NTT in place.  Refusals: a null pointer, message overlapping out, count < 0 or count * L beyond an int,
//     to_ntt on a plan without transforms; count = 0 launches nothing
//   decode(x, message_out, noise_max, stacks):  m = round(t x / Q) mod t with the noise, from coefficient-form residues.
//     x = T[stacks][L][N], any word; message_out = T[stacks][N]; noise_max = T[stacks] or nullptr.  DEFINITION, all
//     integers, per coefficient, on base_conversion.cuh's constants qhat_i^-1 and R_i = floor(2^(W-1+b_i) / q_i), b_i the
//     bit length of q_i:
//       y_i = (x_i [qhat_i^-1 mod q_i]) mod q_i, canonical
//       (a_i, r_i) = divmod(t y_i, q_i)                      -- a_i < t
//       z_i = (r_i R_i) >> (b_i - 1)
//       S = 2^W sum_i a_i + sum_i z_i
//       message_out = ((S + 2^(W-1)) >> W) mod t
//       noise word n = ((S + 2^(W-1)) mod 2^W) - 2^(W-1), a signed W-bit value;  noise_max[s] = max_j |n|
//     Why this is the rounding.  t x / Q = sum_i t y_i / q_i (mod t), and 0 <= r_i 2^W / q_i - z_i < 3, so 2^W (t x / Q)
//     lies in [S, S + 3 L) modulo t 2^W.  THE BAND: outside (S mod 2^W) in [2^(W-1) - 3 L, 2^(W-1)) message_out is
//     round-half-up(t x^ / Q) mod t for any representative x^; inside it is that value or that value - 1 (mod t).  The
//     invariant noise v = t x / Q - round(.) obeys |n| <= 2^W |v| + 3 L and 2^W |v| <= |n| + 3 L.
//     noise_budget_bits(noise_max, L) = max(0, W - 1 - bit_length(noise_max + 3 L)) below is SEAL's invariant noise budget,
//     conservative by the band, and CAPPED at W - 1 - bit_length(3 L): a larger true budget (wide bases, fresh
//     ciphertexts) reads as the cap -- see the limitation stated at the function.
//     What runs: [noise_max given: a hipMemsetAsync of its T[stacks],] ONE launch of bfv_decode: a lane owns a 16-byte
//     group of columns and walks the limbs; the per-stack maximum is reduced across the wave (lane exchanges) and the
//     workgroup (one word per wave in LDS, one barrier) and merged with one atomicMax per workgroup, only when
//     noise_max is given (nullptr: nothing is written there).
//     partials_device (optional, last argument): decode_partials_bytes(stacks) bytes of device memory.  Given, the same
//     words come from TWO launches and no memset: bfv_decode stores every workgroup's maximum there and
//     bfv_decode_merge (one wave per stack) stores noise_max.  Which is faster is a matter of the call's size
//     (DESIGN.md 3.23 has both, measured); decrypt uses the one-launch form.  partials must not overlap x or an output  Refusals: a null x or
//     message_out, x overlapping an output (or the outputs each other), stacks < 0 or beyond the grid limit; stacks = 0
//     launches nothing
//   decrypt(ct, key_switch, s_ntt, message_out, noise_max, count, components, input_ntt, scratch, key_switch_scratch):
//     DEFINITION, word for word:
//       key_switch.phase(ct, s_ntt, scratch, count, components, input_ntt, output_ntt = false, key_switch_scratch)
//       decode(scratch, message_out, noise_max, count)
//     The two plans are checked against each other first, as multiply_relinearize checks them ("The key-switching plan
//     does not match!").  scratch: decrypt_scratch_bytes(count) bytes = T[count][L][N], 256-byte aligned;
//     key_switch_scratch: key_switch.phase_scratch_bytes(count, components, input_ntt) bytes (nullptr is accepted where
//     that is 0).  Every refusal of both calls arrives before the first launch.  Allocates nothing, never synchronises,
//     one stream, capturable as it is (the memset is a node)
//   Not here: CKKS encode / decode, a centred multi-precision output of the phase, BGV, noise flooding, the INTT's last
//     pass fused into bfv_decode.  (BFV batching -- slots to and from the coefficients modulo t -- is rns/bfv_encode.cuh.)
//
//
//   * transforms: as KeySwitchPlan -- ONE caller table pair in full-base order (slot i at i << n_power, the q-base is its
//     first L slots), the M host n^-1 values, the reduction polynomial and a batch_hint; the plan builds four NTTPlan<T>
//     inside its workspace (inverse and forward over the q-base, forward and inverse over the full base).  The tables
//     must outlive the plan.  Both table pointers nullptr: a plan without transforms -- extend and scale_round work for
//     any pairwise coprime Modulus<T> (not necessarily prime), multiply throws
//   * workspace: every constant and every NTTPlan lives in workspace_bytes(L, K, n_power) bytes of device memory (nullptr =
//     the plan allocates and owns it; owns_workspace()).  The constructor waits for `stream` once for its own constants
//     and once in each NTTPlan it builds: up to five host waits per plan, none afterwards
//   * std::invalid_argument from the constructor: "Auxiliary base too small!", a modulus that is not the Modulus<T> of
//     its value ("Invalid modulus!"), n_power outside [1, 28] ("Invalid n_power range!"), moduli of the full base that are
//     not pairwise coprime, L < 1, K < 1, M > 64, t < 2 ("Invalid plaintext modulus!"), one table pointer without the
//     other or without the n^-1 values
#pragma once

#include <cstddef>
#include <cstdint>

#include "gpuntt/common/common.cuh"
#include "gpuntt/common/modular_arith.cuh"
#include "gpuntt/common/nttparameters.cuh"
#include "gpuntt/rns/base_conversion.cuh"
#include "gpuntt/rns/key_switch.cuh"

namespace gpuntt
{
    // terms of one multiply_sum call at most: the cross term is one exact sum of 2 * terms products
    constexpr int BFV_MAX_TERMS = 32;

    // SEAL's invariant noise budget in bits from decode's noise_max over L limbs: max(0, W - 1 - bit_length(noise_max +
    // 3 L)), conservative by the band of decode ("Reading a result back" in this header).
    // LIMITATION: the noise word has W bits, so the result never exceeds W - 1 - bit_length(3 L) (59 bits for u64 at
    // L = 3, 27 for u32).  A ciphertext whose true budget is larger -- any fresh one over a base of two or more 60-bit
    // primes, where the budget is log2(Q / (2 t |e|)) > 64 -- reads as that cap, before and after an operation alike:
    // the value says "at least this much" there and nothing more.  It resolves the budget only once the noise has
    // grown to within W bits of Q / t
    template <typename T> inline int noise_budget_bits(T noise_max, int q_count)
    {
        constexpr int W = static_cast<int>(8 * sizeof(T));
        unsigned __int128 v = static_cast<unsigned __int128>(noise_max) + 3u * static_cast<unsigned>(q_count);
        int bits = 0;
        for (; v != 0; v >>= 1)
            bits++;
        return W - 1 - bits > 0 ? W - 1 - bits : 0;
    }

    // The plan's constants as the host derived them (BfvMultiplyPlan::constants, gpuntt_bfv_constants_*): every pointer
    // is a caller array of the stated length.
    template <typename T> struct BfvConstants
    {
        BaseConvConstants<T> up;   // BaseConvPlan::constants({q} -> {b}): extend, and step 2 of scale_round
        BaseConvConstants<T> down; // BaseConvPlan::constants({b} -> {q}): step 3 of scale_round
        T* t_mod;                  // [M] t mod m_m
        T* t_mod_shoup;            // [M] floor((t mod m_m) 2^W / m_m)
        // what bfv_scale_round multiplies with: t folded into the first constant of the first conversion
        T* t_qhat_inv;       // [L] (t * qhat_i^-1) mod q_i
        T* t_qhat_inv_shoup; // [L] its Shoup companion
    };

    template <typename T> class BfvMultiplyPlan
    {
      public:
        static size_t workspace_bytes(int q_count, int b_count, int n_power);
        static size_t scratch_bytes(int q_count, int b_count, int n_power, int count);

        BfvMultiplyPlan(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host, int b_count,
                        T plain_modulus, int n_power, const Root<T>* forward_table_device,
                        const Root<T>* inverse_table_device, const Ninverse<T>* mod_inverse_host,
                        ReductionPolynomial reduction_poly, int batch_hint, stream_t stream,
                        void* workspace_device = nullptr);
        ~BfvMultiplyPlan();
        BfvMultiplyPlan(const BfvMultiplyPlan&) = delete;
        BfvMultiplyPlan& operator=(const BfvMultiplyPlan&) = delete;

        void extend(const T* device_in, T* device_full, int stacks, stream_t stream) const;
        void scale_round(const T* device_full, T* device_out, int stacks, stream_t stream) const;
        void multiply(const T* device_x, const T* device_y, T* device_out, int count, bool input_ntt, bool output_ntt,
                      void* scratch_device, stream_t stream) const;

        void multiply_relinearize(const T* device_x, const T* device_y, const KeySwitchPlan<T>& key_switch,
                                  const T* device_key, T* device_out, int count, bool input_ntt, bool output_ntt,
                                  void* scratch_device, void* key_switch_scratch_device, stream_t stream) const;

        // sum_t x[t] * y[t] with ONE division by Q; x, y: host arrays of `terms` device pointers ("multiply_sum" above)
        void multiply_sum(const T* const* device_x_host, const T* const* device_y_host, int terms, T* device_out,
                          int count, bool input_ntt, bool output_ntt, void* scratch_device, stream_t stream) const;
        void multiply_relinearize_sum(const T* const* device_x_host, const T* const* device_y_host, int terms,
                                      const KeySwitchPlan<T>& key_switch, const T* device_key, T* device_out, int count,
                                      bool input_ntt, bool output_ntt, void* scratch_device,
                                      void* key_switch_scratch_device, stream_t stream) const;
        // encode, decode and decrypt ("Reading a result back" above)
        void scale_message(const T* device_message, T* device_out, int count, bool to_ntt, stream_t stream) const;
        void decode(const T* device_x, T* device_message_out, T* device_noise_max, int stacks, stream_t stream,
                    void* partials_device = nullptr) const;
        size_t decode_partials_bytes(int stacks) const; // the partial maxima of the two-launch decode
        size_t decrypt_scratch_bytes(int count) const; // T[count][L][N]
        void decrypt(const T* device_ct, const KeySwitchPlan<T>& key_switch, const T* device_s_ntt,
                     T* device_message_out, T* device_noise_max, int count, int components, bool input_ntt,
                     void* scratch_device, void* key_switch_scratch_device, stream_t stream) const;

        int max_terms() const; // min(BFV_MAX_TERMS, floor(B / (2 t N Q))), fixed at construction; >= 1
        static size_t sum_scratch_bytes(int q_count, int b_count, int n_power, int count, int operands);
        size_t sum_scratch_bytes(int count, int operands) const;

        int q_count() const;
        int b_count() const;
        Modulus<T> modulus(int m) const;            // modulus m < M of the full base, as the constructor took it
        ReductionPolynomial reduction_poly() const; // as the constructor took it
        int n_power() const;
        T plain_modulus() const;
        bool has_transforms() const;
        bool owns_workspace() const; // false: the plan lives in the caller's workspace and has allocated nothing
        size_t scratch_bytes(int count) const;

        // host only (no GPU): the constants of these bases and this t, with the checks of the constructor
        static void constants(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host, int b_count,
                              T plain_modulus, int n_power, const BfvConstants<T>& out);
        // host only (no GPU): what max_terms() of a plan of these bases, this t and this ring returns, with the checks of the
        // constructor
        static int max_terms(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host, int b_count,
                             T plain_modulus, int n_power);
        // host only (no GPU): extend / scale_round on HOST arrays, with unsigned __int128 and %, after the same argument
        // checks.  What tests and examples compare the kernels with; never a GPU fall-back
        static void reference_extend(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host,
                                     int b_count, const T* in_host, T* full_host, int n_power, int stacks);
        static void reference_scale_round(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* b_moduli_host,
                                          int b_count, T plain_modulus, const T* full_host, T* out_host, int n_power,
                                          int stacks);

      private:
        struct Impl;
        Impl* p_;
    };
} // namespace gpuntt
