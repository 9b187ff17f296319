// gpuntt/rns/inner_product.cuh -- RNS inner product (extension: no counterpart in the reference).
//
// The multiply-accumulate in the middle of hybrid key switching: every digit of a decomposed polynomial times the
// matching limb of the switching key, in the NTT domain, summed over the digits, once per key component.  All integers,
// W = 8 * sizeof(T).  The plan is built for M moduli q_0 .. q_{M-1}; one call computes, for r < count, c < C, m < M,
// j < N = 2^n_power:
//
//   out[c][r][m][j] = ( [accumulate ? out[c][r][m][j] : 0] + sum_{d < D} a[d][r][m][j] * key[d][c][limb(m)][j] ) mod q_m
//
// ANY word value of a, key and (when accumulating) out is read modulo q_m; every output word is canonical.  D = 1 is
// the Hadamard product; with accumulate the call adds a second product to a first (c_1 = a_0 b_1 + a_1 b_0).
//
//   * layouts: a is T[D][count][M][N] (digit-major), out is T[C][count][M][N] (component-major); each digit or component
//     is a stack in the library's RNS convention (polynomial p uses modulus p % M), so one RNS GPU_NTT call over
//     D * count * M polynomials writes a, one RNS GPU_INTT call over C * count * M polynomials consumes out, and one base
//     conversion per digit fills that digit's stack
//   * key is T[D_key][C][key_mod_count][N]; the call uses its first D digits (digit stride C * key_mod_count * N words
//     whatever D is) and, for modulus m, limb key_limbs[m] in [0, key_mod_count) -- nullptr: limb m.  A caller at a lower
//     level (fewer q-primes plus the special primes) uses the full-level key in place
//   * ranges: 1 <= M <= 64, 1 <= D <= 64, 1 <= C <= 4, count >= 0 (0: nothing happens), M <= key_mod_count <= 256,
//     n_power in [1, 28]
//   * the sum is kept exact -- 64 products of arbitrary words plus one word stay below 2^(2W+7): a 2W-bit sum and a
//     carry count -- and reduced ONCE per output word with the folding constants the plan derives on the host in exact
//     integers (constants()).  Operands are not pre-reduced and Modulus<T>::mu is not used
//   * multiply_accumulate allocates nothing, never synchronises and launches exactly ONE kernel, so it can be captured
//     into a hipGraph as it is (key_limbs_host is read before the call returns and travels as a kernel argument).
//     Every word of a is read once per call, out is written once (and read once only when accumulating), the key is
//     read once per block of inputs
//   * std::invalid_argument: a count or index outside the ranges above, a modulus that is not the Modulus<T> of its value
//     ("Invalid modulus!"), n_power outside [1, 28] ("Invalid n_power range!"), a null pointer, out overlapping a or key
#pragma once

#include <cstddef>
#include <cstdint>

#include "gpuntt/common/common.cuh"
#include "gpuntt/common/modular_arith.cuh"

namespace gpuntt
{
    constexpr int INNERPROD_MAX_MODULI = 64;
    constexpr int INNERPROD_MAX_DIGITS = 64;
    constexpr int INNERPROD_MAX_COMPONENTS = 4;
    constexpr int INNERPROD_MAX_KEY_MODULI = 256;

    // The folding constants as the host derived them (InnerProductPlan::constants, gpuntt_innerprod_constants_*): every
    // pointer is a caller array of M words.  The Shoup companion of w modulo q is floor(w 2^W / q).
    template <typename T> struct InnerProductConstants
    {
        T* pow_w;        // 2^W mod q_m
        T* pow_w_shoup;  // its Shoup companion
        T* pow_2w;       // 2^2W mod q_m
        T* pow_2w_shoup; // its Shoup companion
        T* one_shoup;    // floor(2^W / q_m): the Shoup companion of 1
    };

    template <typename T> class InnerProductPlan
    {
      public:
        static size_t workspace_bytes(int mod_count);
        InnerProductPlan(const Modulus<T>* moduli_host, int mod_count, stream_t stream,
                         void* workspace_device = nullptr);
        ~InnerProductPlan();
        InnerProductPlan(const InnerProductPlan&) = delete;
        InnerProductPlan& operator=(const InnerProductPlan&) = delete;

        void multiply_accumulate(const T* device_a, const T* device_key, T* device_out, int n_power, int digits,
                                 int components, int count, bool accumulate, int key_mod_count,
                                 const int* key_limbs_host, stream_t stream) const;

        int mod_count() const;
        bool owns_workspace() const; // false: the plan lives in the caller's workspace and has allocated nothing
        // host only (no GPU): the constants of these moduli, with the checks of the constructor
        static void constants(const Modulus<T>* moduli_host, int mod_count, const InnerProductConstants<T>& out);
        // host only (no GPU): the definition above on HOST arrays, with unsigned __int128 and %, after the argument
        // checks of multiply_accumulate.  What tests and examples compare the kernel with; never a GPU fall-back
        static void reference(const Modulus<T>* moduli_host, int mod_count, const T* a_host, const T* key_host,
                              T* out_host, int n_power, int digits, int components, int count, bool accumulate,
                              int key_mod_count, const int* key_limbs_host);

      private:
        struct Impl;
        Impl* p_;
    };
} // namespace gpuntt
