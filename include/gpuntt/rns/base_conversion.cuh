// gpuntt/rns/base_conversion.cuh -- RNS fast base conversion (extension: no counterpart in the reference).
//
// From the residues of x modulo q_0 .. q_{L-1} (the input base, Q = prod q_i, qhat_i = Q / q_i) to its residues modulo
// p_0 .. p_{K-1} (the output base) without ever forming x: the kernel behind hybrid key switching (ModUp, ModDown),
// CKKS rescaling (L = 1) and BFV multiplication.  All integers, W = 8 * sizeof(T); per coefficient, from the input words
// x_i (ANY word value is read modulo q_i):
//
//   y_i   = (x_i * [qhat_i^-1 mod q_i]) mod q_i                                         canonical
//   approximate:  out_j = (sum_i y_i * [qhat_i mod p_j]) mod p_j                        = (x~ + u Q) mod p_j, 0 <= u < L
//   centred:      R_i = floor(2^(W-1+b_i) / q_i), b_i = bit length of q_i
//                 z_i = (y_i * R_i) >> (b_i - 1),   v = (sum_i z_i + 2^(W-1)) >> W
//                 out_j = (sum_i y_i * [qhat_i mod p_j] - v * [Q mod p_j]) mod p_j
//                 = the residue of the representative of x in [-Q/2, Q/2 + eps Q), eps = 3 L / 2^W: the exactly
//                 centred value unless x~ / Q lies in the band [1/2, 1/2 + eps)
//   convert_and_divide:  out_j = ((c_j - conv_j) * [Q^-1 mod p_j]) mod p_j  with conv_j from either mode and c a second
//                 operand in the output base (any word value is read modulo p_j).  Centred, with c and x the residues
//                 of one integer C: round(C / Q) mod p_j outside the band -- ModDown, and rescale when L = 1.
// Every output word is canonical.
//
//   * layout (the library's RNS convention, polynomial p uses modulus p % mod_count): in is T[count][L][N], out and c
//     are T[count][K][N], N = 2^n_power, n_power in [1, 28].  out may alias c; in must not overlap out
//   * the constants -- [qhat_i^-1]_{q_i} with its Shoup companion, the L x K matrix [qhat_i]_{p_j}, [Q]_{p_j},
//     [Q^-1]_{p_j}, R_i, b_i, and the folding constants of the final reduction -- are derived ONCE at construction, on the
//     host in exact integers, and uploaded into the workspace (workspace_bytes() bytes; nullptr = the plan allocates and
//     owns it).  The constructor waits for `stream` before it returns
//   * convert / convert_and_divide allocate nothing, never synchronise and launch exactly ONE kernel, so they can be
//     captured into a hipGraph as they are.  Every output word is written once; every input word is read from memory
//     once per call, unless count * N is too small to fill the part: then the outputs of a column tile are split over
//     up to 8 workgroups, each of which re-reads the tile's input
//   * moduli: any Modulus<T> the library accepts (not necessarily prime).  std::invalid_argument when the q_i are not
//     pairwise coprime, some gcd(q_i, p_j) != 1, a count is outside [1, 64], a modulus is not the Modulus<T> of its value
//     ("Invalid modulus!"), n_power is outside [1, 28] ("Invalid n_power range!") or in overlaps out
#pragma once

#include <cstddef>
#include <cstdint>

#include "gpuntt/common/common.cuh"
#include "gpuntt/common/modular_arith.cuh"

namespace gpuntt
{
    constexpr int BASECONV_MAX_COUNT = 64;

    enum class BaseConvMode : int
    {
        approximate = 0,
        centred = 1
    };

    // The plan's constants as the host derived them (BaseConvPlan::constants, gpuntt_baseconv_constants_*): every
    // pointer is a caller array of the stated length.
    template <typename T> struct BaseConvConstants
    {
        T* qhat_inv;       // [L]    qhat_i^-1 mod q_i
        T* qhat_inv_shoup; // [L]    floor(qhat_inv_i * 2^W / q_i)
        T* matrix;         // [L][K] qhat_i mod p_j, row i
        T* q_mod_p;        // [K]    Q mod p_j
        T* q_inv_mod_p;    // [K]    Q^-1 mod p_j
        T* recip;          // [L]    R_i mod 2^W (R_i = 2^W only for a power of two q_i: stored 0, the kernel shifts)
        T* bit_length;     // [L]    b_i
    };

    template <typename T> class BaseConvPlan
    {
      public:
        static size_t workspace_bytes(int in_count, int out_count);
        BaseConvPlan(const Modulus<T>* in_moduli_host, int in_count, const Modulus<T>* out_moduli_host, int out_count,
                     stream_t stream, void* workspace_device = nullptr);
        ~BaseConvPlan();
        BaseConvPlan(const BaseConvPlan&) = delete;
        BaseConvPlan& operator=(const BaseConvPlan&) = delete;

        void convert(const T* device_in, T* device_out, int n_power, int count, BaseConvMode mode,
                     stream_t stream) const;
        void convert_and_divide(const T* device_in, const T* device_c, T* device_out, int n_power, int count,
                                BaseConvMode mode, stream_t stream) const;

        int in_count() const;
        int out_count() const;
        bool owns_workspace() const; // false: the plan lives in the caller's workspace and has allocated nothing
        // host only (no GPU): the constants of these two bases, with the checks of the constructor
        static void constants(const Modulus<T>* in_moduli_host, int in_count, const Modulus<T>* out_moduli_host,
                              int out_count, const BaseConvConstants<T>& out);

      private:
        struct Impl;
        Impl* p_;
    };
} // namespace gpuntt
