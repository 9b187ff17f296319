/*
 * gpuntt_c.h -- C ABI of the MI355X-native NTT library (libgpuntt.so).
 *
 * The reference (Alisah-Ozcan/GPU-NTT) exposes this path only as C++ templates resolved
 * through explicit instantiations; it has no FFI.  This header is the flat
 * extern "C" boundary an FFI (ctypes / cgo / JNI ...) binds instead -- plain pointers and
 * sizes, no C++ or torch types -- one entry point per reference template overload:
 *
 *   gpuntt_ntt_{u32,u64}        GPU_NTT<T>  single modulus   src/include/gpuntt/ntt_merge/ntt.cuh:315-321
 *   gpuntt_intt_{u32,u64}       GPU_INTT<T> single modulus   ntt.cuh:323-329
 *   gpuntt_ntt_rns_{u32,u64}    GPU_NTT<T>  RNS              ntt.cuh:395-401
 *   gpuntt_intt_rns_{u32,u64}   GPU_INTT<T> RNS              ntt.cuh:403-409
 *       (in == out gives the *_Inplace overloads, ntt.cuh:331-340,411-421;
 *        input_signed / output_signed select the Data32s/Data64s instantiations,
 *        src/lib/ntt_merge/ntt.cu:4948-5082)
 *   gpuntt_ntt_modulus_ordered_{u32,u64} / gpuntt_ntt_poly_ordered_{u32,u64}
 *                               GPU_NTT_Modulus_Ordered / GPU_NTT_Poly_Ordered   ntt.cuh:495-603
 *   gpuntt_4step_{u32,u64}      GPU_4STEP_NTT<T> single      src/include/gpuntt/ntt_4step/ntt_4step.cuh:278-283
 *   gpuntt_4step_rns_{u32,u64}  GPU_4STEP_NTT<T> RNS         ntt_4step.cuh:301-307
 *   gpuntt_transpose_{u32,u64}  GPU_Transpose<T>             ntt_4step.cuh:46-49
 *   gpuntt_modulus_*, gpuntt_merge_params_*, gpuntt_4step_params_*
 *                               Modulus<T>, NTTParameters<T>, NTTParameters4Step<T>
 *                               src/include/gpuntt/common/modular_arith.cuh:28-57,
 *                               src/include/gpuntt/common/nttparameters.cuh:56-170
 *
 *   gpuntt_plan_*               extension NTTPlan<T> (include/gpuntt/ntt_merge/ntt.cuh): tables prepared once,
 *                               caller-owned workspace; execute = transform kernels only
 *   gpuntt_automorphism_*, gpuntt_galois_element_u32
 *                               extension Galois automorphisms (include/gpuntt/ntt_merge/galois.cuh), NTT and
 *                               coefficient domain, single modulus or RNS
 *   gpuntt_baseconv_*           extension RNS fast base conversion (include/gpuntt/rns/base_conversion.cuh): ModUp,
 *                               ModDown and rescale from one prepared plan, one kernel launch per call
 *   gpuntt_innerprod_*          extension RNS inner product (include/gpuntt/rns/inner_product.cuh): the key-switching
 *                               multiply-accumulate over digits and key components, one kernel launch per call
 *   gpuntt_keyswitch_*          extension hybrid key switching (include/gpuntt/rns/key_switch.cuh): one plan for the
 *                               digit partition, ModUp of all digits in one launch, the inner product, the transforms
 *                               and ModDown in place inside the stacks; host-only constants and references;
 *                               key material: lift_small, generate_keys, encrypt_symmetric
 *                               decryption and public-key encryption: phase, encrypt_public; gpuntt_bfv_plan_*:
 *                               scale_message, decode, decrypt
 *                               plaintext operands: lift_centred, multiply_plain
 *   gpuntt_bfv_encoder_*, gpuntt_bfv_slot_maps
 *                               extension BFV batching (include/gpuntt/rns/bfv_encode.cuh): slots to and from the
 *                               coefficients modulo t, one permutation launch and one transform per call
 *   gpuntt_sample_*, gpuntt_philox4x32_10
 *                               extension counter-based samplers (include/gpuntt/rns/sampling.cuh): uniform residues and
 *                               small polynomials, with host references; not a cryptographic generator
 *   gpuntt_operator_gpu_*       diagnostic: the public device class OPERATOR_GPU<T>
 *                               (src/include/gpuntt/common/modular_arith.cuh:174-454) applied elementwise
 *
 * All data/table/modulus-array pointers are DEVICE pointers unless the name ends in _host.
 * Calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 * stream).  The transform entry points keep a library-owned twiddle scratch per (device, stream)
 * -- and per capture while a stream is being captured: first use / growth allocates, nothing is
 * freed, reused or synchronised on before gpuntt_release_workspaces(), so hipGraphs captured from
 * these calls stay replayable ("Scratch lifetime and hipGraphs").  gpuntt_plan_execute_* allocates nothing, never
 * synchronises and launches no preparation kernel.
 *
 * Return value: GPUNTT_OK, or a negative code with the text available from
 * gpuntt_last_error() (thread-local).  GPUNTT_ERR_INVALID_ARGUMENT corresponds to the
 * std::invalid_argument the C++ API throws (reference ntt.cu:2088-2091, 2252-2254),
 * GPUNTT_ERR_HIP to HipException/CudaException (reference common.cuh:42-50).
 */
#ifndef GPUNTT_C_H
#define GPUNTT_C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

#define GPUNTT_OK 0
#define GPUNTT_ERR_INVALID_ARGUMENT (-1)
#define GPUNTT_ERR_HIP (-2)
#define GPUNTT_ERR_UNKNOWN (-3)

    /* enum values of the reference (nttparameters.cuh:19-36) */
#define GPUNTT_FORWARD 0
#define GPUNTT_INVERSE 1
#define GPUNTT_PER_POLYNOMIAL 0
#define GPUNTT_PER_COEFFICIENT 1
#define GPUNTT_X_N_PLUS 0  /* negacyclic X^N + 1 */
#define GPUNTT_X_N_MINUS 1 /* cyclic     X^N - 1 */

    /* layout-identical to Modulus<Data32> / Modulus<Data64> */
    typedef struct { uint32_t value, bit, mu; } gpuntt_modulus32;
    typedef struct { uint64_t value, bit, mu; } gpuntt_modulus64;

    const char* gpuntt_last_error(void);
    int gpuntt_version(void);

    /* ---- Modulus<T>(q) ------------------------------------------------------------ */
    int gpuntt_modulus_u32(uint32_t q, gpuntt_modulus32* out_host);
    int gpuntt_modulus_u64(uint64_t q, gpuntt_modulus64* out_host);

    /* ---- Merge NTT, single modulus -------------------------------------------------- */
    int gpuntt_ntt_u32(const void* in, uint32_t* out, const uint32_t* roots,
                       gpuntt_modulus32 modulus, int n_power, int ntt_layout, int reduction_poly,
                       int input_signed, void* stream, int batch_size);
    int gpuntt_ntt_u64(const void* in, uint64_t* out, const uint64_t* roots,
                       gpuntt_modulus64 modulus, int n_power, int ntt_layout, int reduction_poly,
                       int input_signed, void* stream, int batch_size);
    int gpuntt_intt_u32(const uint32_t* in, void* out, const uint32_t* inverse_roots,
                        gpuntt_modulus32 modulus, int n_power, int ntt_layout, int reduction_poly,
                        uint32_t mod_inverse, int output_signed, void* stream, int batch_size);
    int gpuntt_intt_u64(const uint64_t* in, void* out, const uint64_t* inverse_roots,
                        gpuntt_modulus64 modulus, int n_power, int ntt_layout, int reduction_poly,
                        uint64_t mod_inverse, int output_signed, void* stream, int batch_size);

    /* ---- Merge NTT, RNS: polynomial p uses modulus p % mod_count, table at i << n_power -- */
    int gpuntt_ntt_rns_u32(const void* in, uint32_t* out, const uint32_t* roots,
                           const gpuntt_modulus32* modulus, int n_power, int ntt_layout,
                           int reduction_poly, int input_signed, void* stream, int batch_size,
                           int mod_count);
    int gpuntt_ntt_rns_u64(const void* in, uint64_t* out, const uint64_t* roots,
                           const gpuntt_modulus64* modulus, int n_power, int ntt_layout,
                           int reduction_poly, int input_signed, void* stream, int batch_size,
                           int mod_count);
    int gpuntt_intt_rns_u32(const uint32_t* in, void* out, const uint32_t* inverse_roots,
                            const gpuntt_modulus32* modulus, int n_power, int ntt_layout,
                            int reduction_poly, const uint32_t* mod_inverse, int output_signed,
                            void* stream, int batch_size, int mod_count);
    int gpuntt_intt_rns_u64(const uint64_t* in, void* out, const uint64_t* inverse_roots,
                            const gpuntt_modulus64* modulus, int n_power, int ntt_layout,
                            int reduction_poly, const uint64_t* mod_inverse, int output_signed,
                            void* stream, int batch_size, int mod_count);

    /* ---- ordered RNS entry points (reference ntt.cuh:495-603): ntt_type selects the direction,
     *      `order` is a device int array; mod_inverse (device, indexed by prime) is used for
     *      GPUNTT_INVERSE only.  n_power in [10, 28]. */
    int gpuntt_ntt_modulus_ordered_u32(const uint32_t* in, uint32_t* out, const uint32_t* roots,
                                       const gpuntt_modulus32* modulus, int n_power, int ntt_type,
                                       int reduction_poly, const uint32_t* mod_inverse, void* stream,
                                       int batch_size, int mod_count, const int* order);
    int gpuntt_ntt_modulus_ordered_u64(const uint64_t* in, uint64_t* out, const uint64_t* roots,
                                       const gpuntt_modulus64* modulus, int n_power, int ntt_type,
                                       int reduction_poly, const uint64_t* mod_inverse, void* stream,
                                       int batch_size, int mod_count, const int* order);
    int gpuntt_ntt_poly_ordered_u32(const uint32_t* in, uint32_t* out, const uint32_t* roots,
                                    const gpuntt_modulus32* modulus, int n_power, int ntt_type,
                                    int reduction_poly, const uint32_t* mod_inverse, void* stream,
                                    int batch_size, int mod_count, const int* order);
    int gpuntt_ntt_poly_ordered_u64(const uint64_t* in, uint64_t* out, const uint64_t* roots,
                                    const gpuntt_modulus64* modulus, int n_power, int ntt_type,
                                    int reduction_poly, const uint64_t* mod_inverse, void* stream,
                                    int batch_size, int mod_count, const int* order);

    /* ---- extension: polynomial product out = INTT(NTT(a) (.) NTT(b)) in Z_q[X]/(X^N -+ 1), the
     * composition of the reference's CPU example (test_cpu_merge_ntt.cu:69-101); a and b are
     * overwritten with their transforms, out may alias either; mod_inverse = N^-1 (RNS: device array) */
    int gpuntt_polymul_u32(uint32_t* a, uint32_t* b, uint32_t* out, const uint32_t* forward_table,
                           const uint32_t* inverse_table, gpuntt_modulus32 modulus, int n_power,
                           int reduction_poly, uint32_t mod_inverse, void* stream, int batch_size);
    int gpuntt_polymul_u64(uint64_t* a, uint64_t* b, uint64_t* out, const uint64_t* forward_table,
                           const uint64_t* inverse_table, gpuntt_modulus64 modulus, int n_power,
                           int reduction_poly, uint64_t mod_inverse, void* stream, int batch_size);
    int gpuntt_polymul_rns_u32(uint32_t* a, uint32_t* b, uint32_t* out, const uint32_t* forward_table,
                               const uint32_t* inverse_table, const gpuntt_modulus32* modulus,
                               int n_power, int reduction_poly, const uint32_t* mod_inverse,
                               void* stream, int batch_size, int mod_count);
    int gpuntt_polymul_rns_u64(uint64_t* a, uint64_t* b, uint64_t* out, const uint64_t* forward_table,
                               const uint64_t* inverse_table, const gpuntt_modulus64* modulus,
                               int n_power, int reduction_poly, const uint64_t* mod_inverse,
                               void* stream, int batch_size, int mod_count);

    /* ---- extension: Galois automorphisms sigma_k: a(X) -> a(X^k), k odd (include/gpuntt/ntt_merge/galois.cuh) ----
     * in is T[batch][N], out is T[galois_count][batch][N]; galois_elts_host holds 1..64 odd elements (reduced mod 2N
     * for X_N_plus, mod N for X_N_minus), passed to the kernel as arguments: one launch per call, no scratch.  in and
     * out must not overlap.  _ntt: the permutation of GPU_NTT's output order (no modulus); otherwise the coefficient
     * domain, negacyclic sign with the modulus (RNS: polynomial p uses modulus[p % mod_count], a device array). */
    int gpuntt_automorphism_ntt_u32(const uint32_t* in, uint32_t* out, const uint32_t* galois_elts_host,
                                    int galois_count, int n_power, int reduction_poly, void* stream, int batch_size);
    int gpuntt_automorphism_ntt_u64(const uint64_t* in, uint64_t* out, const uint32_t* galois_elts_host,
                                    int galois_count, int n_power, int reduction_poly, void* stream, int batch_size);
    int gpuntt_automorphism_u32(const uint32_t* in, uint32_t* out, const uint32_t* galois_elts_host, int galois_count,
                                gpuntt_modulus32 modulus, int n_power, int reduction_poly, void* stream,
                                int batch_size);
    int gpuntt_automorphism_u64(const uint64_t* in, uint64_t* out, const uint32_t* galois_elts_host, int galois_count,
                                gpuntt_modulus64 modulus, int n_power, int reduction_poly, void* stream,
                                int batch_size);
    int gpuntt_automorphism_rns_u32(const uint32_t* in, uint32_t* out, const uint32_t* galois_elts_host,
                                    int galois_count, const gpuntt_modulus32* modulus, int n_power, int reduction_poly,
                                    void* stream, int batch_size, int mod_count);
    int gpuntt_automorphism_rns_u64(const uint64_t* in, uint64_t* out, const uint32_t* galois_elts_host,
                                    int galois_count, const gpuntt_modulus64* modulus, int n_power, int reduction_poly,
                                    void* stream, int batch_size, int mod_count);
    /* host: conjugation == 0: the element rotating slots by `steps` (5^steps mod 2N, negative steps the inverse);
     * conjugation != 0: 2N - 1 (steps ignored) */
    int gpuntt_galois_element_u32(int steps, int n_power, int conjugation, uint32_t* elt_host);
    /* host: map_host[i] (N entries) = the source the kernels read for output slot i, from the same index functions.
     * GPUNTT_DOMAIN_NTT: a slot of GPU_NTT's output; GPUNTT_DOMAIN_COEFFICIENT: a coefficient, where for X_N_plus a
     * value j >= N means -in[j - N]. */
#define GPUNTT_DOMAIN_NTT 0
#define GPUNTT_DOMAIN_COEFFICIENT 1
    int gpuntt_automorphism_index_map(int n_power, uint32_t galois_elt, int reduction_poly, int domain,
                                      uint32_t* map_host);

    /* ---- 4-Step NTT (cyclic, 12 <= n_power <= 24, in != out) ------------------------ */
    int gpuntt_4step_u32(const uint32_t* in, uint32_t* out, const uint32_t* n1_table,
                         const uint32_t* n2_table, const uint32_t* w_table,
                         gpuntt_modulus32 modulus, int n_power, int ntt_type, uint32_t mod_inverse,
                         void* stream, int batch_size);
    int gpuntt_4step_u64(const uint64_t* in, uint64_t* out, const uint64_t* n1_table,
                         const uint64_t* n2_table, const uint64_t* w_table,
                         gpuntt_modulus64 modulus, int n_power, int ntt_type, uint64_t mod_inverse,
                         void* stream, int batch_size);
    /* extension: the reference examples' natural-order pipeline (GPU_Transpose -> GPU_4STEP_NTT ->
     * GPU_Transpose, test_4step_ntt.cu:147-178 / test_4step_intt.cu:81-179) as one call =
     * NTT_4STEP_CPU::ntt / ::intt; `in_scratch` is overwritten, in_scratch != out */
    int gpuntt_4step_natural_u32(uint32_t* in_scratch, uint32_t* out, const uint32_t* n1_table,
                                 const uint32_t* n2_table, const uint32_t* w_table,
                                 gpuntt_modulus32 modulus, int n_power, int ntt_type,
                                 uint32_t mod_inverse, void* stream, int batch_size);
    int gpuntt_4step_natural_u64(uint64_t* in_scratch, uint64_t* out, const uint64_t* n1_table,
                                 const uint64_t* n2_table, const uint64_t* w_table,
                                 gpuntt_modulus64 modulus, int n_power, int ntt_type,
                                 uint64_t mod_inverse, void* stream, int batch_size);
    int gpuntt_4step_rns_u32(const uint32_t* in, uint32_t* out, const uint32_t* n1_table,
                             const uint32_t* n2_table, const uint32_t* w_table,
                             const gpuntt_modulus32* modulus, int n_power, int ntt_type,
                             const uint32_t* mod_inverse, void* stream, int batch_size,
                             int mod_count);
    int gpuntt_4step_rns_u64(const uint64_t* in, uint64_t* out, const uint64_t* n1_table,
                             const uint64_t* n2_table, const uint64_t* w_table,
                             const gpuntt_modulus64* modulus, int n_power, int ntt_type,
                             const uint64_t* mod_inverse, void* stream, int batch_size,
                             int mod_count);
    int gpuntt_transpose_u32(const uint32_t* in, uint32_t* out, int row, int col, int n_power,
                             int batch_size);
    int gpuntt_transpose_u64(const uint64_t* in, uint64_t* out, int row, int col, int n_power,
                             int batch_size);

    /* ---- host-side parameter / table generation (no GPU needed) --------------------
     * factors_host: {q, omega, psi} or NULL for the built-in pool.
     * info_host[8] = {q, bit, mu, omega, psi, n_inv, root_of_unity_size, n}.
     * tables are written in DEVICE order (bit-reversed), root_of_unity_size entries each. */
    int gpuntt_merge_params_u32(int logn, int reduction_poly, const uint32_t* factors_host,
                                uint64_t* info_host, uint32_t* forward_table_host,
                                uint32_t* inverse_table_host);
    int gpuntt_merge_params_u64(int logn, int reduction_poly, const uint64_t* factors_host,
                                uint64_t* info_host, uint64_t* forward_table_host,
                                uint64_t* inverse_table_host);
    /* info_host[9] = {q, bit, mu, omega, psi, n_inv, n1, n2, n}; inverse != 0 selects the
     * inverse tables; n1/n2 tables in DEVICE order (n1/2, n2/2 entries), W natural (n). */
    int gpuntt_4step_params_u32(int logn, int inverse, uint64_t* info_host,
                                uint32_t* n1_table_host, uint32_t* n2_table_host,
                                uint32_t* w_table_host);
    int gpuntt_4step_params_u64(int logn, int inverse, uint64_t* info_host,
                                uint64_t* n1_table_host, uint64_t* n2_table_host,
                                uint64_t* w_table_host);

    /* ---- extension: prepared transforms (NTTPlan<T>) ----------------------------------------
     * moduli_host[mod_count], mod_inverse_host[mod_count] (GPUNTT_INVERSE only) are HOST arrays;
     * workspace_device: gpuntt_plan_workspace_bytes_*() bytes of device memory owned by the caller, or
     * NULL (the plan allocates).  Construction runs on `stream`; execute: in == out allowed, io_signed
     * = signed input (forward) / centred output (inverse); PerPolynomial layout. */
    typedef struct gpuntt_plan gpuntt_plan;
    int gpuntt_plan_workspace_bytes_u32(int n_power, int mod_count, uint64_t* bytes_host);
    int gpuntt_plan_workspace_bytes_u64(int n_power, int mod_count, uint64_t* bytes_host);
    int gpuntt_plan_create_u32(gpuntt_plan** plan_host, const uint32_t* table, const gpuntt_modulus32* moduli_host,
                               int mod_count, int n_power, int reduction_poly, int ntt_type,
                               const uint32_t* mod_inverse_host, int batch_hint, void* workspace_device,
                               void* stream);
    int gpuntt_plan_create_u64(gpuntt_plan** plan_host, const uint64_t* table, const gpuntt_modulus64* moduli_host,
                               int mod_count, int n_power, int reduction_poly, int ntt_type,
                               const uint64_t* mod_inverse_host, int batch_hint, void* workspace_device,
                               void* stream);
    int gpuntt_plan_execute_u32(const gpuntt_plan* plan, const void* in, void* out, int batch_size, int io_signed,
                                void* stream);
    int gpuntt_plan_execute_u64(const gpuntt_plan* plan, const void* in, void* out, int batch_size, int io_signed,
                                void* stream);
    int gpuntt_plan_fast_path_u32(const gpuntt_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_plan_fast_path_u64(const gpuntt_plan* plan);
    int gpuntt_plan_destroy_u32(gpuntt_plan* plan);
    int gpuntt_plan_destroy_u64(gpuntt_plan* plan);

    /* ---- extension: RNS fast base conversion (BaseConvPlan<T>, include/gpuntt/rns/base_conversion.cuh) ----------
     * in_moduli_host[in_count] (q_0 .. q_{L-1}, pairwise coprime) and out_moduli_host[out_count] (p_0 .. p_{K-1}, each
     * coprime to every q_i) are HOST arrays, 1 <= L, K <= 64.  workspace_device: gpuntt_baseconv_plan_workspace_bytes_*()
     * bytes of device memory owned by the caller, or NULL (the plan allocates).  in is T[count][L][N], out and c are
     * T[count][K][N], N = 2^n_power; out may alias c, in must not overlap out.  mode: GPUNTT_BASECONV_APPROXIMATE
     * ((x~ + u Q) mod p_j, 0 <= u < L) or GPUNTT_BASECONV_CENTRED (the representative in [-Q/2, Q/2 + 3L/2^W Q)).
     * convert_and_divide: out_j = ((c_j - conv_j) * Q^-1) mod p_j.  Both calls allocate nothing, never synchronise
     * and launch one kernel. */
#define GPUNTT_BASECONV_APPROXIMATE 0
#define GPUNTT_BASECONV_CENTRED 1
    typedef struct gpuntt_baseconv_plan gpuntt_baseconv_plan;
    int gpuntt_baseconv_plan_workspace_bytes_u32(int in_count, int out_count, uint64_t* bytes_host);
    int gpuntt_baseconv_plan_workspace_bytes_u64(int in_count, int out_count, uint64_t* bytes_host);
    int gpuntt_baseconv_plan_create_u32(gpuntt_baseconv_plan** plan_host, const gpuntt_modulus32* in_moduli_host,
                                        int in_count, const gpuntt_modulus32* out_moduli_host, int out_count,
                                        void* workspace_device, void* stream);
    int gpuntt_baseconv_plan_create_u64(gpuntt_baseconv_plan** plan_host, const gpuntt_modulus64* in_moduli_host,
                                        int in_count, const gpuntt_modulus64* out_moduli_host, int out_count,
                                        void* workspace_device, void* stream);
    int gpuntt_baseconv_plan_convert_u32(const gpuntt_baseconv_plan* plan, const uint32_t* in, uint32_t* out,
                                         int n_power, int count, int mode, void* stream);
    int gpuntt_baseconv_plan_convert_u64(const gpuntt_baseconv_plan* plan, const uint64_t* in, uint64_t* out,
                                         int n_power, int count, int mode, void* stream);
    int gpuntt_baseconv_plan_convert_and_divide_u32(const gpuntt_baseconv_plan* plan, const uint32_t* in,
                                                    const uint32_t* c, uint32_t* out, int n_power, int count, int mode,
                                                    void* stream);
    int gpuntt_baseconv_plan_convert_and_divide_u64(const gpuntt_baseconv_plan* plan, const uint64_t* in,
                                                    const uint64_t* c, uint64_t* out, int n_power, int count, int mode,
                                                    void* stream);
    int gpuntt_baseconv_plan_owns_workspace_u32(const gpuntt_baseconv_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_baseconv_plan_owns_workspace_u64(const gpuntt_baseconv_plan* plan);
    int gpuntt_baseconv_plan_destroy_u32(gpuntt_baseconv_plan* plan);
    int gpuntt_baseconv_plan_destroy_u64(gpuntt_baseconv_plan* plan);
    /* host only (no GPU): the constants a plan of these bases uploads, with the checks of plan_create.  Caller arrays:
     * qhat_inv[L] = qhat_i^-1 mod q_i, qhat_inv_shoup[L] = floor(qhat_inv_i 2^W / q_i), matrix[L][K] = qhat_i mod p_j,
     * q_mod_p[K], q_inv_mod_p[K], recip[L] = floor(2^(W-1+b_i) / q_i) mod 2^W (0 for a power of two q_i),
     * bit_length[L] = b_i */
    int gpuntt_baseconv_constants_u32(const gpuntt_modulus32* in_moduli_host, int in_count,
                                      const gpuntt_modulus32* out_moduli_host, int out_count, uint32_t* qhat_inv,
                                      uint32_t* qhat_inv_shoup, uint32_t* matrix, uint32_t* q_mod_p,
                                      uint32_t* q_inv_mod_p, uint32_t* recip, uint32_t* bit_length);
    int gpuntt_baseconv_constants_u64(const gpuntt_modulus64* in_moduli_host, int in_count,
                                      const gpuntt_modulus64* out_moduli_host, int out_count, uint64_t* qhat_inv,
                                      uint64_t* qhat_inv_shoup, uint64_t* matrix, uint64_t* q_mod_p,
                                      uint64_t* q_inv_mod_p, uint64_t* recip, uint64_t* bit_length);

    /* ---- extension: RNS inner product (InnerProductPlan<T>, include/gpuntt/rns/inner_product.cuh) ----------------
     * moduli_host[mod_count] (q_0 .. q_{M-1}, 1 <= M <= 64) is a HOST array.  workspace_device:
     * gpuntt_innerprod_plan_workspace_bytes_*() bytes of device memory owned by the caller, or NULL (the plan allocates).
     * execute: out[c][r][m][j] = ([accumulate ? out[c][r][m][j] : 0] + sum_{d < digits} a[d][r][m][j] *
     * key[d][c][limb(m)][j]) mod q_m with a = T[digits][count][M][N], out = T[components][count][M][N],
     * key = T[D_key][components][key_mod_count][N] (its first `digits` digits are used), N = 2^n_power, limb(m) =
     * key_limbs_host[m] in [0, key_mod_count) or m when key_limbs_host is NULL (a HOST array of M ints, read before the
     * call returns).  1 <= digits <= 64, 1 <= components <= 4, count >= 0, M <= key_mod_count <= 256.  Any word value is
     * read modulo q_m; every output word is canonical; out must not overlap a or key.  execute allocates nothing, never
     * synchronises and launches one kernel. */
    typedef struct gpuntt_innerprod_plan gpuntt_innerprod_plan;
    int gpuntt_innerprod_plan_workspace_bytes_u32(int mod_count, uint64_t* bytes_host);
    int gpuntt_innerprod_plan_workspace_bytes_u64(int mod_count, uint64_t* bytes_host);
    int gpuntt_innerprod_plan_create_u32(gpuntt_innerprod_plan** plan_host, const gpuntt_modulus32* moduli_host,
                                         int mod_count, void* workspace_device, void* stream);
    int gpuntt_innerprod_plan_create_u64(gpuntt_innerprod_plan** plan_host, const gpuntt_modulus64* moduli_host,
                                         int mod_count, void* workspace_device, void* stream);
    int gpuntt_innerprod_plan_execute_u32(const gpuntt_innerprod_plan* plan, const uint32_t* a, const uint32_t* key,
                                          uint32_t* out, int n_power, int digits, int components, int count,
                                          int accumulate, int key_mod_count, const int* key_limbs_host, void* stream);
    int gpuntt_innerprod_plan_execute_u64(const gpuntt_innerprod_plan* plan, const uint64_t* a, const uint64_t* key,
                                          uint64_t* out, int n_power, int digits, int components, int count,
                                          int accumulate, int key_mod_count, const int* key_limbs_host, void* stream);
    int gpuntt_innerprod_plan_owns_workspace_u32(const gpuntt_innerprod_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_innerprod_plan_owns_workspace_u64(const gpuntt_innerprod_plan* plan);
    int gpuntt_innerprod_plan_destroy_u32(gpuntt_innerprod_plan* plan);
    int gpuntt_innerprod_plan_destroy_u64(gpuntt_innerprod_plan* plan);
    /* host only (no GPU): the folding constants a plan of these moduli uploads, with the checks of plan_create.  Caller
     * arrays of M words: pow_w = 2^W mod q_m, pow_2w = 2^2W mod q_m, the Shoup companions floor(v 2^W / q_m) of both, and
     * one_shoup = floor(2^W / q_m) */
    int gpuntt_innerprod_constants_u32(const gpuntt_modulus32* moduli_host, int mod_count, uint32_t* pow_w,
                                       uint32_t* pow_w_shoup, uint32_t* pow_2w, uint32_t* pow_2w_shoup,
                                       uint32_t* one_shoup);
    int gpuntt_innerprod_constants_u64(const gpuntt_modulus64* moduli_host, int mod_count, uint64_t* pow_w,
                                       uint64_t* pow_w_shoup, uint64_t* pow_2w, uint64_t* pow_2w_shoup,
                                       uint64_t* one_shoup);
    /* host only (no GPU): what execute computes, on HOST arrays in exact integers, after the same argument checks.  The
     * value tests and examples compare the kernel with; never a fall-back */
    int gpuntt_innerprod_reference_u32(const gpuntt_modulus32* moduli_host, int mod_count, const uint32_t* a_host,
                                       const uint32_t* key_host, uint32_t* out_host, int n_power, int digits,
                                       int components, int count, int accumulate, int key_mod_count,
                                       const int* key_limbs_host);
    int gpuntt_innerprod_reference_u64(const gpuntt_modulus64* moduli_host, int mod_count, const uint64_t* a_host,
                                       const uint64_t* key_host, uint64_t* out_host, int n_power, int digits,
                                       int components, int count, int accumulate, int key_mod_count,
                                       const int* key_limbs_host);

    /* ---- extension: hybrid key switching (KeySwitchPlan<T>, include/gpuntt/rns/key_switch.cuh) --------------------
     * q_moduli_host[q_count] (q_0 .. q_{L-1}) and p_moduli_host[p_count] (the special primes p_0 .. p_{K-1}) are HOST
     * arrays, pairwise coprime over the full base {q, p}, M = L + K <= 64; alpha >= 1 is the digit size, D = ceil(L /
     * alpha).  forward_table / inverse_table: DEVICE tables as for gpuntt_ntt_rns_* / gpuntt_intt_rns_*, slot i at
     * i << n_power in full-base order (both NULL: a plan without transforms -- mod_up and mod_down only);
     * mod_inverse_host[M]: n^-1 per modulus.  key_mod_count / key_limbs_host (M ints or NULL) as for
     * gpuntt_innerprod_plan_execute_*.  workspace_device: gpuntt_keyswitch_plan_workspace_bytes_*() bytes owned by the
     * caller, or NULL (the plan allocates).  scratch: gpuntt_keyswitch_plan_scratch_bytes_*() bytes of DEVICE memory
     * owned by the caller, 256-byte aligned (decompose reads it only with input_ntt).
     *   mod_up         in T[count][L][N] -> a T[D][count][M][N]; mode as for gpuntt_baseconv_plan_convert_*; one launch
     *   mod_down       x T[stacks][M][N] -> out T[stacks][L][N] (centred, divided by P); one launch; out must not overlap x
     *   decompose      [INTT of c_in] mod_up (centred), forward NTT of a
     *   switch_digits  inner product of a and key (T[D_key][components][key_mod_count][N]), INTT, mod_down into
     *                  out T[components][count][L][N], [forward NTT of out]
     *   apply          decompose into the scratch, then switch_digits
     *   rotate_hoisted G rotations from one decomposition: a T[D][count][M][N] (what decompose writes), c0 T[count][L][N] in
     *                  NTT form or NULL, keys_host a HOST array of G device pointers (each T[D_key][2][key_mod_count][N]),
     *                  galois_elements_host G odd elements (HOST, reduced as gpuntt_automorphism_ntt_* reduces them),
     *                  1 <= G <= 64, out T[G][2][count][L][N]; the scratch is
     *                  gpuntt_keyswitch_plan_hoisted_scratch_bytes_*() bytes, 256-byte aligned.  One inner product launch
     *                  that applies the permutations while it multiplies, INTT, mod_down, [forward NTT] over the whole
     *                  batch; out[g] equals automorphism + switch_digits + the rotated c0 word for word (key_switch.cuh)
     *   rotate_hoisted_sum  the weighted sum of those G rotations taken before the ModDown: a, c0, keys_host,
     *                  galois_elements_host and G as for rotate_hoisted; weights_host a HOST array of G device pointers or
     *                  NULL (all weights 1), each T[M][N] in NTT form over the plan's full base (any words, read modulo
     *                  q_m) or NULL (weight 1); out T[2][count][L][N]; the scratch is
     *                  gpuntt_keyswitch_plan_hoisted_sum_scratch_bytes_*() bytes (independent of G), 256-byte aligned.  One
     *                  inner product launch, then ONE INTT, mod_down and [forward NTT] over 2 * count stacks; the result
     *                  rounds once and is NOT word for word the weighted sum of rotate_hoisted's outputs (key_switch.cuh)
     *   multiply_relinearize  the product of count pairs of two-component ciphertexts with the top component switched
     *                  under the relinearization key, in ONE key switch: x, y T[2][count][L][N] in NTT form (any words,
     *                  read modulo q_m; y may equal x), key T[D_key][2][key_mod_count][N], out T[2][count][L][N] (may be
     *                  exactly x or exactly y); the scratch is gpuntt_keyswitch_plan_scratch_bytes_*(count, 2) bytes,
     *                  256-byte aligned.  out equals the three pointwise products, apply on x1 y1 and the two additions
     *                  word for word (key_switch.cuh)
     *   multiply_relinearize_sum  sum_t x_t * y_t over `terms` such pairs with ONE key switch and ONE ModDown (lazy
     *                  relinearization): x_host, y_host HOST arrays of `terms` device pointers, 1 <= terms <= 32, each
     *                  T[2][count][L][N] in NTT form (any words; y_host[t] may be x_host[t], a pointer may appear in
     *                  several terms); key, out, count, output_ntt and the scratch as for multiply_relinearize; out may be
     *                  exactly any one of the operands.  out equals the three summed tensor terms, apply on the top one and
     *                  the two additions word for word; with terms = 1 it equals multiply_relinearize; it is NOT word for
     *                  word the sum of `terms` multiply_relinearize results, which round `terms` times (key_switch.cuh)
     * No call allocates or synchronises.
     * host only (no GPU): constants -- arrays_host holds 18 caller arrays in the order of KeySwitchConstants<T>
     * (up_qhat_inv[L], up_qhat_inv_shoup[L], up_matrix[L][M], up_q_mod[D][M], up_recip[L], up_bit_length[L],
     * down_qhat_inv[K], down_qhat_inv_shoup[K], down_matrix[K][L], down_p_mod_q[L], down_p_inv_mod_q[L], down_recip[K],
     * down_bit_length[K], pow_w[M], pow_w_shoup[M], pow_2w[M], pow_2w_shoup[M], one_shoup[M]); reference_mod_up /
     * reference_mod_down -- what mod_up / mod_down compute, on HOST arrays in exact integers after the same argument
     * checks: the value tests and examples compare the kernels with, never a fall-back */
    typedef struct gpuntt_keyswitch_plan gpuntt_keyswitch_plan;
    int gpuntt_keyswitch_plan_workspace_bytes_u32(int q_count, int p_count, int alpha, int n_power, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_scratch_bytes_u32(int q_count, int p_count, int alpha, int n_power, int count,
                                                int components, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_create_u32(gpuntt_keyswitch_plan** plan_host, const gpuntt_modulus32* q_moduli_host, int q_count,
                                         const gpuntt_modulus32* p_moduli_host, int p_count, int alpha, int n_power,
                                         const uint32_t* forward_table, const uint32_t* inverse_table,
                                         const uint32_t* mod_inverse_host, int reduction_poly, int batch_hint,
                                         int key_mod_count, const int* key_limbs_host, void* workspace_device,
                                         void* stream);
    int gpuntt_keyswitch_plan_mod_up_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* in, uint32_t* a, int count, int mode,
                                         void* stream);
    int gpuntt_keyswitch_plan_mod_down_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* x, uint32_t* out, int stacks,
                                           void* stream);
    /* mod_down with an addend (T[stacks][L][N], any word; it may be exactly out): key_switch.cuh, "mod_down_add" */
    int gpuntt_keyswitch_plan_mod_down_add_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* x, const uint32_t* addend, uint32_t* out,
                                               int stacks, void* stream);
    /* the key switch of three-component ciphertexts: c01 = T[2][count][L][N], c2 = T[count][L][N]; key_switch.cuh,
       "relinearize" */
    int gpuntt_keyswitch_plan_relinearize_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* c01, const uint32_t* c2, const uint32_t* key,
                                              uint32_t* out, int count, int input_ntt, int output_ntt, void* scratch,
                                              void* stream);
    int gpuntt_keyswitch_plan_decompose_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* c_in, uint32_t* a, int count,
                                            int input_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_switch_digits_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* a, const uint32_t* key,
                                                uint32_t* out, int count, int components, int output_ntt, void* scratch,
                                                void* stream);
    int gpuntt_keyswitch_plan_apply_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* c_in, const uint32_t* key, uint32_t* out,
                                        int count, int components, int input_ntt, int output_ntt, void* scratch,
                                        void* stream);
    int gpuntt_keyswitch_plan_hoisted_scratch_bytes_u32(int q_count, int p_count, int alpha, int n_power, int count,
                                                        int elements, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_rotate_hoisted_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* a, const uint32_t* c0,
                                                 const uint32_t* const* keys_host, const uint32_t* galois_elements_host,
                                                 int elements, uint32_t* out, int count, int output_ntt, void* scratch,
                                                 void* stream);
    int gpuntt_keyswitch_plan_hoisted_sum_scratch_bytes_u32(int q_count, int p_count, int alpha, int n_power, int count,
                                                            uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_rotate_hoisted_sum_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* a, const uint32_t* c0,
                                                     const uint32_t* const* keys_host, const uint32_t* galois_elements_host,
                                                     const uint32_t* const* weights_host, int elements, uint32_t* out,
                                                     int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* x, const uint32_t* y,
                                                       const uint32_t* key, uint32_t* out, int count, int output_ntt,
                                                       void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_sum_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* const* x_host,
                                                           const uint32_t* const* y_host, int terms, const uint32_t* key,
                                                           uint32_t* out, int count, int output_ntt, void* scratch,
                                                           void* stream);
    int gpuntt_keyswitch_plan_owns_workspace_u32(const gpuntt_keyswitch_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_keyswitch_plan_destroy_u32(gpuntt_keyswitch_plan* plan);
    int gpuntt_keyswitch_constants_u32(const gpuntt_modulus32* q_moduli_host, int q_count, const gpuntt_modulus32* p_moduli_host, int p_count,
                                       int alpha, uint32_t* const* arrays_host);
    int gpuntt_keyswitch_reference_mod_up_u32(const gpuntt_modulus32* q_moduli_host, int q_count, const gpuntt_modulus32* p_moduli_host,
                                              int p_count, int alpha, const uint32_t* in_host, uint32_t* a_host, int n_power,
                                              int count, int mode);
    int gpuntt_keyswitch_reference_mod_down_u32(const gpuntt_modulus32* q_moduli_host, int q_count, const gpuntt_modulus32* p_moduli_host,
                                                int p_count, const uint32_t* x_host, uint32_t* out_host, int n_power, int stacks);
    int gpuntt_keyswitch_plan_workspace_bytes_u64(int q_count, int p_count, int alpha, int n_power, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_scratch_bytes_u64(int q_count, int p_count, int alpha, int n_power, int count,
                                                int components, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_create_u64(gpuntt_keyswitch_plan** plan_host, const gpuntt_modulus64* q_moduli_host, int q_count,
                                         const gpuntt_modulus64* p_moduli_host, int p_count, int alpha, int n_power,
                                         const uint64_t* forward_table, const uint64_t* inverse_table,
                                         const uint64_t* mod_inverse_host, int reduction_poly, int batch_hint,
                                         int key_mod_count, const int* key_limbs_host, void* workspace_device,
                                         void* stream);
    int gpuntt_keyswitch_plan_mod_up_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* in, uint64_t* a, int count, int mode,
                                         void* stream);
    int gpuntt_keyswitch_plan_mod_down_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* x, uint64_t* out, int stacks,
                                           void* stream);
    /* mod_down with an addend (T[stacks][L][N], any word; it may be exactly out): key_switch.cuh, "mod_down_add" */
    int gpuntt_keyswitch_plan_mod_down_add_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* x, const uint64_t* addend, uint64_t* out,
                                               int stacks, void* stream);
    /* the key switch of three-component ciphertexts: c01 = T[2][count][L][N], c2 = T[count][L][N]; key_switch.cuh,
       "relinearize" */
    int gpuntt_keyswitch_plan_relinearize_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* c01, const uint64_t* c2, const uint64_t* key,
                                              uint64_t* out, int count, int input_ntt, int output_ntt, void* scratch,
                                              void* stream);
    int gpuntt_keyswitch_plan_decompose_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* c_in, uint64_t* a, int count,
                                            int input_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_switch_digits_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* a, const uint64_t* key,
                                                uint64_t* out, int count, int components, int output_ntt, void* scratch,
                                                void* stream);
    int gpuntt_keyswitch_plan_apply_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* c_in, const uint64_t* key, uint64_t* out,
                                        int count, int components, int input_ntt, int output_ntt, void* scratch,
                                        void* stream);
    int gpuntt_keyswitch_plan_hoisted_scratch_bytes_u64(int q_count, int p_count, int alpha, int n_power, int count,
                                                        int elements, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_rotate_hoisted_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* a, const uint64_t* c0,
                                                 const uint64_t* const* keys_host, const uint32_t* galois_elements_host,
                                                 int elements, uint64_t* out, int count, int output_ntt, void* scratch,
                                                 void* stream);
    int gpuntt_keyswitch_plan_hoisted_sum_scratch_bytes_u64(int q_count, int p_count, int alpha, int n_power, int count,
                                                            uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_rotate_hoisted_sum_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* a, const uint64_t* c0,
                                                     const uint64_t* const* keys_host, const uint32_t* galois_elements_host,
                                                     const uint64_t* const* weights_host, int elements, uint64_t* out,
                                                     int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* x, const uint64_t* y,
                                                       const uint64_t* key, uint64_t* out, int count, int output_ntt,
                                                       void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_sum_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* const* x_host,
                                                           const uint64_t* const* y_host, int terms, const uint64_t* key,
                                                           uint64_t* out, int count, int output_ntt, void* scratch,
                                                           void* stream);
    int gpuntt_keyswitch_plan_owns_workspace_u64(const gpuntt_keyswitch_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_keyswitch_plan_destroy_u64(gpuntt_keyswitch_plan* plan);
    int gpuntt_keyswitch_constants_u64(const gpuntt_modulus64* q_moduli_host, int q_count, const gpuntt_modulus64* p_moduli_host, int p_count,
                                       int alpha, uint64_t* const* arrays_host);
    int gpuntt_keyswitch_reference_mod_up_u64(const gpuntt_modulus64* q_moduli_host, int q_count, const gpuntt_modulus64* p_moduli_host,
                                              int p_count, int alpha, const uint64_t* in_host, uint64_t* a_host, int n_power,
                                              int count, int mode);
    int gpuntt_keyswitch_reference_mod_down_u64(const gpuntt_modulus64* q_moduli_host, int q_count, const gpuntt_modulus64* p_moduli_host,
                                                int p_count, const uint64_t* x_host, uint64_t* out_host, int n_power, int stacks);

    /* ---- extension: rescaling inside the key switching plan (include/gpuntt/rns/key_switch.cuh, "Rescaling") --------
     * create_rescale / workspace_bytes_rescale: gpuntt_keyswitch_plan_create_* / _workspace_bytes_* with
     * rescale_limbs = R, 0 <= R <= L - 1 (R = 0: exactly the plan and the bytes of the functions above; R > 0: two more
     * constants images and, with transforms, two more transform plans -- two more host waits at creation).  Every call
     * below returns an error on a plan with R = 0.  L' = L - R.
     *   mod_down_rescale  x T[stacks][M][N] -> out T[stacks][L'][N]: centred, divided by P q_{L-R} ... q_{L-1} with one
     *                  rounding; one launch; out must not overlap x
     *   rescale        x T[stacks][L][N] (q-base, any words) -> out T[stacks][L'][N], divided by q_{L-R} ... q_{L-1}.
     *                  ntt_form 0: coefficient form, one launch, scratch unused (NULL).  ntt_form 1: x and out in NTT
     *                  form; scratch gpuntt_keyswitch_plan_rescale_scratch_bytes_*() bytes, 256-byte aligned; only the R
     *                  dropped limbs are inverse-transformed.  out must not overlap x or the scratch
     *   multiply_relinearize_rescale, multiply_relinearize_sum_rescale, rotate_hoisted_sum_rescale  the calls without the
     *                  suffix with mod_down_rescale as their ModDown: out T[2][count][L'][N], rounded ONCE -- within 1 per
     *                  coefficient of the call followed by rescale, not word for word equal to it (key_switch.cuh)
     * host only (no GPU): reference_mod_down_rescale / reference_rescale (coefficient form), R in [1, L - 1] */
    int gpuntt_keyswitch_plan_workspace_bytes_rescale_u32(int q_count, int p_count, int alpha, int n_power, int rescale_limbs,
                                                          uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_create_rescale_u32(gpuntt_keyswitch_plan** plan_host, const gpuntt_modulus32* q_moduli_host,
                                                 int q_count, const gpuntt_modulus32* p_moduli_host, int p_count, int alpha,
                                                 int n_power, const uint32_t* forward_table, const uint32_t* inverse_table,
                                                 const uint32_t* mod_inverse_host, int reduction_poly, int batch_hint,
                                                 int key_mod_count, const int* key_limbs_host, int rescale_limbs,
                                                 void* workspace_device, void* stream);
    int gpuntt_keyswitch_plan_rescale_limbs_u32(const gpuntt_keyswitch_plan* plan); /* R, negative on error */
    int gpuntt_keyswitch_plan_rescale_scratch_bytes_u32(const gpuntt_keyswitch_plan* plan, int stacks, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_mod_down_rescale_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* x, uint32_t* out,
                                                   int stacks, void* stream);
    int gpuntt_keyswitch_plan_rescale_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* x, uint32_t* out, int stacks,
                                          int ntt_form, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_rescale_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* x,
                                                               const uint32_t* y, const uint32_t* key, uint32_t* out,
                                                               int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_sum_rescale_u32(const gpuntt_keyswitch_plan* plan,
                                                                   const uint32_t* const* x_host,
                                                                   const uint32_t* const* y_host, int terms,
                                                                   const uint32_t* key, uint32_t* out, int count,
                                                                   int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_rotate_hoisted_sum_rescale_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* a,
                                                             const uint32_t* c0, const uint32_t* const* keys_host,
                                                             const uint32_t* galois_elements_host,
                                                             const uint32_t* const* weights_host, int elements,
                                                             uint32_t* out, int count, int output_ntt, void* scratch,
                                                             void* stream);
    int gpuntt_keyswitch_reference_mod_down_rescale_u32(const gpuntt_modulus32* q_moduli_host, int q_count,
                                                        const gpuntt_modulus32* p_moduli_host, int p_count,
                                                        int rescale_limbs, const uint32_t* x_host, uint32_t* out_host,
                                                        int n_power, int stacks);
    int gpuntt_keyswitch_reference_rescale_u32(const gpuntt_modulus32* q_moduli_host, int q_count, int rescale_limbs,
                                               const uint32_t* x_host, uint32_t* out_host, int n_power, int stacks);
    int gpuntt_keyswitch_plan_workspace_bytes_rescale_u64(int q_count, int p_count, int alpha, int n_power, int rescale_limbs,
                                                          uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_create_rescale_u64(gpuntt_keyswitch_plan** plan_host, const gpuntt_modulus64* q_moduli_host,
                                                 int q_count, const gpuntt_modulus64* p_moduli_host, int p_count, int alpha,
                                                 int n_power, const uint64_t* forward_table, const uint64_t* inverse_table,
                                                 const uint64_t* mod_inverse_host, int reduction_poly, int batch_hint,
                                                 int key_mod_count, const int* key_limbs_host, int rescale_limbs,
                                                 void* workspace_device, void* stream);
    int gpuntt_keyswitch_plan_rescale_limbs_u64(const gpuntt_keyswitch_plan* plan); /* R, negative on error */
    int gpuntt_keyswitch_plan_rescale_scratch_bytes_u64(const gpuntt_keyswitch_plan* plan, int stacks, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_mod_down_rescale_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* x, uint64_t* out,
                                                   int stacks, void* stream);
    int gpuntt_keyswitch_plan_rescale_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* x, uint64_t* out, int stacks,
                                          int ntt_form, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_rescale_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* x,
                                                               const uint64_t* y, const uint64_t* key, uint64_t* out,
                                                               int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_multiply_relinearize_sum_rescale_u64(const gpuntt_keyswitch_plan* plan,
                                                                   const uint64_t* const* x_host,
                                                                   const uint64_t* const* y_host, int terms,
                                                                   const uint64_t* key, uint64_t* out, int count,
                                                                   int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_rotate_hoisted_sum_rescale_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* a,
                                                             const uint64_t* c0, const uint64_t* const* keys_host,
                                                             const uint32_t* galois_elements_host,
                                                             const uint64_t* const* weights_host, int elements,
                                                             uint64_t* out, int count, int output_ntt, void* scratch,
                                                             void* stream);
    int gpuntt_keyswitch_reference_mod_down_rescale_u64(const gpuntt_modulus64* q_moduli_host, int q_count,
                                                        const gpuntt_modulus64* p_moduli_host, int p_count,
                                                        int rescale_limbs, const uint64_t* x_host, uint64_t* out_host,
                                                        int n_power, int stacks);
    int gpuntt_keyswitch_reference_rescale_u64(const gpuntt_modulus64* q_moduli_host, int q_count, int rescale_limbs,
                                               const uint64_t* x_host, uint64_t* out_host, int n_power, int stacks);

    /* ---- KeySwitchPlan<T>::linear_transform_bsgs: the double-hoisted baby-step/giant-step linear transform ----
     * out = sum_g sigma_{k_g}( sum_b pt_{g,b} (.) sigma_{k_b}(ct) ): the diagonal is applied BEFORE the giant rotation.
     *   a T[D][count][M][N] (what decompose writes), c0 / c1 T[count][L][N] in NTT form (c0 may be NULL; c1 is needed
     *   only if a baby key is NULL); baby_keys_host / giant_keys_host HOST arrays of n1 / n2 device pointers, a NULL key
     *   = no key switch for that step, accepted only where the reduced element is 1; weights_host a HOST array of
     *   n2 * n1 device pointers, row-major [g][b], each T[M][N] in NTT form over the full base -- a NULL entry means the
     *   term is ABSENT (weight 0), unlike rotate_hoisted_sum, where NULL means 1; every giant row needs one present
     *   weight.  1 <= n1, n2 <= 64, n1 * n2 <= 256.  out T[2][count][L][N] (L' with _rescale, a plan with R > 0).  The
     *   scratch is gpuntt_keyswitch_plan_bsgs_scratch_bytes_*() bytes, 256-byte aligned.  n1 + n2 keys, ONE final ModDown;
     *   every word equals the composition of the existing calls that key_switch.cuh defines */
    int gpuntt_keyswitch_plan_bsgs_scratch_bytes_u32(int q_count, int p_count, int alpha, int n_power, int count, int n1,
                                                     int n2, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_bsgs_scratch_bytes_u64(int q_count, int p_count, int alpha, int n_power, int count, int n1,
                                                     int n2, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_linear_transform_bsgs_u32(
        const gpuntt_keyswitch_plan* plan, const uint32_t* a, const uint32_t* c0, const uint32_t* c1,
        const uint32_t* const* baby_keys_host, const uint32_t* baby_elements_host, int n1,
        const uint32_t* const* giant_keys_host, const uint32_t* giant_elements_host, int n2,
        const uint32_t* const* weights_host, uint32_t* out, int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_linear_transform_bsgs_u64(
        const gpuntt_keyswitch_plan* plan, const uint64_t* a, const uint64_t* c0, const uint64_t* c1,
        const uint64_t* const* baby_keys_host, const uint32_t* baby_elements_host, int n1,
        const uint64_t* const* giant_keys_host, const uint32_t* giant_elements_host, int n2,
        const uint64_t* const* weights_host, uint64_t* out, int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_linear_transform_bsgs_rescale_u32(
        const gpuntt_keyswitch_plan* plan, const uint32_t* a, const uint32_t* c0, const uint32_t* c1,
        const uint32_t* const* baby_keys_host, const uint32_t* baby_elements_host, int n1,
        const uint32_t* const* giant_keys_host, const uint32_t* giant_elements_host, int n2,
        const uint32_t* const* weights_host, uint32_t* out, int count, int output_ntt, void* scratch, void* stream);
    int gpuntt_keyswitch_plan_linear_transform_bsgs_rescale_u64(
        const gpuntt_keyswitch_plan* plan, const uint64_t* a, const uint64_t* c0, const uint64_t* c1,
        const uint64_t* const* baby_keys_host, const uint32_t* baby_elements_host, int n1,
        const uint64_t* const* giant_keys_host, const uint32_t* giant_elements_host, int n2,
        const uint64_t* const* weights_host, uint64_t* out, int count, int output_ntt, void* scratch, void* stream);

    /* ---- extension: scale-invariant ciphertext multiplication (BfvMultiplyPlan<T>, include/gpuntt/rns/bfv_multiply.cuh) ----
     * round(t (x (x) y) / Q) for the q-base q_moduli_host (L), the auxiliary base b_moduli_host (K, B = prod b_j >=
     * 2 t N Q or GPUNTT_ERR_INVALID_ARGUMENT "Auxiliary base too small!") and the plaintext modulus t >= 2; the full base
     * is {q.., b..}, M = L + K <= 64.  forward_table / inverse_table / mod_inverse_host, reduction_poly, batch_hint and
     * workspace_device as for gpuntt_keyswitch_plan_create_* (tables over the full base; all three NULL: a plan without
     * transforms, extend and scale_round only); the workspace is gpuntt_bfv_plan_workspace_bytes_*() bytes.
     *   extend       in T[stacks][L][N] (coefficient form, any words) -> full T[stacks][M][N]: the q-limbs reduced, the
     *                b-limbs word for word the centred gpuntt_baseconv_plan_convert_* of {q} -> {b}; one kernel launch
     *   scale_round  full T[stacks][M][N] (coefficient form, any words) -> out T[stacks][L][N]: every limb times t, the
     *                centred convert_and_divide {q} -> {b}, the centred convert {b} -> {q}, word for word; one launch
     *   multiply     x, y T[2][count][L][N] (y may be x) -> out T[3][count][L][N], the three components of the product;
     *                input_ntt / output_ntt: the operands / the result are in NTT form over the q-base (operands in NTT
     *                form are canonical residues; in coefficient form any word is read modulo its q).  The scratch is
     *                gpuntt_bfv_plan_scratch_bytes_*() bytes, 256-byte aligned, owned by the caller; out may be exactly x
     *                or exactly y.  out[2] is the c_in of gpuntt_keyswitch_plan_apply_* (components = 2) for
     *                relinearization
     * No call allocates or synchronises.
     * host only (no GPU): constants -- arrays_host holds 18 caller arrays in the order of BfvConstants<T>: the seven of
     * gpuntt_baseconv_constants_* for {q} -> {b} (qhat_inv[L], qhat_inv_shoup[L], matrix[L][K], q_mod_p[K],
     * q_inv_mod_p[K], recip[L], bit_length[L]), the same seven for {b} -> {q}, then t_mod[M], t_mod_shoup[M],
     * t_qhat_inv[L], t_qhat_inv_shoup[L]; reference_extend / reference_scale_round -- what extend / scale_round compute,
     * on HOST arrays in exact integers after the same argument checks: what tests and examples compare the kernels with,
     * never a fall-back */
    typedef struct gpuntt_bfv_plan gpuntt_bfv_plan;
    int gpuntt_bfv_plan_workspace_bytes_u32(int q_count, int b_count, int n_power, uint64_t* bytes_host);
    int gpuntt_bfv_plan_workspace_bytes_u64(int q_count, int b_count, int n_power, uint64_t* bytes_host);
    int gpuntt_bfv_plan_scratch_bytes_u32(int q_count, int b_count, int n_power, int count, uint64_t* bytes_host);
    int gpuntt_bfv_plan_scratch_bytes_u64(int q_count, int b_count, int n_power, int count, uint64_t* bytes_host);
    int gpuntt_bfv_plan_create_u32(gpuntt_bfv_plan** plan_host, const gpuntt_modulus32* q_moduli_host, int q_count,
                                   const gpuntt_modulus32* b_moduli_host, int b_count, uint32_t plain_modulus, int n_power,
                                   const uint32_t* forward_table, const uint32_t* inverse_table,
                                   const uint32_t* mod_inverse_host, int reduction_poly, int batch_hint,
                                   void* workspace_device, void* stream);
    int gpuntt_bfv_plan_create_u64(gpuntt_bfv_plan** plan_host, const gpuntt_modulus64* q_moduli_host, int q_count,
                                   const gpuntt_modulus64* b_moduli_host, int b_count, uint64_t plain_modulus, int n_power,
                                   const uint64_t* forward_table, const uint64_t* inverse_table,
                                   const uint64_t* mod_inverse_host, int reduction_poly, int batch_hint,
                                   void* workspace_device, void* stream);
    int gpuntt_bfv_plan_extend_u32(const gpuntt_bfv_plan* plan, const uint32_t* in, uint32_t* full, int stacks, void* stream);
    int gpuntt_bfv_plan_extend_u64(const gpuntt_bfv_plan* plan, const uint64_t* in, uint64_t* full, int stacks, void* stream);
    int gpuntt_bfv_plan_scale_round_u32(const gpuntt_bfv_plan* plan, const uint32_t* full, uint32_t* out, int stacks,
                                        void* stream);
    int gpuntt_bfv_plan_scale_round_u64(const gpuntt_bfv_plan* plan, const uint64_t* full, uint64_t* out, int stacks,
                                        void* stream);
    int gpuntt_bfv_plan_multiply_u32(const gpuntt_bfv_plan* plan, const uint32_t* x, const uint32_t* y, uint32_t* out,
                                     int count, int input_ntt, int output_ntt, void* scratch, void* stream);
    int gpuntt_bfv_plan_multiply_u64(const gpuntt_bfv_plan* plan, const uint64_t* x, const uint64_t* y, uint64_t* out,
                                     int count, int input_ntt, int output_ntt, void* scratch, void* stream);
    /* BFV ct x ct, relinearized, in one call: out = T[2][count][L][N]; key_switch_scratch is the key-switching plan's
       scratch_bytes(count, 2); bfv_multiply.cuh, "multiply_relinearize" */
    int gpuntt_bfv_plan_multiply_relinearize_u32(const gpuntt_bfv_plan* plan, const uint32_t* x, const uint32_t* y,
                                                 const gpuntt_keyswitch_plan* key_switch, const uint32_t* key, uint32_t* out,
                                                 int count, int input_ntt, int output_ntt, void* scratch,
                                                 void* key_switch_scratch, void* stream);
    int gpuntt_bfv_plan_owns_workspace_u32(const gpuntt_bfv_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_bfv_plan_owns_workspace_u64(const gpuntt_bfv_plan* plan);
    /* BFV ct x ct, relinearized, in one call: out = T[2][count][L][N]; key_switch_scratch is the key-switching plan's
       scratch_bytes(count, 2); bfv_multiply.cuh, "multiply_relinearize" */
    int gpuntt_bfv_plan_multiply_relinearize_u64(const gpuntt_bfv_plan* plan, const uint64_t* x, const uint64_t* y,
                                                 const gpuntt_keyswitch_plan* key_switch, const uint64_t* key, uint64_t* out,
                                                 int count, int input_ntt, int output_ntt, void* scratch,
                                                 void* key_switch_scratch, void* stream);
    /* sum_t x_t * y_t over `terms` pairs with ONE division by Q (bfv_multiply.cuh, "multiply_sum"): x_host, y_host are
       HOST arrays of `terms` device pointers, each T[2][count][L][N]; y[t] may be x[t] and a pointer may appear in several
       terms -- every distinct pointer is extended and transformed once.  1 <= terms <= 32 and terms <= max_terms
       (min(32, floor(B / (2 t N Q))); returned by gpuntt_bfv_plan_max_terms_*, negative on error).  The scratch is
       gpuntt_bfv_plan_sum_scratch_bytes_*(.., count, operands) bytes for operands >= the number of distinct pointers,
       256-byte aligned.  multiply_sum: out = T[3][count][L][N]; multiply_relinearize_sum: out = T[2][count][L][N], with
       ONE key switch and ONE ModDown.  With terms = 1 they return the words of multiply / multiply_relinearize; with
       more terms they round once where `terms` separate calls round `terms` times */
    int gpuntt_bfv_plan_max_terms_u32(const gpuntt_bfv_plan* plan);
    int gpuntt_bfv_plan_max_terms_u64(const gpuntt_bfv_plan* plan);
    /* host only (no GPU): what gpuntt_bfv_plan_max_terms_* of a plan of these bases returns, with the checks of create */
    int gpuntt_bfv_max_terms_u32(const gpuntt_modulus32* q_moduli_host, int q_count, const gpuntt_modulus32* b_moduli_host,
                                 int b_count, uint32_t plain_modulus, int n_power, int* terms_host);
    int gpuntt_bfv_max_terms_u64(const gpuntt_modulus64* q_moduli_host, int q_count, const gpuntt_modulus64* b_moduli_host,
                                 int b_count, uint64_t plain_modulus, int n_power, int* terms_host);
    int gpuntt_bfv_plan_sum_scratch_bytes_u32(int q_count, int b_count, int n_power, int count, int operands,
                                              uint64_t* bytes_host);
    int gpuntt_bfv_plan_sum_scratch_bytes_u64(int q_count, int b_count, int n_power, int count, int operands,
                                              uint64_t* bytes_host);
    int gpuntt_bfv_plan_multiply_sum_u32(const gpuntt_bfv_plan* plan, const uint32_t* const* x_host,
                                         const uint32_t* const* y_host, int terms, uint32_t* out, int count, int input_ntt,
                                         int output_ntt, void* scratch, void* stream);
    int gpuntt_bfv_plan_multiply_sum_u64(const gpuntt_bfv_plan* plan, const uint64_t* const* x_host,
                                         const uint64_t* const* y_host, int terms, uint64_t* out, int count, int input_ntt,
                                         int output_ntt, void* scratch, void* stream);
    int gpuntt_bfv_plan_multiply_relinearize_sum_u32(const gpuntt_bfv_plan* plan, const uint32_t* const* x_host,
                                                     const uint32_t* const* y_host, int terms,
                                                     const gpuntt_keyswitch_plan* key_switch, const uint32_t* key,
                                                     uint32_t* out, int count, int input_ntt, int output_ntt,
                                                     void* scratch, void* key_switch_scratch, void* stream);
    int gpuntt_bfv_plan_multiply_relinearize_sum_u64(const gpuntt_bfv_plan* plan, const uint64_t* const* x_host,
                                                     const uint64_t* const* y_host, int terms,
                                                     const gpuntt_keyswitch_plan* key_switch, const uint64_t* key,
                                                     uint64_t* out, int count, int input_ntt, int output_ntt,
                                                     void* scratch, void* key_switch_scratch, void* stream);
    int gpuntt_bfv_plan_destroy_u32(gpuntt_bfv_plan* plan);
    int gpuntt_bfv_plan_destroy_u64(gpuntt_bfv_plan* plan);
    int gpuntt_bfv_constants_u32(const gpuntt_modulus32* q_moduli_host, int q_count, const gpuntt_modulus32* b_moduli_host,
                                 int b_count, uint32_t plain_modulus, int n_power, uint32_t* const* arrays_host);
    int gpuntt_bfv_constants_u64(const gpuntt_modulus64* q_moduli_host, int q_count, const gpuntt_modulus64* b_moduli_host,
                                 int b_count, uint64_t plain_modulus, int n_power, uint64_t* const* arrays_host);
    int gpuntt_bfv_reference_extend_u32(const gpuntt_modulus32* q_moduli_host, int q_count,
                                        const gpuntt_modulus32* b_moduli_host, int b_count, const uint32_t* in_host,
                                        uint32_t* full_host, int n_power, int stacks);
    int gpuntt_bfv_reference_extend_u64(const gpuntt_modulus64* q_moduli_host, int q_count,
                                        const gpuntt_modulus64* b_moduli_host, int b_count, const uint64_t* in_host,
                                        uint64_t* full_host, int n_power, int stacks);
    int gpuntt_bfv_reference_scale_round_u32(const gpuntt_modulus32* q_moduli_host, int q_count,
                                             const gpuntt_modulus32* b_moduli_host, int b_count, uint32_t plain_modulus,
                                             const uint32_t* full_host, uint32_t* out_host, int n_power, int stacks);
    int gpuntt_bfv_reference_scale_round_u64(const gpuntt_modulus64* q_moduli_host, int q_count,
                                             const gpuntt_modulus64* b_moduli_host, int b_count, uint64_t plain_modulus,
                                             const uint64_t* full_host, uint64_t* out_host, int n_power, int stacks);

    /* ---- extension: prepared 4-step transforms (FourStepPlan<T>, include/gpuntt/ntt_4step/ntt_4step.cuh) ----
     * The Shoup pairs of the n1 / n2 / W tables are derived once, at creation, into workspace_device
     * (gpuntt_4step_plan_workspace_bytes_*() bytes owned by the caller) or a buffer the plan allocates (NULL).
     * natural_order 0: execute == gpuntt_4step_* (n2 x n1 in, n1 x n2 out); 1: == gpuntt_4step_natural_* (`in` is
     * scratch).  in != out.  Creation runs on `stream`; execute allocates nothing and never synchronises. */
    typedef struct gpuntt_4step_plan gpuntt_4step_plan;
    int gpuntt_4step_plan_workspace_bytes_u32(int n_power, uint64_t* bytes_host);
    int gpuntt_4step_plan_workspace_bytes_u64(int n_power, uint64_t* bytes_host);
    int gpuntt_4step_plan_create_u32(gpuntt_4step_plan** plan_host, const uint32_t* n1_table, const uint32_t* n2_table,
                                     const uint32_t* w_table, gpuntt_modulus32 modulus, int n_power, int ntt_type,
                                     uint32_t mod_inverse, int natural_order, int batch_hint, void* workspace_device,
                                     void* stream);
    int gpuntt_4step_plan_create_u64(gpuntt_4step_plan** plan_host, const uint64_t* n1_table, const uint64_t* n2_table,
                                     const uint64_t* w_table, gpuntt_modulus64 modulus, int n_power, int ntt_type,
                                     uint64_t mod_inverse, int natural_order, int batch_hint, void* workspace_device,
                                     void* stream);
    int gpuntt_4step_plan_execute_u32(const gpuntt_4step_plan* plan, uint32_t* in, uint32_t* out, int batch_size,
                                      void* stream);
    int gpuntt_4step_plan_execute_u64(const gpuntt_4step_plan* plan, uint64_t* in, uint64_t* out, int batch_size,
                                      void* stream);
    int gpuntt_4step_plan_fast_path_u32(const gpuntt_4step_plan* plan); /* 1 / 0, negative on error */
    int gpuntt_4step_plan_fast_path_u64(const gpuntt_4step_plan* plan);
    int gpuntt_4step_plan_destroy_u32(gpuntt_4step_plan* plan);
    int gpuntt_4step_plan_destroy_u64(gpuntt_4step_plan* plan);

    /* ---- extension: root-of-unity tables built on the device (include/gpuntt/common/parameter_sets.hpp) ----
     * power table: out[k] = base^(bit_reversed ? bitreverse(k, log_count) : k), k < 2^log_count (log_count <= 28) --
     * with bit_reversed = 1 the device-order table GPU_NTT / GPU_INTT / the 4-step n1, n2 slots take;
     * 4-step W:  GPUNTT_FORWARD W[i*n2+j] = root^(bitreverse(i, log n1) * j), GPUNTT_INVERSE root^(bitreverse(j, log n2) * i)
     * (pass the inverse root), N = 2^n_power entries, 12 <= n_power <= 24.  Replaces the host loops of the
     * reference's src/lib/common/nttparameters.cu:356-444 and the upload. */
    int gpuntt_generate_power_table_u32(uint32_t* out, uint32_t base, gpuntt_modulus32 modulus, int log_count,
                                        int bit_reversed, void* stream);
    int gpuntt_generate_power_table_u64(uint64_t* out, uint64_t base, gpuntt_modulus64 modulus, int log_count,
                                        int bit_reversed, void* stream);
    int gpuntt_generate_4step_w_u32(uint32_t* out, uint32_t root, gpuntt_modulus32 modulus, int n_power, int ntt_type,
                                    void* stream);
    int gpuntt_generate_4step_w_u64(uint64_t* out, uint64_t root, gpuntt_modulus64 modulus, int n_power, int ntt_type,
                                    void* stream);

    /* ---- counter-based samplers (include/gpuntt/rns/sampling.cuh) -- NOT a cryptographic generator: tests, benchmarks
     * and reproducible experiments.  Every word is a pure function of (seed, stream_id, word index).
     *   philox4x32_10: the standard Philox4x32 with ten rounds, on the host.
     *   sample_uniform: out T[stacks][mod_count][N] on the device, stack s at s * stack_stride_words (>= mod_count * N),
     *     moduli_host mod_count HOST values (1 .. 256 of them, none 0); bounded rejection over 32 candidates.
     *   sample_small: out int32[polys][N] on the device; distribution GPUNTT_SAMPLE_TERNARY (uniform on -1, 0, 1) or
     *     GPUNTT_SAMPLE_CBD21 (centred binomial, variance 10.5).
     *   sample_reference_*: the same words on HOST arrays (no GPU); max_candidates >= 1 (the device uses 32). */
#define GPUNTT_SAMPLE_TERNARY 0
#define GPUNTT_SAMPLE_CBD21 1
    int gpuntt_philox4x32_10(const uint32_t* ctr4_host, const uint32_t* key2_host, uint32_t* out4_host);
    int gpuntt_sample_uniform_u32(uint32_t* out, const uint32_t* moduli_host, int mod_count, int n_power, int stacks,
                                  uint64_t stack_stride_words, uint64_t seed, uint32_t stream_id, void* stream);
    int gpuntt_sample_uniform_u64(uint64_t* out, const uint64_t* moduli_host, int mod_count, int n_power, int stacks,
                                  uint64_t stack_stride_words, uint64_t seed, uint32_t stream_id, void* stream);
    int gpuntt_sample_small(int32_t* out, int polys, int n_power, int distribution, uint64_t seed, uint32_t stream_id,
                            void* stream);
    int gpuntt_sample_reference_uniform_u32(uint32_t* out_host, const uint32_t* moduli_host, int mod_count, int n_power,
                                            int stacks, uint64_t stack_stride_words, uint64_t seed, uint32_t stream_id,
                                            int max_candidates);
    int gpuntt_sample_reference_uniform_u64(uint64_t* out_host, const uint64_t* moduli_host, int mod_count, int n_power,
                                            int stacks, uint64_t stack_stride_words, uint64_t seed, uint32_t stream_id,
                                            int max_candidates);
    int gpuntt_sample_reference_small(int32_t* out_host, int polys, int n_power, int distribution, uint64_t seed,
                                      uint32_t stream_id);

    /* ---- KeySwitchPlan<T>: key material (include/gpuntt/rns/key_switch.cuh, "Key material") ----
     *   lift_small: small int32[polys][N] -> out T[polys][M or L][N], the canonical residues; to_ntt: the plan's forward
     *     transform over that base follows in place.
     *   generate_keys: s T[M][N] and s_from T[keys][M][N] in NTT form over the full base, errors int32[keys][D][N],
     *     keys_host a HOST array of `keys` (0 .. 64) device pointers, each T[D][2][M][N] with component 1 = a on entry;
     *     component 0 = E - a s + P g_d s_from is written.  The scratch is keygen_scratch_bytes bytes, 256-byte aligned.
     *   encrypt_symmetric: out T[2][count][L][N] with out[1] = a on entry; out[0] = E - a s + message is written; message
     *     T[count][L][N] in NTT form or NULL; errors int32[count][N].  The scratch is encrypt_scratch_bytes bytes. */
    int gpuntt_keyswitch_plan_lift_small_u32(const gpuntt_keyswitch_plan* plan, const int32_t* small, uint32_t* out,
                                             int polys, int full_base, int to_ntt, void* stream);
    int gpuntt_keyswitch_plan_lift_small_u64(const gpuntt_keyswitch_plan* plan, const int32_t* small, uint64_t* out,
                                             int polys, int full_base, int to_ntt, void* stream);
    int gpuntt_keyswitch_plan_keygen_scratch_bytes_u32(const gpuntt_keyswitch_plan* plan, int keys, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_keygen_scratch_bytes_u64(const gpuntt_keyswitch_plan* plan, int keys, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_encrypt_scratch_bytes_u32(const gpuntt_keyswitch_plan* plan, int count, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_encrypt_scratch_bytes_u64(const gpuntt_keyswitch_plan* plan, int count, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_generate_keys_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* s, const uint32_t* s_from,
                                                const int32_t* errors, uint32_t* const* keys_host, int keys, void* scratch,
                                                void* stream);
    int gpuntt_keyswitch_plan_generate_keys_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* s, const uint64_t* s_from,
                                                const int32_t* errors, uint64_t* const* keys_host, int keys, void* scratch,
                                                void* stream);
    int gpuntt_keyswitch_plan_encrypt_symmetric_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* s,
                                                    const int32_t* errors, const uint32_t* message, uint32_t* out, int count,
                                                    void* scratch, void* stream);
    int gpuntt_keyswitch_plan_encrypt_symmetric_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* s,
                                                    const int32_t* errors, const uint64_t* message, uint64_t* out, int count,
                                                    void* scratch, void* stream);

    /* ---- decryption and public-key encryption (key_switch.cuh, "Decryption and public-key encryption";
     *      bfv_multiply.cuh, "Reading a result back") ----
     *   phase: ct T[components][count][L][N] (components 2 or 3), s T[M][N] in NTT form, out T[count][L][N] =
     *     c0 + c1 s [+ c2 s^2]; the scratch is phase_scratch_bytes bytes (0 and NULL accepted for NTT-form input).
     *   encrypt_public: pk T[2][L][N] in NTT form, small int32[3][count][N] = (u, e0, e1), message T[count][L][N] in NTT
     *     form or NULL, out T[2][count][L][N]; the scratch is encrypt_public_scratch_bytes bytes.
     *   bfv scale_message: message T[count][N] (read modulo t) -> out T[count][L][N] = round(Q m / t) in the q-base.
     *   bfv decode: x T[stacks][L][N] in coefficient form -> message_out T[stacks][N], noise_max T[stacks] or NULL.
     *   bfv decrypt: phase into the scratch (decrypt_scratch_bytes bytes), then decode; key_switch_scratch is the
     *     key-switching plan's phase_scratch_bytes bytes.
     *   noise_budget_bits (host only): max(0, W - 1 - bit_length(noise_max + 3 q_count)). */
    int gpuntt_keyswitch_plan_phase_scratch_bytes_u32(const gpuntt_keyswitch_plan* plan, int count, int components,
                                                      int input_ntt, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_phase_scratch_bytes_u64(const gpuntt_keyswitch_plan* plan, int count, int components,
                                                      int input_ntt, uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_phase_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* ct, const uint32_t* s,
                                        uint32_t* out, int count, int components, int input_ntt, int output_ntt,
                                        void* scratch, void* stream);
    int gpuntt_keyswitch_plan_phase_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* ct, const uint64_t* s,
                                        uint64_t* out, int count, int components, int input_ntt, int output_ntt,
                                        void* scratch, void* stream);
    int gpuntt_keyswitch_plan_encrypt_public_scratch_bytes_u32(const gpuntt_keyswitch_plan* plan, int count,
                                                               uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_encrypt_public_scratch_bytes_u64(const gpuntt_keyswitch_plan* plan, int count,
                                                               uint64_t* bytes_host);
    int gpuntt_keyswitch_plan_encrypt_public_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* pk,
                                                 const int32_t* small, const uint32_t* message, uint32_t* out, int count,
                                                 void* scratch, void* stream);
    int gpuntt_keyswitch_plan_encrypt_public_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* pk,
                                                 const int32_t* small, const uint64_t* message, uint64_t* out, int count,
                                                 void* scratch, void* stream);
    int gpuntt_bfv_plan_scale_message_u32(const gpuntt_bfv_plan* plan, const uint32_t* message, uint32_t* out, int count,
                                          int to_ntt, void* stream);
    int gpuntt_bfv_plan_scale_message_u64(const gpuntt_bfv_plan* plan, const uint64_t* message, uint64_t* out, int count,
                                          int to_ntt, void* stream);
    int gpuntt_bfv_plan_decode_u32(const gpuntt_bfv_plan* plan, const uint32_t* x, uint32_t* message_out,
                                   uint32_t* noise_max, int stacks, void* stream);
    int gpuntt_bfv_plan_decode_u64(const gpuntt_bfv_plan* plan, const uint64_t* x, uint64_t* message_out,
                                   uint64_t* noise_max, int stacks, void* stream);
    /* decode with noise_max from two launches and no memset: partials is decode_partials_bytes bytes of device memory */
    int gpuntt_bfv_plan_decode_partials_bytes_u32(const gpuntt_bfv_plan* plan, int stacks, uint64_t* bytes_host);
    int gpuntt_bfv_plan_decode_partials_bytes_u64(const gpuntt_bfv_plan* plan, int stacks, uint64_t* bytes_host);
    int gpuntt_bfv_plan_decode_two_launch_u32(const gpuntt_bfv_plan* plan, const uint32_t* x, uint32_t* message_out,
                                              uint32_t* noise_max, int stacks, void* partials, void* stream);
    int gpuntt_bfv_plan_decode_two_launch_u64(const gpuntt_bfv_plan* plan, const uint64_t* x, uint64_t* message_out,
                                              uint64_t* noise_max, int stacks, void* partials, void* stream);
    int gpuntt_bfv_plan_decrypt_scratch_bytes_u32(const gpuntt_bfv_plan* plan, int count, uint64_t* bytes_host);
    int gpuntt_bfv_plan_decrypt_scratch_bytes_u64(const gpuntt_bfv_plan* plan, int count, uint64_t* bytes_host);
    int gpuntt_bfv_plan_decrypt_u32(const gpuntt_bfv_plan* plan, const uint32_t* ct,
                                    const gpuntt_keyswitch_plan* key_switch, const uint32_t* s, uint32_t* message_out,
                                    uint32_t* noise_max, int count, int components, int input_ntt, void* scratch,
                                    void* key_switch_scratch, void* stream);
    int gpuntt_bfv_plan_decrypt_u64(const gpuntt_bfv_plan* plan, const uint64_t* ct,
                                    const gpuntt_keyswitch_plan* key_switch, const uint64_t* s, uint64_t* message_out,
                                    uint64_t* noise_max, int count, int components, int input_ntt, void* scratch,
                                    void* key_switch_scratch, void* stream);
    int gpuntt_bfv_noise_budget_bits_u32(uint32_t noise_max, int q_count);
    int gpuntt_bfv_noise_budget_bits_u64(uint64_t noise_max, int q_count);

    /* ---- BFV batching (include/gpuntt/rns/bfv_encode.cuh; key_switch.cuh, "Plaintext operands") ----
     *   slot_maps (host only): to_position[N] indexed by slot, to_slot[N] its inverse, for the slot convention of
     *     bfv_encode.cuh.  "Invalid n_power range!" outside [1, 28].
     *   encoder create: t the modulus struct of the plaintext modulus, the tables modulo t on the device as for the
     *     negacyclic transforms, n_inverse = N^-1 mod t.  "Plaintext modulus does not support batching!" unless
     *     (t - 1) mod 2N = 0; "Invalid modulus!"; "Invalid n_power range!"; "null pointer argument".
     *   encode: values T[count][N] (any word, by slot) -> plain T[count][N], coefficients modulo t.
     *   decode: plain T[count][N] (canonical) -> values T[count][N]; the scratch is scratch_bytes bytes, 256-byte
     *     aligned.  "Invalid count!", "null pointer argument", "encode input and output overlap!", "decode input and
     *     output overlap!", "The scratch overlaps an operand!", "The scratch is not 256-byte aligned!".
     *   lift_centred: words T[polys][N] read modulo t and centred -> out T[polys][M or L][N]; to_ntt: the plan's forward
     *     transform follows in place.  "Invalid plaintext modulus!", "Invalid polys!", "null pointer argument", "The
     *     lift's input and output overlap!".
     *   multiply_plain: ct T[2][count][L][N] times pt T[plain_count][L][N] (plain_count 1 or count), word by word; out
     *     may be ct.  "Invalid count!", "Invalid plain_count!", "null pointer argument", "out overlaps an operand!". */
    typedef struct gpuntt_bfv_encoder gpuntt_bfv_encoder;
    int gpuntt_bfv_slot_maps(int n_power, uint32_t* to_position_host, uint32_t* to_slot_host);
    int gpuntt_bfv_encoder_workspace_bytes_u32(int n_power, uint64_t* bytes_host);
    int gpuntt_bfv_encoder_workspace_bytes_u64(int n_power, uint64_t* bytes_host);
    int gpuntt_bfv_encoder_scratch_bytes_u32(int n_power, int count, uint64_t* bytes_host);
    int gpuntt_bfv_encoder_scratch_bytes_u64(int n_power, int count, uint64_t* bytes_host);
    int gpuntt_bfv_encoder_create_u32(gpuntt_bfv_encoder** encoder_host, gpuntt_modulus32 plain_modulus, int n_power,
                                      const uint32_t* forward_table, const uint32_t* inverse_table, uint32_t n_inverse,
                                      int batch_hint, void* workspace_device, void* stream);
    int gpuntt_bfv_encoder_create_u64(gpuntt_bfv_encoder** encoder_host, gpuntt_modulus64 plain_modulus, int n_power,
                                      const uint64_t* forward_table, const uint64_t* inverse_table, uint64_t n_inverse,
                                      int batch_hint, void* workspace_device, void* stream);
    int gpuntt_bfv_encoder_encode_u32(const gpuntt_bfv_encoder* encoder, const uint32_t* values, uint32_t* plain,
                                      int count, void* stream);
    int gpuntt_bfv_encoder_encode_u64(const gpuntt_bfv_encoder* encoder, const uint64_t* values, uint64_t* plain,
                                      int count, void* stream);
    int gpuntt_bfv_encoder_decode_u32(const gpuntt_bfv_encoder* encoder, const uint32_t* plain, uint32_t* values,
                                      int count, void* scratch, void* stream);
    int gpuntt_bfv_encoder_decode_u64(const gpuntt_bfv_encoder* encoder, const uint64_t* plain, uint64_t* values,
                                      int count, void* scratch, void* stream);
    int gpuntt_bfv_encoder_owns_workspace_u32(const gpuntt_bfv_encoder* encoder);
    int gpuntt_bfv_encoder_owns_workspace_u64(const gpuntt_bfv_encoder* encoder);
    int gpuntt_bfv_encoder_destroy_u32(gpuntt_bfv_encoder* encoder);
    int gpuntt_bfv_encoder_destroy_u64(gpuntt_bfv_encoder* encoder);
    int gpuntt_keyswitch_plan_lift_centred_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* words,
                                               uint32_t plain_modulus, uint32_t* out, int polys, int full_base,
                                               int to_ntt, void* stream);
    int gpuntt_keyswitch_plan_lift_centred_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* words,
                                               uint64_t plain_modulus, uint64_t* out, int polys, int full_base,
                                               int to_ntt, void* stream);
    int gpuntt_keyswitch_plan_multiply_plain_u32(const gpuntt_keyswitch_plan* plan, const uint32_t* ct,
                                                 const uint32_t* pt, uint32_t* out, int count, int plain_count,
                                                 void* stream);
    int gpuntt_keyswitch_plan_multiply_plain_u64(const gpuntt_keyswitch_plan* plan, const uint64_t* ct,
                                                 const uint64_t* pt, uint64_t* out, int count, int plain_count,
                                                 void* stream);

    /* frees the library-owned scratch buffers of the drop-in entry points (synchronises the device); only when no
     * hipGraph captured from drop-in calls will be replayed again and no call is in flight */
    int gpuntt_release_workspaces(void);

    /* process-wide tuning / test option (GPU_NTT_SetOption, include/gpuntt/ntt_merge/ntt.cuh lists the names);
     * the library itself reads no environment variable */
    int gpuntt_set_option(const char* name, const char* value);

    /* ---- diagnostic: OPERATOR_GPU<T> elementwise on device arrays -----------------------------
     * op: 0 add, 1 sub, 2 mult, 3 reduce (unsigned a), 4 reduce (a read as signed), 5 centered_reduction;
     * b is ignored by ops 3..5 */
    int gpuntt_operator_gpu_u32(int op, const uint32_t* a, const uint32_t* b, uint32_t* out,
                                gpuntt_modulus32 modulus, uint64_t count, void* stream);
    int gpuntt_operator_gpu_u64(int op, const uint64_t* a, const uint64_t* b, uint64_t* out,
                                gpuntt_modulus64 modulus, uint64_t count, void* stream);

    /* diagnostic: the normalised reciprocal floor(2^(W-1+b) / q) (b = bit length of q; 0 for q < 3 and powers of two) the
     * preparation kernels derive for every device-side modulus -- exactness is checked against integers in the tests */
    int gpuntt_debug_recip_norm_u32(const uint32_t* q, uint32_t* out, uint64_t count, void* stream);
    int gpuntt_debug_recip_norm_u64(const uint64_t* q, uint64_t* out, uint64_t count, void* stream);

    /* diagnostic: the public device butterflies CooleyTukeyUnit (gentleman_sande = 0) / GentlemanSandeUnit (1)
     * (reference src/include/gpuntt/ntt_merge/ntt.cuh:69-92) applied to the pairs (u[i], v[i]) with roots[i], in place */
    int gpuntt_butterfly_unit_u32(int gentleman_sande, uint32_t* u, uint32_t* v, const uint32_t* roots,
                                  gpuntt_modulus32 modulus, uint64_t count, void* stream);
    int gpuntt_butterfly_unit_u64(int gentleman_sande, uint64_t* u, uint64_t* v, const uint64_t* roots,
                                  gpuntt_modulus64 modulus, uint64_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPUNTT_C_H */
