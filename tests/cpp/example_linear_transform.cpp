// example_linear_transform.cpp -- a C++ caller of KeySwitchPlan<T>::linear_transform_bsgs (gpuntt/rns/key_switch.cuh): a
// baby-step/giant-step linear transform of one ciphertext (c0, c1) with 3 baby steps and 2 giant steps -- six diagonals,
// three switching keys (the b = 0 and g = 0 steps are the identity and take no key), ONE decompose and ONE final ModDown.
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2).
//   out = sum_g sigma_{k_g}( sum_b pt_{g,b} (.) sigma_{k_b}(ct) ): the diagonal is applied BEFORE the giant rotation.
//   decompose(c1) once; then
//     fused:        linear_transform_bsgs(a, c0, c1, baby keys {null, k, k}, giant keys {null, k}, 2 x 3 weights -- one of
//                   them null: that term is ABSENT)
//     composition:  the definition of the header, step by step, through GPU_Automorphism_NTT,
//                   InnerProductPlan::multiply_accumulate, the full-base INTT, mod_down, decompose and the q-base NTT,
//                   with the modular additions on the host
//   and every output word of the two is compared, in coefficient and in NTT form.  Keys and weights are random (a real
//   key encrypts the rotated secret, a real weight is an encoded matrix diagonal; the data path is the same).
//
//   ./example_linear_transform <LOGN <= 14> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/galois.cuh"
#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/inner_product.cuh"
#include "gpuntt/rns/key_switch.cuh"

using U128 = unsigned __int128;

template <typename T> T mulmod(T a, T b, T m) { return static_cast<T>(static_cast<U128>(a) * b % m); }
template <typename T> T addmod(T a, T b, T m) { return static_cast<T>((static_cast<U128>(a) + b) % m); }
template <typename T> T powmod(T a, std::uint64_t e, T m)
{
    T r = 1;
    for (; e != 0; e >>= 1, a = mulmod(a, a, m))
        if (e & 1)
            r = mulmod(r, a, m);
    return r;
}

template <typename T> struct Prime
{
    T q, psi; // psi: a primitive 2^(max_logn + 1)-th root of unity
};

template <typename T> T* upload(const std::vector<T>& h)
{
    T* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, h.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> T* device_words(size_t words)
{
    T* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, words * sizeof(T)));
    return d;
}
template <typename T> std::vector<T> download(const T* d, size_t words)
{
    std::vector<T> h(words);
    GPUNTT_CUDA_CHECK(hipMemcpy(h.data(), d, words * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

template <typename T> int run(int logn, const Prime<T> (&primes)[3], int max_logn)
{
    using namespace gpuntt;
    constexpr int L = 2, K = 1, M = 3, ALPHA = 1, N1 = 3, N2 = 2, count = 1;
    const size_t n = size_t(1) << logn;
    const auto poly = ReductionPolynomial::X_N_plus;

    std::vector<Modulus<T>> mods;
    std::vector<Root<T>> fwd(M * n), inv(M * n);
    std::vector<Ninverse<T>> ninv;
    for (int m = 0; m < M; m++)
    {
        const T q = primes[m].q, psi = powmod<T>(primes[m].psi, std::uint64_t(1) << (max_logn - logn), q);
        NTTParameters<T> prm(logn, NTTFactors<T>(Modulus<T>(q), mulmod(psi, psi, q), psi), poly);
        const auto f = prm.gpu_root_of_unity_table_generator(prm.forward_root_of_unity_table);
        const auto b = prm.gpu_root_of_unity_table_generator(prm.inverse_root_of_unity_table);
        std::copy(f.begin(), f.end(), fwd.begin() + m * n); // the table of modulus m starts at m << n_power
        std::copy(b.begin(), b.end(), inv.begin() + m * n);
        mods.push_back(prm.modulus);
        ninv.push_back(prm.n_inv);
    }
    const int D = KeySwitchPlan<T>::digits(L, ALPHA);
    // baby steps: the identity (no key), rotations by 1 and 2; giant steps: the identity (no key), rotation by 3
    const std::uint32_t belts[N1] = {1u, GaloisElementForRotation(1, logn), GaloisElementForRotation(2, logn)};
    const std::uint32_t gelts[N2] = {1u, GaloisElementForRotation(3, logn)};

    std::mt19937_64 rng(37);
    const size_t ct_words = size_t(count) * L * n, stack = size_t(count) * M * n;
    std::vector<T> c0(ct_words), c1(ct_words);
    for (size_t i = 0; i < ct_words; i++)
    {
        c0[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // NTT form
        c1[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // coefficient form; its NTT form is computed below
    }
    const size_t key_words = size_t(D) * 2 * M * n, a_words = size_t(D) * stack, acc_words = 2 * stack,
                 out_words = size_t(2) * count * L * n;
    auto random_key = [&] {
        std::vector<T> key(key_words);
        for (size_t i = 0; i < key.size(); i++)
            key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);
        return upload(key);
    };
    const T* bkeys[N1] = {nullptr, random_key(), random_key()};
    const T* gkeys[N2] = {nullptr, random_key()};
    // the weights, row-major [g][b]; (g, b) = (1, 0) is ABSENT.  The same weights as keys T[N1][1][M][N] per giant step,
    // zero limbs for the absent entry
    const T* weights[N2 * N1];
    std::vector<T> weight_key(size_t(N2) * N1 * M * n, T(0));
    for (int i = 0; i < N2 * N1; i++)
    {
        if (i == 1 * N1 + 0)
        {
            weights[i] = nullptr;
            continue;
        }
        std::vector<T> w(size_t(M) * n);
        for (size_t j = 0; j < w.size(); j++)
            w[j] = weight_key[i * M * n + j] = static_cast<T>(rng() % primes[j / n].q);
        weights[i] = upload(w);
    }
    T *d_c0 = upload(c0), *d_c1 = upload(c1), *d_c1_ntt = device_words<T>(ct_words), *d_pc0 = device_words<T>(ct_words),
      *d_rot_c = device_words<T>(ct_words), *d_a = device_words<T>(a_words), *d_a_rot = device_words<T>(a_words),
      *d_u = device_words<T>(N1 * acc_words), *d_v = device_words<T>(acc_words), *d_t = device_words<T>(ct_words),
      *d_a2 = device_words<T>(a_words), *d_s = device_words<T>(acc_words), *d_rot_v = device_words<T>(stack),
      *d_acc = device_words<T>(acc_words), *d_wkey = upload(weight_key), *d_out = device_words<T>(out_words),
      *d_want = device_words<T>(out_words);
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);
    void *d_scratch = nullptr, *d_bsgs = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, KeySwitchPlan<T>::scratch_bytes(L, K, ALPHA, logn, count, 2)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_bsgs, KeySwitchPlan<T>::bsgs_scratch_bytes(L, K, ALPHA, logn, count, N1, N2)));

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            2 * count * M, M, nullptr, 0);
        InnerProductPlan<T> inner(mods.data(), M, 0);
        NTTPlan<T> intt_full(d_inv, mods.data(), M, logn, poly, INVERSE, ninv.data(), 2 * count * M, 0);
        NTTPlan<T> ntt_q(d_fwd, mods.data(), L, logn, poly, FORWARD, nullptr, 2 * count * L, 0);
        ok = ok && ks.bsgs_scratch_bytes(count, N1, N2) == KeySwitchPlan<T>::bsgs_scratch_bytes(L, K, ALPHA, logn, count, N1, N2);

        ks.decompose(d_c1, d_a, count, false, d_scratch, 0); // ONCE
        ntt_q.execute(d_c1, d_c1_ntt, count * L, 0);         // the step without a key reads c1 itself, in NTT form
        const std::vector<T> c1_ntt = download(d_c1_ntt, ct_words);
        // (P mod q_m) * c_c: what the baby steps fold in before any ModDown
        std::vector<T> pc0(ct_words), pc1(ct_words);
        for (size_t i = 0; i < ct_words; i++)
        {
            const T q = primes[(i / n) % L].q, pq = static_cast<T>(primes[L].q % q);
            pc0[i] = mulmod<T>(c0[i], pq, q), pc1[i] = mulmod<T>(c1_ntt[i], pq, q);
        }
        GPUNTT_CUDA_CHECK(hipMemcpy(d_pc0, pc0.data(), ct_words * sizeof(T), hipMemcpyHostToDevice));

        for (const bool output_ntt : {false, true})
        {
            ks.linear_transform_bsgs(d_a, d_c0, d_c1_ntt, bkeys, belts, N1, gkeys, gelts, N2, weights, d_out, count,
                                     output_ntt, d_bsgs, 0);
            const std::vector<T> got = download(d_out, out_words);

            // 1. the baby accumulators u_b: T[N1][2][count][M][N]
            std::vector<T> u(N1 * acc_words, T(0));
            for (int r = 0; r < count; r++) // b = 0, no key: P c_c on the q-limbs, zero on the special limb
                for (int m = 0; m < L; m++)
                    for (size_t j = 0; j < n; j++)
                    {
                        u[(size_t(r) * M + m) * n + j] = pc0[(size_t(r) * L + m) * n + j];
                        u[stack + (size_t(r) * M + m) * n + j] = pc1[(size_t(r) * L + m) * n + j];
                    }
            for (int b = 1; b < N1; b++)
            {
                GPU_Automorphism_NTT(d_a, d_a_rot, belts + b, 1, logn, poly, D * count * M, 0);
                GPU_Automorphism_NTT(d_pc0, d_rot_c, belts + b, 1, logn, poly, count * L, 0);
                inner.multiply_accumulate(d_a_rot, bkeys[b], d_s, logn, D, 2, count, false, M, nullptr, 0);
                const std::vector<T> ub = download(d_s, acc_words), rot = download(d_rot_c, ct_words);
                std::copy(ub.begin(), ub.end(), u.begin() + b * acc_words);
                for (int r = 0; r < count; r++)
                    for (int m = 0; m < L; m++)
                        for (size_t j = 0; j < n; j++)
                        {
                            T& x = u[b * acc_words + (size_t(r) * M + m) * n + j];
                            x = addmod<T>(x, rot[(size_t(r) * L + m) * n + j], primes[m].q);
                        }
            }
            GPUNTT_CUDA_CHECK(hipMemcpy(d_u, u.data(), u.size() * sizeof(T), hipMemcpyHostToDevice));

            std::vector<T> acc(acc_words, T(0));
            for (int g = 0; g < N2; g++)
            {
                // 2. v_g: the N1 stacks as digits, the weights of row g as the key
                inner.multiply_accumulate(d_u, d_wkey + size_t(g) * N1 * M * n, d_v, logn, N1, 1, 2 * count, false, M,
                                          nullptr, 0);
                std::vector<T> s = download(d_v, acc_words);
                if (gkeys[g] != nullptr)
                {
                    // 3. the second component down to the q-base, into digits again, switched and rotated; the first
                    //    component rotated and added with multiplier 1, on ALL M limbs
                    GPUNTT_CUDA_CHECK(hipMemcpy(d_s, d_v + stack, stack * sizeof(T), hipMemcpyDeviceToDevice));
                    intt_full.execute(d_s, d_s, count * M, 0);
                    ks.mod_down(d_s, d_t, count, 0);
                    ks.decompose(d_t, d_a2, count, false, d_scratch, 0);
                    GPU_Automorphism_NTT(d_a2, d_a_rot, gelts + g, 1, logn, poly, D * count * M, 0);
                    inner.multiply_accumulate(d_a_rot, gkeys[g], d_s, logn, D, 2, count, false, M, nullptr, 0);
                    GPU_Automorphism_NTT(d_v, d_rot_v, gelts + g, 1, logn, poly, count * M, 0);
                    s = download(d_s, acc_words);
                    const std::vector<T> v0 = download(d_rot_v, stack);
                    for (size_t i = 0; i < stack; i++)
                        s[i] = addmod<T>(s[i], v0[i], primes[(i / n) % M].q);
                }
                // 4. the sum over the giant steps
                for (size_t i = 0; i < acc_words; i++)
                    acc[i] = addmod<T>(acc[i], s[i], primes[(i / n) % M].q);
            }
            GPUNTT_CUDA_CHECK(hipMemcpy(d_acc, acc.data(), acc_words * sizeof(T), hipMemcpyHostToDevice));
            intt_full.execute(d_acc, d_acc, 2 * count * M, 0);
            ks.mod_down(d_acc, d_want, 2 * count, 0);
            if (output_ntt)
                ntt_q.execute(d_want, d_want, 2 * count * L, 0);
            const std::vector<T> want = download(d_want, out_words);
            ok = ok && want == got;
        }

        // a null key at an element other than 1, and a giant row without a weight, are refused before anything is launched
        try
        {
            const std::uint32_t moved[N1] = {belts[1], belts[1], belts[2]};
            ks.linear_transform_bsgs(d_a, d_c0, d_c1_ntt, bkeys, moved, N1, gkeys, gelts, N2, weights, d_out, count, false,
                                     d_bsgs, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        try
        {
            const T* none[N2 * N1] = {weights[0], weights[1], weights[2], nullptr, nullptr, nullptr};
            ks.linear_transform_bsgs(d_a, d_c0, d_c1_ntt, bkeys, belts, N1, gkeys, gelts, N2, none, d_out, count, false,
                                     d_bsgs, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_c0, (void*) d_c1, (void*) d_c1_ntt, (void*) d_pc0, (void*) d_rot_c, (void*) d_a,
                    (void*) d_a_rot, (void*) d_u, (void*) d_v, (void*) d_t, (void*) d_a2, (void*) d_s, (void*) d_rot_v,
                    (void*) d_acc, (void*) d_wkey, (void*) d_out, (void*) d_want, (void*) d_fwd, (void*) d_inv, d_scratch,
                    d_bsgs})
        (void) hipFree(p);
    for (const T* p : bkeys)
        (void) hipFree(const_cast<T*>(p));
    for (const T* p : gkeys)
        (void) hipFree(const_cast<T*>(p));
    for (const T* p : weights)
        (void) hipFree(const_cast<T*>(p));
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 2) ? std::atoi(argv[1]) : 12;
    const bool u32 = (argc >= 3) && std::string(argv[2]) == "u32";
    if (logn < 1 || logn > 14)
        return EXIT_FAILURE;
    if (u32)
        return run<Data32>(logn, {{536641537u, 167028958u}, {536608769u, 417302965u}, {1073643521u, 269685106u}}, 14);
    return run<Data64>(logn,
                       {{576460752300015617ull, 296969298802020438ull},
                        {576460752298835969ull, 132309083155986965ull},
                        {1152921504598720513ull, 560939867933173424ull}},
                       16);
}
