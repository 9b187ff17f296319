// example_hoisted_sum.cpp -- a C++ caller of KeySwitchPlan<T>::rotate_hoisted_sum (gpuntt/rns/key_switch.cuh): the
// weighted sum of three rotations of one ciphertext (c0, c1) from ONE decompose, one ModDown for all of them.
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2).
//   decompose(c1) once; then
//     hoisted sum:  rotate_hoisted_sum(a, c0, three keys, three Galois elements, three weights -- one of them null)
//     composition:  per rotation GPU_Automorphism_NTT(a) and InnerProductPlan::multiply_accumulate (C = 2), the term
//                   (P mod q_m) * c0 rotated by GPU_Automorphism_NTT and added to component 0 on the host; then ONE
//                   multiply_accumulate with the three stacks as digits and the weights as the key, the full-base INTT,
//                   mod_down and the q-base NTT                                            -- the definition
//   and every output word of the two is compared, in coefficient and in NTT form.  Keys and weights are random (a real
//   key encrypts the rotated secret, a real weight is an encoded matrix diagonal; the data path is the same).
//
//   ./example_hoisted_sum <LOGN <= 14> [u32]
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
    constexpr int L = 2, K = 1, M = 3, ALPHA = 1, G = 3, count = 1;
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
    const std::uint32_t elts[G] = {GaloisElementForRotation(1, logn), GaloisElementForRotation(2, logn),
                                   GaloisElementForRotation(3, logn)};

    std::mt19937_64 rng(31);
    std::vector<T> c0(count * L * n), c1(count * L * n);
    for (size_t i = 0; i < c0.size(); i++)
    {
        c0[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // NTT form
        c1[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // coefficient form
    }
    const size_t key_words = size_t(D) * 2 * M * n, a_words = size_t(D) * count * M * n,
                 acc_words = size_t(2) * count * M * n, out_words = size_t(2) * count * L * n;
    std::vector<T*> d_keys;
    std::vector<const T*> d_weights; // weights[1] stays null: weight 1
    std::vector<T> weight_key(size_t(G) * M * n, T(1)); // the same weights as a key T[G][1][M][N], ones for the null entry
    for (int g = 0; g < G; g++)
    {
        std::vector<T> key(key_words);
        for (size_t i = 0; i < key.size(); i++)
            key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);
        d_keys.push_back(upload(key));
        if (g == 1)
        {
            d_weights.push_back(nullptr);
            continue;
        }
        std::vector<T> w(size_t(M) * n);
        for (size_t i = 0; i < w.size(); i++)
            w[i] = weight_key[g * M * n + i] = static_cast<T>(rng() % primes[i / n].q);
        d_weights.push_back(upload(w));
    }
    // (P mod q_m) * c0, what the kernel folds into component 0 before the ModDown
    std::vector<T> pc0(c0.size());
    for (size_t i = 0; i < c0.size(); i++)
    {
        const T q = primes[(i / n) % L].q;
        pc0[i] = mulmod<T>(c0[i], static_cast<T>(primes[L].q % q), q);
    }
    T *d_c0 = upload(c0), *d_pc0 = upload(pc0), *d_c1 = upload(c1), *d_a = device_words<T>(a_words),
      *d_a_rot = device_words<T>(G * a_words), *d_c0_rot = device_words<T>(G * c0.size()),
      *d_u = device_words<T>(G * acc_words), *d_acc = device_words<T>(acc_words), *d_wkey = upload(weight_key),
      *d_out = device_words<T>(out_words), *d_want = device_words<T>(out_words);
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);
    void *d_scratch = nullptr, *d_hoist = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, KeySwitchPlan<T>::scratch_bytes(L, K, ALPHA, logn, count, 2)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_hoist, KeySwitchPlan<T>::hoisted_sum_scratch_bytes(L, K, ALPHA, logn, count)));

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            2 * count * M, M, nullptr, 0);
        InnerProductPlan<T> inner(mods.data(), M, 0);
        NTTPlan<T> intt_full(d_inv, mods.data(), M, logn, poly, INVERSE, ninv.data(), 2 * count * M, 0);
        NTTPlan<T> ntt_q(d_fwd, mods.data(), L, logn, poly, FORWARD, nullptr, 2 * count * L, 0);
        ok = ok && ks.hoisted_sum_scratch_bytes(count) == KeySwitchPlan<T>::hoisted_sum_scratch_bytes(L, K, ALPHA, logn, count);
        ok = ok && ks.hoisted_sum_scratch_bytes(count) == ks.hoisted_scratch_bytes(count, 1); // it does not grow with G

        ks.decompose(d_c1, d_a, count, false, d_scratch, 0); // ONCE
        for (const bool output_ntt : {false, true})
        {
            ks.rotate_hoisted_sum(d_a, d_c0, d_keys.data(), elts, d_weights.data(), G, d_out, count, output_ntt, d_hoist,
                                  0);
            const std::vector<T> got = download(d_out, out_words);

            // the definition: u_g = inner product of the permuted digits, plus the rotated P c0 on component 0 ...
            GPU_Automorphism_NTT(d_a, d_a_rot, elts, G, logn, poly, D * count * M, 0);
            GPU_Automorphism_NTT(d_pc0, d_c0_rot, elts, G, logn, poly, count * L, 0);
            const std::vector<T> c0_rot = download(d_c0_rot, G * c0.size());
            for (int g = 0; g < G; g++)
            {
                inner.multiply_accumulate(d_a_rot + g * a_words, d_keys[g], d_u + g * acc_words, logn, D, 2, count, false,
                                          M, nullptr, 0);
                std::vector<T> u = download(d_u + g * acc_words, acc_words);
                for (int r = 0; r < count; r++)
                    for (int m = 0; m < L; m++) // component 0 is the first count stacks of M limbs
                        for (size_t j = 0; j < n; j++)
                        {
                            T& x = u[(size_t(r) * M + m) * n + j];
                            x = static_cast<T>((static_cast<U128>(x) + c0_rot[((size_t(g) * count + r) * L + m) * n + j]) %
                                               primes[m].q);
                        }
                GPUNTT_CUDA_CHECK(hipMemcpy(d_u + g * acc_words, u.data(), acc_words * sizeof(T), hipMemcpyHostToDevice));
            }
            // ... then the weighted sum over g (the G stacks as digits, the weights as the key), and ONE of each step
            inner.multiply_accumulate(d_u, d_wkey, d_acc, logn, G, 1, 2 * count, false, M, nullptr, 0);
            intt_full.execute(d_acc, d_acc, 2 * count * M, 0);
            ks.mod_down(d_acc, d_want, 2 * count, 0);
            if (output_ntt)
                ntt_q.execute(d_want, d_want, 2 * count * L, 0);
            const std::vector<T> want = download(d_want, out_words);
            ok = ok && want == got;
        }

        // an even element is refused before anything is launched
        try
        {
            const std::uint32_t even[G] = {elts[0], 2u, elts[2]};
            ks.rotate_hoisted_sum(d_a, d_c0, d_keys.data(), even, d_weights.data(), G, d_out, count, false, d_hoist, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_c0, (void*) d_pc0, (void*) d_c1, (void*) d_a, (void*) d_a_rot, (void*) d_c0_rot, (void*) d_u,
                    (void*) d_acc, (void*) d_wkey, (void*) d_out, (void*) d_want, (void*) d_fwd, (void*) d_inv, d_scratch,
                    d_hoist})
        (void) hipFree(p);
    for (T* p : d_keys)
        (void) hipFree(p);
    for (const T* p : d_weights)
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
