// example_hoisted_rotation.cpp -- a C++ caller of KeySwitchPlan<T>::rotate_hoisted (gpuntt/rns/key_switch.cuh): one
// ciphertext (c0, c1) rotated by three steps from ONE decompose.
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2).
//   decompose(c1) once; then
//     hoisted:      rotate_hoisted(a, c0, three keys, three Galois elements)              -- one inner product launch
//     composition:  per rotation GPU_Automorphism_NTT(a), switch_digits, GPU_Automorphism_NTT(c0) [+ INTT], and the
//                   addition mod q_m on the host                                          -- the definition
//   and every output word of the two is compared, in coefficient and in NTT form.  The keys are random (a real one
//   encrypts the rotated secret under the secret; the data path is the same).
//
//   ./example_hoisted_rotation <LOGN <= 14> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/galois.cuh"
#include "gpuntt/ntt_merge/ntt.cuh"
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

    std::mt19937_64 rng(29);
    std::vector<T> c0(count * L * n), c1(count * L * n);
    for (size_t i = 0; i < c0.size(); i++)
    {
        c0[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // NTT form
        c1[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // coefficient form
    }
    const size_t key_words = size_t(D) * 2 * M * n, a_words = size_t(D) * count * M * n,
                 out_words = size_t(2) * count * L * n;
    std::vector<T*> d_keys;
    for (int g = 0; g < G; g++)
    {
        std::vector<T> key(key_words);
        for (size_t i = 0; i < key.size(); i++)
            key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);
        d_keys.push_back(upload(key));
    }
    T *d_c0 = upload(c0), *d_c1 = upload(c1), *d_a = device_words<T>(a_words), *d_a_rot = device_words<T>(G * a_words),
      *d_c0_rot = device_words<T>(G * c0.size()), *d_out = device_words<T>(G * out_words),
      *d_each = device_words<T>(out_words);
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);
    void *d_scratch = nullptr, *d_hoist = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, KeySwitchPlan<T>::scratch_bytes(L, K, ALPHA, logn, count, 2)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_hoist, KeySwitchPlan<T>::hoisted_scratch_bytes(L, K, ALPHA, logn, count, G)));

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            G * 2 * count * M, M, nullptr, 0);
        NTTPlan<T> intt_q(d_inv, mods.data(), L, logn, poly, INVERSE, ninv.data(), G * count * L, 0);
        ok = ok && ks.hoisted_scratch_bytes(count, G) == KeySwitchPlan<T>::hoisted_scratch_bytes(L, K, ALPHA, logn, count, G);

        ks.decompose(d_c1, d_a, count, false, d_scratch, 0); // ONCE
        for (const bool output_ntt : {false, true})
        {
            ks.rotate_hoisted(d_a, d_c0, d_keys.data(), elts, G, d_out, count, output_ntt, d_hoist, 0);
            const std::vector<T> got = download(d_out, G * out_words);

            // the definition: permute, switch, add the rotated c0 to component 0
            GPU_Automorphism_NTT(d_a, d_a_rot, elts, G, logn, poly, D * count * M, 0);
            GPU_Automorphism_NTT(d_c0, d_c0_rot, elts, G, logn, poly, count * L, 0);
            if (!output_ntt)
                intt_q.execute(d_c0_rot, d_c0_rot, G * count * L, 0);
            const std::vector<T> c0_rot = download(d_c0_rot, G * c0.size());
            for (int g = 0; g < G; g++)
            {
                ks.switch_digits(d_a_rot + g * a_words, d_keys[g], d_each, count, 2, output_ntt, d_scratch, 0);
                std::vector<T> want = download(d_each, out_words);
                for (size_t i = 0; i < c0.size(); i++) // component 0 is the first count * L polynomials
                {
                    const T q = primes[(i / n) % L].q;
                    want[i] = static_cast<T>((static_cast<U128>(want[i]) + c0_rot[g * c0.size() + i]) % q);
                }
                ok = ok && std::equal(want.begin(), want.end(), got.begin() + g * out_words);
            }
        }

        // an even element is refused before anything is launched
        try
        {
            const std::uint32_t even[G] = {elts[0], 2u, elts[2]};
            ks.rotate_hoisted(d_a, d_c0, d_keys.data(), even, G, d_out, count, false, d_hoist, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_c0, (void*) d_c1, (void*) d_a, (void*) d_a_rot, (void*) d_c0_rot, (void*) d_out,
                    (void*) d_each, (void*) d_fwd, (void*) d_inv, d_scratch, d_hoist})
        (void) hipFree(p);
    for (T* p : d_keys)
        (void) hipFree(p);
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
