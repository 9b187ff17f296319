// example_keygen_rotate.cpp -- a C++ caller that makes its key material ON THE DEVICE (gpuntt/rns/sampling.cuh and the
// "Key material" calls of gpuntt/rns/key_switch.cuh) and then rotates with it:
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2).
//   secret:      sample_small (ternary) -> lift_small (full base, NTT form)            = s
//   source:      GPU_Automorphism_NTT(s, k)                                            = sigma_k(s), k = rotation by 1
//   key:         sample_uniform into the `a` planes in place, sample_small (cbd21) errors, generate_keys
//   ciphertext:  lift_small of a small message (q-base, NTT form), sample_uniform into out[1], sample_small errors,
//                encrypt_symmetric
//   rotation:    decompose(c1), rotate_hoisted(a, c0, key, k), coefficient form
//   and the HOST decrypts: out_0 + out_1 s - sigma_k(m) must be the same small integer under both q-limbs, within
//     21 (the rotated encryption error) + N D 21 max(q) / (2 P) (the key's errors through the key switch: digits below
//     q / 2 against errors of at most 21, divided by P) + (1 + |s|_1) / 2 + 1 (the two ModDowns).
//   The samplers are not cryptographic (sampling.cuh): a production caller fills the same buffers from its own generator.
//
//   ./example_keygen_rotate <LOGN <= 12> [u32]
#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/galois.cuh"
#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/key_switch.cuh"
#include "gpuntt/rns/sampling.cuh"

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
    constexpr int L = 2, K = 1, M = 3, ALPHA = 1, count = 1;
    const size_t n = size_t(1) << logn;
    const auto poly = ReductionPolynomial::X_N_plus;

    std::vector<Modulus<T>> mods;
    std::vector<T> values;
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
        values.push_back(q);
        ninv.push_back(prm.n_inv);
    }
    const int D = KeySwitchPlan<T>::digits(L, ALPHA);
    const std::uint32_t elts[1] = {GaloisElementForRotation(1, logn)};
    const std::uint64_t seed = 0x5EEDull;

    std::vector<std::int32_t> message(n);
    for (size_t j = 0; j < n; j++)
        message[j] = (static_cast<std::int32_t>((j * 2654435761u) % 2001) - 1000) * (1 << 20); // far above the noise

    const size_t key_words = size_t(D) * 2 * M * n, ct_words = size_t(2) * count * L * n;
    std::int32_t *d_s_small = device_words<std::int32_t>(n), *d_key_err = device_words<std::int32_t>(D * n),
                 *d_ct_err = device_words<std::int32_t>(count * n), *d_message = upload(message);
    T *d_s = device_words<T>(M * n), *d_s_from = device_words<T>(M * n), *d_key = device_words<T>(key_words),
      *d_msg = device_words<T>(count * L * n), *d_ct = device_words<T>(ct_words),
      *d_a = device_words<T>(size_t(D) * count * M * n), *d_out = device_words<T>(ct_words);
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            2 * count * M, M, nullptr, 0);
        void *d_keygen = nullptr, *d_encrypt = nullptr, *d_scratch = nullptr, *d_hoist = nullptr;
        GPUNTT_CUDA_CHECK(hipMalloc(&d_keygen, ks.keygen_scratch_bytes(1)));
        GPUNTT_CUDA_CHECK(hipMalloc(&d_encrypt, ks.encrypt_scratch_bytes(count)));
        GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, ks.scratch_bytes(count, 2)));
        GPUNTT_CUDA_CHECK(hipMalloc(&d_hoist, ks.hoisted_scratch_bytes(count, 1)));

        // the secret, and what the rotation key switches from
        sample_small(d_s_small, 1, logn, SmallDistribution::ternary, seed, 0, 0);
        ks.lift_small(d_s_small, d_s, 1, true, true, 0);
        GPU_Automorphism_NTT(d_s, d_s_from, elts, 1, logn, poly, M, 0);
        // the key: a in place, then component 0
        sample_uniform<T>(d_key + M * n, values.data(), M, logn, D, 2 * M * n, seed, 1, 0);
        sample_small(d_key_err, D, logn, SmallDistribution::cbd21, seed, 2, 0);
        T* keys[1] = {d_key};
        ks.generate_keys(d_s, d_s_from, d_key_err, keys, 1, d_keygen, 0);
        // the ciphertext
        ks.lift_small(d_message, d_msg, count, false, true, 0);
        sample_uniform<T>(d_ct + count * L * n, values.data(), L, logn, count, L * n, seed, 3, 0);
        sample_small(d_ct_err, count, logn, SmallDistribution::cbd21, seed, 4, 0);
        ks.encrypt_symmetric(d_s, d_ct_err, d_msg, d_ct, count, d_encrypt, 0);
        // the rotation
        ks.decompose(d_ct + count * L * n, d_a, count, true, d_scratch, 0);
        ks.rotate_hoisted(d_a, d_ct, keys, elts, 1, d_out, count, false, d_hoist, 0);

        const std::vector<T> out = download(d_out, ct_words);
        const std::vector<std::int32_t> s = download(d_s_small, n);
        // the device words equal the host references
        std::vector<std::int32_t> s_ref(n);
        reference_sample_small(s_ref.data(), 1, logn, SmallDistribution::ternary, seed, 0);
        ok = ok && s == s_ref;
        std::vector<T> a_ref(key_words, T(0));
        reference_sample_uniform<T>(a_ref.data() + M * n, values.data(), M, logn, D, 2 * M * n, seed, 1);
        const std::vector<T> key = download(d_key, key_words);
        for (int d = 0; d < D; d++)
            for (size_t i = 0; i < M * n; i++)
                ok = ok && key[(size_t(2 * d) + 1) * M * n + i] == a_ref[(size_t(2 * d) + 1) * M * n + i];

        // decrypt: out_0 + out_1 s in Z_q[X] / (X^N + 1), then minus sigma_k(m)
        long long h = 0;
        for (std::int32_t v : s)
            h += v < 0 ? -v : v;
        const double qmax = static_cast<double>(std::max(primes[0].q, primes[1].q));
        const double bound =
            21.0 + double(n) * D * 21.0 * qmax / (2.0 * static_cast<double>(primes[2].q)) + (1.0 + double(h)) / 2.0 + 1.0;
        std::vector<long long> rotated(n); // sigma_k(m)
        for (size_t i = 0; i < n; i++)
        {
            const size_t e = (i * elts[0]) % (2 * n);
            rotated[e % n] = e < n ? message[i] : -message[i];
        }
        std::vector<long long> err[L];
        for (int m = 0; m < L; m++)
        {
            const T q = primes[m].q;
            std::vector<T> v(out.begin() + m * n, out.begin() + (m + 1) * n); // component 0
            const T* c1 = out.data() + (size_t(count) * L + m) * n;
            for (size_t i = 0; i < n; i++)
                for (size_t j = 0; j < n; j++)
                {
                    if (s[j] == 0)
                        continue;
                    const bool wrap = i + j >= n;
                    const bool minus = (s[j] < 0) != wrap;
                    T& x = v[(i + j) % n];
                    x = minus ? (x >= c1[i] ? x - c1[i] : x + (q - c1[i])) : static_cast<T>((static_cast<U128>(x) + c1[i]) % q);
                }
            for (size_t j = 0; j < n; j++)
            {
                const T mag = static_cast<T>(static_cast<std::uint64_t>(rotated[j] < 0 ? -rotated[j] : rotated[j]) % q);
                const T want = rotated[j] < 0 && mag != 0 ? q - mag : mag; // the message may pass a 32-bit q
                const T d = v[j] >= want ? v[j] - want : v[j] + (q - want);
                err[m].push_back(d > q / 2 ? -static_cast<long long>(q - d) : static_cast<long long>(d));
            }
        }
        long long worst = 0;
        for (size_t j = 0; j < n; j++)
        {
            ok = ok && err[0][j] == err[1][j]; // one integer, seen under both limbs
            worst = std::max(worst, err[0][j] < 0 ? -err[0][j] : err[0][j]);
        }
        ok = ok && static_cast<double>(worst) <= bound;
        std::cout << "rotation error " << worst << ", bound " << bound << std::endl;

        // a plan that reads its keys through key_limbs does not generate them
        try
        {
            const int limbs[M] = {1, 0, 2};
            KeySwitchPlan<T> other(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                                   2 * count * M, M, limbs, 0);
            other.generate_keys(d_s, d_s_from, d_key_err, keys, 1, d_keygen, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
        for (void* p : {d_keygen, d_encrypt, d_scratch, d_hoist})
            (void) hipFree(p);
    }
    for (void* p : {(void*) d_s_small, (void*) d_key_err, (void*) d_ct_err, (void*) d_message, (void*) d_s, (void*) d_s_from,
                    (void*) d_key, (void*) d_msg, (void*) d_ct, (void*) d_a, (void*) d_out, (void*) d_fwd, (void*) d_inv})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 2) ? std::atoi(argv[1]) : 10;
    const bool u32 = (argc >= 3) && std::string(argv[2]) == "u32";
    if (logn < 1 || logn > 12)
        return EXIT_FAILURE;
    if (u32)
        return run<Data32>(logn, {{536641537u, 167028958u}, {536608769u, 417302965u}, {1073643521u, 269685106u}}, 14);
    return run<Data64>(logn,
                       {{576460752300015617ull, 296969298802020438ull},
                        {576460752298835969ull, 132309083155986965ull},
                        {1152921504598720513ull, 560939867933173424ull}},
                       16);
}
