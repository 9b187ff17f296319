// example_bfv_roundtrip.cpp -- a C++ caller that closes the BFV loop ON THE DEVICE with more than one q-prime
// (gpuntt/rns/sampling.cuh, gpuntt/rns/key_switch.cuh "Key material" and "Decryption and public-key encryption",
// gpuntt/rns/bfv_multiply.cuh "Reading a result back"):
//
//   q-base {q0, q1} (L = 2), auxiliary base {b0, b1, b2} for the t / Q rounding, special primes {p0, p1}, alpha = 2 (one
//   digit); every prime has 40 bits, found here by search with its 2N-th root of unity; t = 257.
//   secret:       sample_small (ternary) -> lift_small (full base {q, p}, NTT form)                 = s
//   relin key:    s^2 by GPU_PointwiseMul per limb, sample_uniform into the `a` plane, cbd21 errors, generate_keys
//   public key:   sample_uniform into pk[1], cbd21 error, encrypt_symmetric of zero
//   messages:     m1 uniform modulo t (sample_uniform with the one modulus t), m2 with 8 non-zero coefficients
//   encode:       BfvMultiplyPlan::scale_message (round(Q m / t), NTT form)
//   encrypt:      KeySwitchPlan::encrypt_public (u ternary, e0 / e1 cbd21)
//   decrypt:      BfvMultiplyPlan::decrypt -> the messages, exactly, and the fresh noise
//   evaluate:     BfvMultiplyPlan::multiply_relinearize, then decrypt -> m1 m2 mod (t, X^N + 1), and the noise after
//   The host only compares messages (the sparse negacyclic product in 64-bit integers) and prints the two noise budgets.
//   The samplers are not cryptographic (sampling.cuh): a production caller fills the same buffers from its own generator.
//
//   ./example_bfv_roundtrip [LOGN in 4 .. 12, default 10]
#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/bfv_multiply.cuh"
#include "gpuntt/rns/key_switch.cuh"
#include "gpuntt/rns/sampling.cuh"

using T = Data64;
using U128 = unsigned __int128;

static T mulmod(T a, T b, T m) { return static_cast<T>(static_cast<U128>(a) * b % m); }
static T powmod(T a, std::uint64_t e, T m)
{
    T r = 1;
    for (; e != 0; e >>= 1, a = mulmod(a, a, m))
        if (e & 1)
            r = mulmod(r, a, m);
    return r;
}
static bool is_prime(T q) // Miller-Rabin, deterministic for 64-bit words with these bases
{
    if (q < 4)
        return q == 2 || q == 3;
    if (q % 2 == 0)
        return false;
    T d = q - 1;
    int r = 0;
    while (d % 2 == 0)
        d /= 2, r++;
    for (T a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull})
    {
        if (a % q == 0)
            continue;
        T x = powmod(a % q, d, q);
        if (x == 1 || x == q - 1)
            continue;
        bool composite = true;
        for (int i = 1; i < r && composite; i++)
        {
            x = mulmod(x, x, q);
            composite = x != q - 1;
        }
        if (composite)
            return false;
    }
    return true;
}
struct Prime
{
    T q, psi; // psi: a primitive 2N-th root of unity
};
// `count` primes q = 1 (mod 2N) going down from 2^bits, each with a primitive 2N-th root of unity
static std::vector<Prime> find_primes(int bits, int logn, int count)
{
    std::vector<Prime> out;
    const T two_n = T(2) << logn;
    for (T q = (T(1) << bits) - two_n + 1; static_cast<int>(out.size()) < count; q -= two_n)
    {
        if (!is_prime(q))
            continue;
        for (T x = 2;; x++)
        {
            const T psi = powmod(x, (q - 1) / two_n, q);
            if (powmod(psi, two_n / 2, q) == q - 1) // order exactly 2N
            {
                out.push_back({q, psi});
                break;
            }
        }
    }
    return out;
}

template <typename V> V* upload(const std::vector<V>& h)
{
    V* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, h.size() * sizeof(V)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice));
    return d;
}
template <typename V> V* device_words(size_t words)
{
    V* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, words * sizeof(V)));
    GPUNTT_CUDA_CHECK(hipMemset(d, 0, words * sizeof(V)));
    return d;
}
static void* device_bytes(size_t bytes)
{
    void* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, bytes < 256 ? 256 : bytes));
    return d;
}
template <typename V> std::vector<V> download(const V* d, size_t words)
{
    std::vector<V> h(words);
    GPUNTT_CUDA_CHECK(hipMemcpy(h.data(), d, words * sizeof(V), hipMemcpyDeviceToHost));
    return h;
}

int main(int argc, char* argv[])
{
    using namespace gpuntt;
    CudaDevice();
    const int logn = (argc >= 2) ? std::atoi(argv[1]) : 10;
    if (logn < 4 || logn > 12)
        return EXIT_FAILURE;
    constexpr int L = 2, KB = 3, KP = 2, ALPHA = 2, MB = L + KB, MP = L + KP, count = 2;
    const T t = 257;
    const size_t n = size_t(1) << logn;
    const auto poly = ReductionPolynomial::X_N_plus;
    const std::vector<Prime> primes = find_primes(40, logn, L + KB + KP);

    // one table set per full base, modulus m of the base at m << n_power: {q, b} = primes 0 .. 4, {q, p} = 0 1 5 6
    auto tables = [&](const std::vector<int>& which, std::vector<Modulus<T>>& mods, std::vector<T>& values,
                      std::vector<Root<T>>& fwd, std::vector<Root<T>>& inv, std::vector<Ninverse<T>>& ninv) {
        fwd.resize(which.size() * n), inv.resize(which.size() * n);
        for (size_t m = 0; m < which.size(); m++)
        {
            const Prime& p = primes[which[m]];
            NTTParameters<T> prm(logn, NTTFactors<T>(Modulus<T>(p.q), mulmod(p.psi, p.psi, p.q), p.psi), poly);
            const auto f = prm.gpu_root_of_unity_table_generator(prm.forward_root_of_unity_table);
            const auto b = prm.gpu_root_of_unity_table_generator(prm.inverse_root_of_unity_table);
            std::copy(f.begin(), f.end(), fwd.begin() + m * n);
            std::copy(b.begin(), b.end(), inv.begin() + m * n);
            mods.push_back(prm.modulus), values.push_back(p.q), ninv.push_back(prm.n_inv);
        }
    };
    std::vector<Modulus<T>> mods_b, mods_p;
    std::vector<T> val_b, val_p;
    std::vector<Root<T>> fwd_b, inv_b, fwd_p, inv_p;
    std::vector<Ninverse<T>> ninv_b, ninv_p;
    tables({0, 1, 2, 3, 4}, mods_b, val_b, fwd_b, inv_b, ninv_b);
    tables({0, 1, 5, 6}, mods_p, val_p, fwd_p, inv_p, ninv_p);
    Root<T>*d_fwd_b = upload(fwd_b), *d_inv_b = upload(inv_b), *d_fwd_p = upload(fwd_p), *d_inv_p = upload(inv_p);

    // m2: 8 non-zero coefficients, so that the host forms m1 m2 in 8 N steps
    std::vector<T> m2(n, 0);
    std::vector<size_t> where;
    for (int k = 0; k < 8; k++)
    {
        const size_t at = (size_t(k) * 2654435761u + 17) % n;
        if (m2[at] == 0)
            where.push_back(at);
        m2[at] = 1 + (k * 37 + 5) % (t - 1);
    }

    const std::uint64_t seed = 0xB0F5EEDull;
    const size_t ct_words = size_t(2) * count * L * n;
    std::int32_t *d_s_small = device_words<std::int32_t>(n), *d_key_err = device_words<std::int32_t>(n),
                 *d_pk_err = device_words<std::int32_t>(n), *d_small = device_words<std::int32_t>(3 * count * n);
    T *d_s = device_words<T>(MP * n), *d_s2 = device_words<T>(MP * n), *d_key = device_words<T>(2 * MP * n),
      *d_pk = device_words<T>(2 * L * n), *d_msg = device_words<T>(count * n), *d_scaled = device_words<T>(count * L * n),
      *d_ct = device_words<T>(ct_words), *d_x = device_words<T>(2 * L * n), *d_y = device_words<T>(2 * L * n),
      *d_prod = device_words<T>(2 * L * n), *d_out = device_words<T>(count * n), *d_noise = device_words<T>(count);

    bool ok = true;
    {
        BfvMultiplyPlan<T> bfv(mods_b.data(), L, mods_b.data() + L, KB, t, logn, d_fwd_b, d_inv_b, ninv_b.data(), poly,
                               4 * MB, 0);
        KeySwitchPlan<T> ks(mods_p.data(), L, mods_p.data() + L, KP, ALPHA, logn, d_fwd_p, d_inv_p, ninv_p.data(), poly,
                            3 * count * L, MP, nullptr, 0);
        ok = ok && ks.digits() == 1;
        void *d_keygen = device_bytes(ks.keygen_scratch_bytes(1)), *d_sym = device_bytes(ks.encrypt_scratch_bytes(1)),
             *d_pub = device_bytes(ks.encrypt_public_scratch_bytes(count)),
             *d_dec = device_bytes(bfv.decrypt_scratch_bytes(count)), *d_mul = device_bytes(bfv.scratch_bytes(1)),
             *d_ks = device_bytes(ks.scratch_bytes(1, 2));

        // the secret and its square, the relinearization key, the public key
        sample_small(d_s_small, 1, logn, SmallDistribution::ternary, seed, 0, 0);
        ks.lift_small(d_s_small, d_s, 1, true, true, 0);
        for (int m = 0; m < MP; m++)
            GPU_PointwiseMul(d_s + m * n, d_s + m * n, d_s2 + m * n, mods_p[m], logn, 1, 0);
        sample_uniform<T>(d_key + MP * n, val_p.data(), MP, logn, 1, 2 * MP * n, seed, 1, 0);
        sample_small(d_key_err, 1, logn, SmallDistribution::cbd21, seed, 2, 0);
        T* keys[1] = {d_key};
        ks.generate_keys(d_s, d_s2, d_key_err, keys, 1, d_keygen, 0);
        sample_uniform<T>(d_pk + L * n, val_p.data(), L, logn, 1, L * n, seed, 3, 0);
        sample_small(d_pk_err, 1, logn, SmallDistribution::cbd21, seed, 4, 0);
        ks.encrypt_symmetric(d_s, d_pk_err, nullptr, d_pk, 1, d_sym, 0);

        // the messages, encoded and encrypted under the public key
        const T tv[1] = {t};
        sample_uniform<T>(d_msg, tv, 1, logn, 1, n, seed, 5, 0);
        GPUNTT_CUDA_CHECK(hipMemcpy(d_msg + n, m2.data(), n * sizeof(T), hipMemcpyHostToDevice));
        bfv.scale_message(d_msg, d_scaled, count, true, 0);
        sample_small(d_small, count, logn, SmallDistribution::ternary, seed, 6, 0);
        sample_small(d_small + count * n, 2 * count, logn, SmallDistribution::cbd21, seed, 7, 0);
        ks.encrypt_public(d_pk, d_small, d_scaled, d_ct, count, d_pub, 0);

        // fresh: the messages come back
        bfv.decrypt(d_ct, ks, d_s, d_out, d_noise, count, 2, true, d_dec, nullptr, 0);
        const std::vector<T> msg = download(d_msg, count * n);
        ok = ok && download(d_out, count * n) == msg;
        const std::vector<T> fresh = download(d_noise, count);
        const int budget_fresh = std::min(noise_budget_bits<T>(fresh[0], L), noise_budget_bits<T>(fresh[1], L));

        // ct x ct, relinearized: component-major T[2][count][L][N] -> the two operands T[2][1][L][N]
        for (int c = 0; c < 2; c++)
        {
            GPUNTT_CUDA_CHECK(hipMemcpy(d_x + c * L * n, d_ct + (size_t(c) * count + 0) * L * n, L * n * sizeof(T),
                                        hipMemcpyDeviceToDevice));
            GPUNTT_CUDA_CHECK(hipMemcpy(d_y + c * L * n, d_ct + (size_t(c) * count + 1) * L * n, L * n * sizeof(T),
                                        hipMemcpyDeviceToDevice));
        }
        bfv.multiply_relinearize(d_x, d_y, ks, d_key, d_prod, 1, true, true, d_mul, d_ks, 0);
        bfv.decrypt(d_prod, ks, d_s, d_out, d_noise, 1, 2, true, d_dec, nullptr, 0);
        const std::vector<T> got = download(d_out, n);
        const int budget_after = noise_budget_bits<T>(download(d_noise, 1)[0], L);

        // m1 m2 mod (t, X^N + 1), 8 shifted copies of m1
        std::vector<long long> want(n, 0);
        for (size_t at : where)
            for (size_t i = 0; i < n; i++)
            {
                const long long p = static_cast<long long>(msg[i]) * static_cast<long long>(m2[at]);
                want[(i + at) % n] += i + at >= n ? -p : p;
            }
        for (size_t i = 0; i < n; i++)
        {
            const long long w = ((want[i] % static_cast<long long>(t)) + static_cast<long long>(t)) % static_cast<long long>(t);
            ok = ok && got[i] == static_cast<T>(w);
        }
        std::cout << "noise budget: fresh " << budget_fresh << " bits, after one multiplication " << budget_after
                  << " bits" << std::endl;
        ok = ok && budget_after > 0 && budget_after < budget_fresh;

        // a plaintext modulus above a q-prime is refused by the new calls, before a launch
        try
        {
            BfvMultiplyPlan<T> wide(mods_b.data(), 1, mods_b.data() + 1, MB - 1, primes[0].q + 2, logn, nullptr, nullptr,
                                    nullptr, poly, 1, 0);
            wide.decode(d_scaled, d_out, d_noise, 1, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
        for (void* p : {d_keygen, d_sym, d_pub, d_dec, d_mul, d_ks})
            (void) hipFree(p);
    }
    for (void* p : {(void*) d_s_small, (void*) d_key_err, (void*) d_pk_err, (void*) d_small, (void*) d_s, (void*) d_s2,
                    (void*) d_key, (void*) d_pk, (void*) d_msg, (void*) d_scaled, (void*) d_ct, (void*) d_x, (void*) d_y,
                    (void*) d_prod, (void*) d_out, (void*) d_noise, (void*) d_fwd_b, (void*) d_inv_b, (void*) d_fwd_p,
                    (void*) d_inv_p})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}
