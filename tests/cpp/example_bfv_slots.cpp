// example_bfv_slots.cpp -- a C++ caller that works on BFV SLOTS, on the device (gpuntt/rns/bfv_encode.cuh and
// gpuntt/rns/key_switch.cuh "Plaintext operands", beside the calls example_bfv_roundtrip.cpp uses):
//
//   q-base {q0, q1} (L = 2), auxiliary base {b0, b1, b2}, special primes {p0, p1}, alpha = 2; every prime has 40 bits, found
//   here by search with its 2N-th root of unity; t = 65537, with the tables modulo t for the encoder.
//   encode:    BfvBatchEncoder::encode of two slot vectors u and v (2 x N/2 matrices)
//   encrypt:   scale_message and encrypt_public of u
//   rotate:    a Galois key for GaloisElementForRotation(1) from s_from = GPU_Automorphism_NTT(s), then rotate_hoisted
//   multiply:  lift_centred(encode(v)) into the q-base in NTT form, then multiply_plain
//   decrypt, decode: BfvMultiplyPlan::decrypt, BfvBatchEncoder::decode
//   The host only checks the slots: out[r][c] = u[r][(c + 1) mod N/2] * v[r][c] mod t -- both rows rotated LEFT by one.
//   The samplers are not cryptographic (sampling.cuh): a production caller fills the same buffers from its own generator.
//
//   ./example_bfv_slots [LOGN in 4 .. 12, default 10]
#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "gpuntt/ntt_merge/galois.cuh"
#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/bfv_encode.cuh"
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
static T root_of(T q, int logn) // a primitive 2N-th root of unity modulo the prime q = 1 (mod 2N)
{
    const T two_n = T(2) << logn;
    for (T x = 2;; x++)
    {
        const T psi = powmod(x, (q - 1) / two_n, q);
        if (powmod(psi, two_n / 2, q) == q - 1) // order exactly 2N
            return psi;
    }
}
// `count` primes q = 1 (mod 2N) going down from 2^bits, each with a primitive 2N-th root of unity
static std::vector<Prime> find_primes(int bits, int logn, int count)
{
    std::vector<Prime> out;
    const T two_n = T(2) << logn;
    for (T q = (T(1) << bits) - two_n + 1; static_cast<int>(out.size()) < count; q -= two_n)
        if (is_prime(q))
            out.push_back({q, root_of(q, logn)});
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
    constexpr int L = 2, KB = 3, KP = 2, ALPHA = 2, MB = L + KB, MP = L + KP;
    const T t = 65537;
    const size_t n = size_t(1) << logn, half = n / 2;
    const auto poly = ReductionPolynomial::X_N_plus;
    const std::vector<Prime> primes = find_primes(40, logn, L + KB + KP);

    // one table set per full base, modulus m of the base at m << n_power: {q, b} = primes 0 .. 4, {q, p} = 0 1 5 6
    auto tables = [&](const std::vector<Prime>& which, std::vector<Modulus<T>>& mods, std::vector<T>& values,
                      std::vector<Root<T>>& fwd, std::vector<Root<T>>& inv, std::vector<Ninverse<T>>& ninv) {
        fwd.resize(which.size() * n), inv.resize(which.size() * n);
        for (size_t m = 0; m < which.size(); m++)
        {
            const Prime& p = which[m];
            NTTParameters<T> prm(logn, NTTFactors<T>(Modulus<T>(p.q), mulmod(p.psi, p.psi, p.q), p.psi), poly);
            const auto f = prm.gpu_root_of_unity_table_generator(prm.forward_root_of_unity_table);
            const auto b = prm.gpu_root_of_unity_table_generator(prm.inverse_root_of_unity_table);
            std::copy(f.begin(), f.end(), fwd.begin() + m * n);
            std::copy(b.begin(), b.end(), inv.begin() + m * n);
            mods.push_back(prm.modulus), values.push_back(p.q), ninv.push_back(prm.n_inv);
        }
    };
    std::vector<Modulus<T>> mods_b, mods_p, mods_t;
    std::vector<T> val_b, val_p, val_t;
    std::vector<Root<T>> fwd_b, inv_b, fwd_p, inv_p, fwd_t, inv_t;
    std::vector<Ninverse<T>> ninv_b, ninv_p, ninv_t;
    tables({primes[0], primes[1], primes[2], primes[3], primes[4]}, mods_b, val_b, fwd_b, inv_b, ninv_b);
    tables({primes[0], primes[1], primes[5], primes[6]}, mods_p, val_p, fwd_p, inv_p, ninv_p);
    tables({Prime{t, root_of(t, logn)}}, mods_t, val_t, fwd_t, inv_t, ninv_t);
    Root<T>*d_fwd_b = upload(fwd_b), *d_inv_b = upload(inv_b), *d_fwd_p = upload(fwd_p), *d_inv_p = upload(inv_p),
           *d_fwd_t = upload(fwd_t), *d_inv_t = upload(inv_t);

    // the slot vectors u and v, any values below t
    std::vector<T> slots(2 * n);
    std::uint64_t state = 0x51075ull;
    for (auto& w : slots)
    {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        w = (state >> 33) % t;
    }

    const std::uint64_t seed = 0x51075EEDull;
    const std::uint32_t elt = GaloisElementForRotation(1, logn);
    std::int32_t *d_s_small = device_words<std::int32_t>(n), *d_key_err = device_words<std::int32_t>(n),
                 *d_pk_err = device_words<std::int32_t>(n), *d_small = device_words<std::int32_t>(3 * n);
    T *d_s = device_words<T>(MP * n), *d_s_rot = device_words<T>(MP * n), *d_key = device_words<T>(2 * MP * n),
      *d_pk = device_words<T>(2 * L * n), *d_values = upload(slots), *d_plain = device_words<T>(2 * n),
      *d_scaled = device_words<T>(L * n), *d_ct = device_words<T>(2 * L * n), *d_a = device_words<T>(MP * n),
      *d_rot = device_words<T>(2 * L * n), *d_pt = device_words<T>(L * n), *d_msg = device_words<T>(n),
      *d_out = device_words<T>(n), *d_noise = device_words<T>(1);

    bool ok = true;
    {
        BfvBatchEncoder<T> enc(mods_t[0], logn, d_fwd_t, d_inv_t, ninv_t[0], 2, 0);
        BfvMultiplyPlan<T> bfv(mods_b.data(), L, mods_b.data() + L, KB, t, logn, d_fwd_b, d_inv_b, ninv_b.data(), poly,
                               4 * MB, 0);
        KeySwitchPlan<T> ks(mods_p.data(), L, mods_p.data() + L, KP, ALPHA, logn, d_fwd_p, d_inv_p, ninv_p.data(), poly,
                            3 * L, MP, nullptr, 0);
        ok = ok && ks.digits() == 1;
        void *d_keygen = device_bytes(ks.keygen_scratch_bytes(1)), *d_sym = device_bytes(ks.encrypt_scratch_bytes(1)),
             *d_pub = device_bytes(ks.encrypt_public_scratch_bytes(1)), *d_dec = device_bytes(bfv.decrypt_scratch_bytes(1)),
             *d_ks = device_bytes(ks.scratch_bytes(1, 1)), *d_hoist = device_bytes(ks.hoisted_scratch_bytes(1, 1)),
             *d_enc = device_bytes(enc.scratch_bytes(1));

        // the secret, the Galois key of the rotation by one (s_from = sigma_k(s)), the public key
        sample_small(d_s_small, 1, logn, SmallDistribution::ternary, seed, 0, 0);
        ks.lift_small(d_s_small, d_s, 1, true, true, 0);
        GPU_Automorphism_NTT<T>(d_s, d_s_rot, &elt, 1, logn, poly, MP, 0);
        sample_uniform<T>(d_key + MP * n, val_p.data(), MP, logn, 1, 2 * MP * n, seed, 1, 0);
        sample_small(d_key_err, 1, logn, SmallDistribution::cbd21, seed, 2, 0);
        T* keys[1] = {d_key};
        ks.generate_keys(d_s, d_s_rot, d_key_err, keys, 1, d_keygen, 0);
        sample_uniform<T>(d_pk + L * n, val_p.data(), L, logn, 1, L * n, seed, 3, 0);
        sample_small(d_pk_err, 1, logn, SmallDistribution::cbd21, seed, 4, 0);
        ks.encrypt_symmetric(d_s, d_pk_err, nullptr, d_pk, 1, d_sym, 0);

        // encode both vectors; encrypt u
        enc.encode(d_values, d_plain, 2, 0);
        bfv.scale_message(d_plain, d_scaled, 1, true, 0);
        sample_small(d_small, 1, logn, SmallDistribution::ternary, seed, 6, 0);
        sample_small(d_small + n, 2, logn, SmallDistribution::cbd21, seed, 7, 0);
        ks.encrypt_public(d_pk, d_small, d_scaled, d_ct, 1, d_pub, 0);

        // rotate the ciphertext by one slot, then multiply it by the plaintext v
        ks.decompose(d_ct + L * n, d_a, 1, true, d_ks, 0);
        const T* rot_keys[1] = {d_key};
        ks.rotate_hoisted(d_a, d_ct, rot_keys, &elt, 1, d_rot, 1, true, d_hoist, 0);
        ks.lift_centred(d_plain + n, t, d_pt, 1, false, true, 0);
        ks.multiply_plain(d_rot, d_pt, d_rot, 1, 1, 0);

        // decrypt and decode
        bfv.decrypt(d_rot, ks, d_s, d_msg, d_noise, 1, 2, true, d_dec, nullptr, 0);
        enc.decode(d_msg, d_out, 1, d_enc, 0);
        const std::vector<T> got = download(d_out, n);
        for (size_t r = 0; r < 2; r++)
            for (size_t c = 0; c < half; c++)
            {
                const T want = mulmod(slots[r * half + (c + 1) % half], slots[n + r * half + c], t);
                ok = ok && got[r * half + c] == want;
            }
        std::cout << "slots rotated left by one and multiplied by a plaintext vector: "
                  << (ok ? "as expected" : "WRONG") << std::endl;

        // a plaintext modulus without a 2N-th root of unity is refused
        try
        {
            BfvBatchEncoder<T> bad(Modulus<T>(257), 12, d_fwd_t, d_inv_t, 1, 1, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
        for (void* p : {d_keygen, d_sym, d_pub, d_dec, d_ks, d_hoist, d_enc})
            (void) hipFree(p);
    }
    for (void* p : {(void*) d_s_small, (void*) d_key_err, (void*) d_pk_err, (void*) d_small, (void*) d_s, (void*) d_s_rot,
                    (void*) d_key, (void*) d_pk, (void*) d_values, (void*) d_plain, (void*) d_scaled, (void*) d_ct,
                    (void*) d_a, (void*) d_rot, (void*) d_pt, (void*) d_msg, (void*) d_out, (void*) d_noise,
                    (void*) d_fwd_b, (void*) d_inv_b, (void*) d_fwd_p, (void*) d_inv_p, (void*) d_fwd_t, (void*) d_inv_t})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}
