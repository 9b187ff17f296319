// example_bfv_dot_product.cpp -- a C++ caller of BfvMultiplyPlan<T>::multiply_relinearize_sum and multiply_sum
// (gpuntt/rns/bfv_multiply.cuh): an encrypted dot product of three pairs of messages, sum_t m_t m'_t, formed on the GPU
// in ONE call -- one division by Q, one key switch, one ModDown -- and decrypted on the host under (1, s).
//
//   base q = {q0} (Q = q0), auxiliary base {b0, b1}, special base {p0} (P = p0); plaintext modulus t, Delta = Q / t.
//     encrypt:      ct = (Delta m + e - a s, a) mod Q, s ternary, e in {-1, 0, 1}, a uniform         -- on the host
//     key:          (-a' s + P s^2, a') over {q0, p0}, one digit (alpha = 1), in NTT form            -- on the host + NTT
//     the sum:      out = relinearize(round(t sum_t (x_t (x) y_t) / Q)), two components              -- ONE call
//     decrypt:      round(t (out0 + out1 s) / Q) mod t  =  sum_t m_t m'_t mod (t, X^N + 1)           -- on the host
//   The second term squares a ciphertext and the third shares its x with the first: four distinct operands in all,
//   each extended and transformed once.  In coefficient form, through the NTT-form entry of the same call, and once
//   more as the two calls of the definition: multiply_sum, then relinearize on the three components it returned -- the
//   same words; the digest of each is printed.
//
//   ./example_bfv_dot_product <LOGN <= 12 (u32: 5)> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/bfv_multiply.cuh"
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
template <typename T> std::vector<T> download(const T* d, size_t words)
{
    std::vector<T> h(words);
    GPUNTT_CUDA_CHECK(hipMemcpy(h.data(), d, words * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

// a * b in Z_q[X] / (X^N + 1), canonical words
template <typename T> std::vector<T> negacyclic(const std::vector<T>& a, const std::vector<T>& b, T q)
{
    const size_t n = a.size();
    std::vector<T> out(n, 0);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++)
        {
            const T p = mulmod(a[i], b[j], q);
            T& o = out[(i + j) % n];
            o = (i + j < n) ? static_cast<T>((static_cast<U128>(o) + p) % q) : static_cast<T>((static_cast<U128>(o) + q - p) % q);
        }
    return out;
}

template <typename T> int run(int logn, const Prime<T> (&primes)[4], int max_logn, T t)
{
    using namespace gpuntt;
    constexpr int L = 1, KB = 2, KP = 1, count = 1;
    constexpr int MB = L + KB, MP = L + KP; // the two full bases: {q0, b0, b1} and {q0, p0}
    const size_t n = size_t(1) << logn;
    const auto poly = ReductionPolynomial::X_N_plus;

    // one table set per full base, modulus m of the base at m << n_power: primes 0 1 2 and primes 0 3
    auto tables = [&](const std::vector<int>& which, std::vector<Modulus<T>>& mods, std::vector<Root<T>>& fwd,
                      std::vector<Root<T>>& inv, std::vector<Ninverse<T>>& ninv) {
        fwd.resize(which.size() * n), inv.resize(which.size() * n);
        for (size_t m = 0; m < which.size(); m++)
        {
            const Prime<T>& p = primes[which[m]];
            const T psi = powmod<T>(p.psi, std::uint64_t(1) << (max_logn - logn), p.q);
            NTTParameters<T> prm(logn, NTTFactors<T>(Modulus<T>(p.q), mulmod(psi, psi, p.q), psi), poly);
            const auto f = prm.gpu_root_of_unity_table_generator(prm.forward_root_of_unity_table);
            const auto b = prm.gpu_root_of_unity_table_generator(prm.inverse_root_of_unity_table);
            std::copy(f.begin(), f.end(), fwd.begin() + m * n);
            std::copy(b.begin(), b.end(), inv.begin() + m * n);
            mods.push_back(prm.modulus);
            ninv.push_back(prm.n_inv);
        }
    };
    std::vector<Modulus<T>> mods_b, mods_p;
    std::vector<Root<T>> fwd_b, inv_b, fwd_p, inv_p;
    std::vector<Ninverse<T>> ninv_b, ninv_p;
    tables({0, 1, 2}, mods_b, fwd_b, inv_b, ninv_b);
    tables({0, 3}, mods_p, fwd_p, inv_p, ninv_p);
    const T Q = primes[0].q, P = primes[3].q, delta = Q / t;

    std::mt19937_64 rng(43);
    std::vector<T> s(n);
    for (auto& v : s)
        v = static_cast<T>(rng() % 3); // 0, 1, 2 stands for 0, 1, -1
    auto secret = [&](T m) { // s modulo m
        std::vector<T> r(n);
        for (size_t i = 0; i < n; i++)
            r[i] = s[i] == 2 ? static_cast<T>(m - 1) : s[i];
        return r;
    };
    const std::vector<T> sq = secret(Q), sp = secret(P);
    auto encrypt = [&](const std::vector<T>& m) { // T[2][count][L][N]
        std::vector<T> a(n), ct(2 * n);
        for (auto& v : a)
            v = static_cast<T>(rng() % Q);
        const std::vector<T> as = negacyclic(a, sq, Q);
        for (size_t i = 0; i < n; i++)
        {
            const T e = static_cast<T>((rng() % 3 + Q - 1) % Q);
            ct[i] = static_cast<T>((static_cast<U128>(mulmod(delta, m[i], Q)) + e + Q - as[i]) % Q);
            ct[n + i] = a[i];
        }
        return ct;
    };
    auto decrypt = [&](const std::vector<T>& out) { // T[2][count][L][N], under (1, s)
        const std::vector<T> c0(out.begin(), out.begin() + n), c1(out.begin() + n, out.end());
        const std::vector<T> p1 = negacyclic(c1, sq, Q);
        std::vector<T> m(n);
        for (size_t i = 0; i < n; i++)
        {
            const T v = static_cast<T>((static_cast<U128>(c0[i]) + p1[i]) % Q);
            // round(t v / Q) mod t of the centred v: for v >= Q / 2 the centred value is v - Q, and t (v - Q) / Q = t v / Q - t
            m[i] = static_cast<T>(((static_cast<U128>(v) * t * 2 + Q) / (2 * static_cast<U128>(Q))) % t);
        }
        return m;
    };
    // the relinearization key T[D = 1][2][MP][N], coefficient form: a' is ONE integer polynomial (below min(Q, P)), so
    // its two limbs are its residues; limb q0 of component 0 carries P s^2, limb p0 does not (P = 0 mod p0).  Noiseless
    std::vector<T> key(2 * MP * n);
    {
        std::vector<T> a(n);
        for (auto& v : a)
            v = static_cast<T>(rng() % (Q < P ? Q : P));
        const std::vector<T> as_q = negacyclic(a, sq, Q), as_p = negacyclic(a, sp, P), s2 = negacyclic(sq, sq, Q);
        for (size_t i = 0; i < n; i++)
        {
            key[i] = static_cast<T>((static_cast<U128>(mulmod(static_cast<T>(P % Q), s2[i], Q)) + Q - as_q[i]) % Q);
            key[n + i] = static_cast<T>((P - as_p[i]) % P);
            key[MP * n + i] = a[i], key[MP * n + n + i] = a[i];
        }
    }
    // four messages a, b, c, d; the sum a b + c c + a d
    std::vector<std::vector<T>> msg(4, std::vector<T>(n));
    for (auto& m : msg)
        for (auto& v : m)
            v = static_cast<T>(rng() % t);
    std::vector<T> want(n, 0); // below 3 N t^2 < Q / 2: the sum over the integers, reduced modulo t next
    for (const auto& pr : {std::pair<int, int>{0, 1}, {2, 2}, {0, 3}})
    {
        const std::vector<T> p = negacyclic(msg[pr.first], msg[pr.second], Q);
        for (size_t i = 0; i < n; i++)
            want[i] = static_cast<T>((static_cast<U128>(want[i]) + p[i]) % Q);
    }
    for (size_t i = 0; i < n; i++)
    {
        const T w = want[i];
        want[i] = w > Q / 2 ? static_cast<T>((t - (Q - w) % t) % t) : static_cast<T>(w % t);
    }
    constexpr int terms = 3, operands = 4;
    T* d_op[operands];
    for (int i = 0; i < operands; i++)
        d_op[i] = upload(encrypt(msg[i]));
    const T* xs[terms] = {d_op[0], d_op[2], d_op[0]};
    const T* ys[terms] = {d_op[1], d_op[2], d_op[3]};
    auto digest = [](const std::vector<T>& v) { // FNV-1a over the words
        std::uint64_t h = 1469598103934665603ull;
        for (T w : v)
            h = (h ^ static_cast<std::uint64_t>(w)) * 1099511628211ull;
        return h;
    };

    T *d_key = upload(key), *d_out = nullptr, *d_three = nullptr;
    Root<T>*d_fwd_b = upload(fwd_b), *d_inv_b = upload(inv_b), *d_fwd_p = upload(fwd_p), *d_inv_p = upload(inv_p);
    GPUNTT_CUDA_CHECK(hipMalloc(&d_out, 2 * n * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_three, 3 * n * sizeof(T)));
    void *d_scratch = nullptr, *d_ks_scratch = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, BfvMultiplyPlan<T>::sum_scratch_bytes(L, KB, logn, count, operands)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_ks_scratch, KeySwitchPlan<T>::scratch_bytes(L, KP, 1, logn, count, 2)));

    bool ok = true;
    {
        BfvMultiplyPlan<T> bfv(mods_b.data(), L, mods_b.data() + L, KB, t, logn, d_fwd_b, d_inv_b, ninv_b.data(), poly,
                               2 * operands * count * MB, 0);
        KeySwitchPlan<T> ks(mods_p.data(), L, mods_p.data() + L, KP, 1, logn, d_fwd_p, d_inv_p, ninv_p.data(), poly,
                            2 * count * MP, MP, nullptr, 0);
        NTTPlan<T> ntt_p(d_fwd_p, mods_p.data(), MP, logn, poly, FORWARD, nullptr, 2 * MP, 0);
        NTTPlan<T> ntt_q(d_fwd_p, mods_p.data(), L, logn, poly, FORWARD, nullptr, 2 * count * L, 0);
        NTTPlan<T> intt_q(d_inv_p, mods_p.data(), L, logn, poly, INVERSE, ninv_p.data(), 2 * count * L, 0);
        ntt_p.execute(d_key, d_key, 2 * MP, 0); // the key lives in NTT form
        ok = ok && ks.modulus(0).value == bfv.modulus(0).value && ks.reduction_poly() == bfv.reduction_poly();
        ok = ok && bfv.max_terms() >= terms;

        // coefficient form in, coefficient form out
        bfv.multiply_relinearize_sum(xs, ys, terms, ks, d_key, d_out, count, false, false, d_scratch, d_ks_scratch, 0);
        const std::vector<T> coeff = download(d_out, 2 * n);
        ok = ok && decrypt(coeff) == want;
        std::cout << "digest coefficient form " << digest(coeff) << std::endl;

        // the definition: multiply_sum, then relinearize on the three components -- the same words
        bfv.multiply_sum(xs, ys, terms, d_three, count, false, false, d_scratch, 0);
        ks.relinearize(d_three, d_three + 2 * count * L * n, d_key, d_three, count, false, false, d_ks_scratch, 0);
        const std::vector<T> two_calls = download(d_three, 2 * n);
        ok = ok && two_calls == coeff;
        std::cout << "digest multiply_sum then relinearize " << digest(two_calls) << std::endl;

        // NTT form in, NTT form out: the same two components, transformed
        for (T* op : d_op)
            ntt_q.execute(op, op, 2 * count * L, 0);
        bfv.multiply_relinearize_sum(xs, ys, terms, ks, d_key, d_out, count, true, true, d_scratch, d_ks_scratch, 0);
        intt_q.execute(d_out, d_out, 2 * count * L, 0);
        const std::vector<T> through_ntt = download(d_out, 2 * n);
        ok = ok && through_ntt == coeff;
        std::cout << "digest NTT form " << digest(through_ntt) << std::endl;

        // more terms than BFV_MAX_TERMS are refused before anything is launched
        try
        {
            bfv.multiply_sum(xs, ys, BFV_MAX_TERMS + 1, d_three, count, true, true, d_scratch, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_op[0], (void*) d_op[1], (void*) d_op[2], (void*) d_op[3], (void*) d_key, (void*) d_out,
                    (void*) d_three, (void*) d_fwd_b, (void*) d_inv_b, (void*) d_fwd_p, (void*) d_inv_p, d_scratch,
                    d_ks_scratch})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 2) ? std::atoi(argv[1]) : 10;
    const bool u32 = (argc >= 3) && std::string(argv[2]) == "u32";
    // one q-prime is all the noise budget there is: t and N stay small (N t^2 and t^2 N^2 far below Q / t)
    if (logn < 1 || logn > (u32 ? 5 : 12))
        return EXIT_FAILURE;
    if (u32)
        return run<Data32>(logn,
                           {{536641537u, 167028958u}, {536608769u, 417302965u}, {1073643521u, 269685106u},
                            {536543233u, 254502220u}},
                           14, 17u);
    return run<Data64>(logn,
                       {{576460752300015617ull, 296969298802020438ull},
                        {576460752298835969ull, 132309083155986965ull},
                        {1152921504598720513ull, 560939867933173424ull},
                        {576460752298180609ull, 283462520361873529ull}},
                       16, 257ull);
}
