// rns_host.hpp -- the small host helpers every RNS plan shares (base_conversion.hip, inner_product.hip, key_switch.hip,
// bfv_multiply.hip): alignment, byte-range overlap, the n_power check, the column tiles of a launch with HIP's grid
// limit, the output-split loop and the constants of the three-word fold (bc_fold, IpFold).  One copy of each; a refusal
// whose words differ between callers takes them as an argument.  Not a public header.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>

namespace gpuntt
{
    namespace host
    {
        // bytes rounded up to the 256-byte granule of every workspace and scratch layout
        inline size_t rns_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

        // do [a, a + a_bytes) and [b, b + b_bytes) share a byte?
        inline bool rns_overlap(const void* a, std::uint64_t a_bytes, const void* b, std::uint64_t b_bytes)
        {
            const auto al = reinterpret_cast<uintptr_t>(a), bl = reinterpret_cast<uintptr_t>(b);
            return al < bl + b_bytes && bl < al + a_bytes;
        }

        inline void rns_check_n_power(int n_power)
        {
            if (n_power <= 0 || n_power >= 29)
                throw std::invalid_argument("Invalid n_power range!");
        }

        // workgroups of nt lanes that cover `total` columns; HIP caps a launch at 2^32 - 1 work-items per dimension:
        // beyond that, std::invalid_argument(message)
        inline unsigned long long column_tiles(unsigned long long total, unsigned nt, const char* message)
        {
            const unsigned long long tiles = (total + nt - 1) / nt;
            if (tiles * nt > 0xFFFFFFFFull)
                throw std::invalid_argument(message);
            return tiles;
        }

        // Workgroups per column tile, out of `units` pieces of a tile's outputs.  A workgroup that owns all of a tile's
        // outputs reads the input once.  Below two workgroups per CU (256 CUs) the pieces are spread over up to 8
        // workgroups per tile, which re-read the tile's input from L2 and recompute what they park in LDS.  Both numbers
        // are estimates (two workgroups per CU as the fill target), not measured: DESIGN.md 3.10.  forced > 0 (a test
        // hook's value) replaces the choice
        inline int rns_split(unsigned long long tiles, int units, int forced)
        {
            int s = 1;
            if (forced > 0)
                s = forced;
            else
                while (s < 8 && tiles * s < 512)
                    s *= 2;
            return s < units ? s : units;
        }

        // the constants of bc_fold (base_conversion_internal.hpp) and IpFold (inner_product_internal.hpp) for modulus m
        // and word width W: 2^W mod m, 2^2W mod m, their Shoup companions floor(v 2^W / m), and the companion of 1
        struct RnsFoldConsts
        {
            std::uint64_t t1, t1p, t2, t2p, onep;
        };
        inline RnsFoldConsts rns_fold_consts(std::uint64_t m, int W)
        {
            using U128 = unsigned __int128;
            auto shoup = [&](std::uint64_t v) { return static_cast<std::uint64_t>((static_cast<U128>(v) << W) / m); };
            const std::uint64_t t1 = static_cast<std::uint64_t>((static_cast<U128>(1) << W) % m);
            const std::uint64_t t2 = static_cast<std::uint64_t>(static_cast<U128>(t1) * t1 % m);
            return RnsFoldConsts{t1, shoup(t1), t2, shoup(t2), shoup(1)};
        }
    } // namespace host
} // namespace gpuntt
