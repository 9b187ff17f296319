// contig_p4_map.hpp -- index maps of the four-polynomial tile of the forward 64-bit contiguous pass (K = 10 stages on a
// 4096-coefficient tile, merge_lazy_kernels.hpp: pass_body<..., P4>).  Plain constexpr functions, host and device: the
// kernel computes its addresses with them and tests/cpp/contig_p4_map_check.cpp walks them on the CPU.
//
// The tile is FOUR polynomials x ONE 1024-coefficient segment of the ring instead of four consecutive segments of one
// polynomial: tile element e = (polynomial << 10) | position in the segment.  The same 256-coefficient block of the four
// polynomials uses identical twiddles, so once a wave holds one block of all four (rounds 1 and 2) the twiddles of
// stage bits 7..4 are wave-uniform (scalar registers) and the four 16-lane rows of a wave read the SAME per-lane
// twiddles in stage bits 3..0.
//
//   round 0 (stage bits 9, 8; register window 6..9)   wave w = polynomial w, lanes = tile bits 0..5
//   -- block-wide exchange --
//   round 1 (stage bits 7..4; register window 4..7)   wave b = tile bits 8, 9; lane bits 0..3 = tile bits 0..3,
//                                                     lane bits 4, 5 = tile bits 10, 11 (the polynomial)
//   round 2 (stage bits 3..0; register window 0..3)   the same threads: tile bits 4..7 move from registers to lanes
//   store window                                      wave b, lanes = tile bits 0..5, registers = tile bits 6, 7 and the
//                                                     polynomial: 512 bytes per store, 2 KiB runs per polynomial and wave
// Rounds 1, 2 and the store window hold the same 1024 elements per wave: those exchanges never leave the wave.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPUNTT_P4_HD __host__ __device__
#else
#define GPUNTT_P4_HD
#endif

namespace gpuntt
{
    namespace kern
    {
        namespace p4
        {
            constexpr int TLOG = 12; // log2 tile
            constexpr int K = 10;    // stages of the pass = log2 segment
            constexpr int RB = 4;    // log2 coefficients per thread
            constexpr int NT = 256;  // threads per block
            constexpr int POLYS = 1 << (TLOG - K);
            constexpr int ROUNDS = 3;
            // one pad element per 16 (lds_pad of the other kernels) + 16 per polynomial: with lane bits 4, 5 on tile bits
            // 10, 11 the plain padding puts the two polynomials of a half-wave 1088 = 34 * 32 elements apart -- the same
            // banks; 1104 elements apart they interleave
            constexpr int LDS_ELEMS = (1 << TLOG) + (1 << (TLOG - 4)) + 16 * (POLYS - 1);

            GPUNTT_P4_HD constexpr int window(int r) { return r == 0 ? 6 : (r == 1 ? 4 : 0); }

            // thread index the register window of round r is laid over
            GPUNTT_P4_HD constexpr unsigned thread_of(int r, unsigned t)
            {
                return r == 0 ? t : ((t & 15u) | ((t >> 6) << 4) | (((t >> 4) & 3u) << 6));
            }
            // thread t, register j of round r -> tile element
            GPUNTT_P4_HD constexpr unsigned elem(int r, unsigned t, unsigned j)
            {
                const unsigned u = thread_of(r, t);
                const int w = window(r);
                return (u & ((1u << w) - 1u)) | (j << w) | ((u >> w) << (w + RB));
            }
            // thread t, register j of the store window -> tile element
            GPUNTT_P4_HD constexpr unsigned elem_out(unsigned t, unsigned j)
            {
                return (t & 63u) | ((j & 3u) << 6) | ((t >> 6) << 8) | ((j >> 2) << K);
            }
            // tile element -> LDS slot
            GPUNTT_P4_HD constexpr unsigned lds_slot(unsigned e) { return e + (e >> 4) + ((e >> K) << 4); }
            // tile element -> offset from the tile's base (first polynomial, first coefficient of the segment);
            // poly_stride = coefficients between two polynomials of the tile: 2^n, or mod_count * 2^n in an RNS stack
            GPUNTT_P4_HD constexpr unsigned long long mem_offset(unsigned e, unsigned long long poly_stride)
            {
                return static_cast<unsigned long long>(e >> K) * poly_stride + (e & ((1u << K) - 1u));
            }
            // ring position of tile element e of segment seg (every polynomial of the tile alike)
            GPUNTT_P4_HD constexpr unsigned ring_pos(unsigned seg, unsigned e) { return (seg << K) | (e & ((1u << K) - 1u)); }

            // Prepared-table index (prep.hip, table laid out for 4096-coefficient tiles) of entry kk of stage bit p.
            // Rounds 0 and 1: uniform over the wave -- blk = 0 in round 0, tile bits 8, 9 = the wave in round 1;
            // entry kk follows the register bits above p.
            GPUNTT_P4_HD constexpr unsigned tw_uniform_index(int n, unsigned seg, unsigned blk, int p, unsigned kk)
            {
                return (1u << (n - 1 - p)) + (((seg << K) | (blk << 8)) >> (p + 1)) + kk;
            }
            // Round 2 (p = 3 .. 0): the [tile][k][thread] layout of the distance-1/2/4 stages and the plain layout of
            // stage 3 agree on  stage + tile * (CNT * 256) + k * 256 + group  with CNT = 8 >> p entries per thread and
            // group = the thread's 16-coefficient group inside the 4096-coefficient tile of the RING it lies in
            GPUNTT_P4_HD constexpr unsigned tw_lane_index(int n, unsigned seg, unsigned t, int p, unsigned kk)
            {
                const unsigned group = ((seg & 3u) << 6) | ((t >> 6) << 4) | (t & 15u);
                return (1u << (n - 1 - p)) + (seg >> 2) * ((8u >> p) * NT) + kk * NT + group;
            }
        } // namespace p4

        // The hoisted first twiddle product of the last pass (merge_lazy_kernels.hpp: pass_body<..., PRE>).  The first
        // stage of the 10-stage last pass -- distance 512 inside a 1024-coefficient segment -- multiplies the elements
        // with ring bit 9 set by a twiddle that depends on the segment alone.  The strided pass in front of it (K stages
        // on a 4096-coefficient tile of 2^K rows x 2^(12-K) columns, row = segment) does that product on its way out and
        // stores T = V w in V's place; the last pass then starts from U' = U + T, V' = 2 U + 4 q - U'.
        namespace premul
        {
            constexpr int BIT = p4::K - 1; // ring bit of the hoisted stage
            // the hoisted stage's operand V lies at this ring position
            GPUNTT_P4_HD constexpr bool premultiplied(unsigned ring_pos) { return ((ring_pos >> BIT) & 1u) != 0u; }
            // prepared-table index the STRIDED pass reads for the element at ring position ring_pos
            GPUNTT_P4_HD constexpr unsigned tw_index(int n, unsigned ring_pos)
            {
                return (1u << (n - 1 - BIT)) + (ring_pos >> (BIT + 1));
            }
            // the index the last pass reads today for the same stage of segment seg
            GPUNTT_P4_HD constexpr unsigned tw_index_contig(int n, unsigned seg) { return p4::tw_uniform_index(n, seg, 0u, BIT, 0u); }
            // strided pass of k stages, last register round (window at tile bit 12 - k): thread t, register j -> tile element
            GPUNTT_P4_HD constexpr unsigned strided_elem(int k, unsigned t, unsigned j)
            {
                const int w = p4::TLOG - k;
                return (t & ((1u << w) - 1u)) | (j << w) | ((t >> w) << (w + p4::RB));
            }
            // ring position of element e of tile b of a polynomial (kern::LTileMap, STRIDED, p_lo = n - k)
            GPUNTT_P4_HD constexpr unsigned strided_ring_pos(int n, int k, unsigned b, unsigned e)
            {
                const int l = p4::TLOG - k, p_lo = n - k;
                const unsigned xb = b & ((1u << (p_lo - l)) - 1u), hi = b >> (p_lo - l);
                return ((hi << (p_lo + k)) | (xb << l)) + (((e >> l) << p_lo) | (e & ((1u << l) - 1u)));
            }
        } // namespace premul
    } // namespace kern
} // namespace gpuntt
