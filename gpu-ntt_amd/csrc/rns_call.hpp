// rns_call.hpp -- the argument checks every pipeline call of the RNS plans makes before its first launch (key_switch.hip,
// bfv_multiply.hip, bfv_encode.hip): null pointers, the scratch alignment, the int batch of the transforms, byte-range
// overlaps, and the typed regions of a scratch.  Host only: nothing of HIP, no allocation; a plain host compiler builds
// it (tests/cpp/rns_call_check.cpp).  As in rns_host.hpp, a refusal whose words differ between callers takes them as an
// argument.  Not a public header.
#pragma once

#include <cstdint>
#include <initializer_list>
#include <stdexcept>

#include "rns_host.hpp"

namespace gpuntt
{
    namespace host
    {
        // [p, p + bytes); as a read, exact: the range may be exactly the write it is compared with (the same start)
        struct RnsRange
        {
            const void* p;
            std::uint64_t bytes;
            bool exact = false;
        };

        template <typename... P> void need_pointers(const P*... p)
        {
            for (const bool null : {(p == nullptr)...})
                if (null)
                    throw std::invalid_argument("null pointer argument");
        }

        inline void need_aligned_scratch(const void* scratch)
        {
            if (reinterpret_cast<uintptr_t>(scratch) % 256 != 0)
                throw std::invalid_argument("The scratch is not 256-byte aligned!");
        }

        // the batch of a transform (stacks times limbs) is an int
        inline void need_int_batch(unsigned long long stacks_times_limbs, const char* message)
        {
            if (stacks_times_limbs > 0x7FFFFFFFull)
                throw std::invalid_argument(message);
        }

        // The first (write, read) pair, writes outermost, that shares a byte as rns_overlap counts it (so a zero-length
        // range strictly inside another one does).  A null range is an absent optional operand and is skipped; a read
        // marked exact is skipped against a write with its start.  Returns false when there is none
        inline bool first_overlap(const RnsRange* writes, int write_count, const RnsRange* reads, int read_count,
                                  int& write_hit, int& read_hit)
        {
            for (int w = 0; w < write_count; w++)
                for (int r = 0; r < read_count; r++)
                {
                    const RnsRange &a = writes[w], &b = reads[r];
                    if (a.p == nullptr || b.p == nullptr || (b.exact && b.p == a.p))
                        continue;
                    if (rns_overlap(a.p, a.bytes, b.p, b.bytes))
                    {
                        write_hit = w, read_hit = r;
                        return true;
                    }
                }
            return false;
        }

        inline void refuse_overlap(std::initializer_list<RnsRange> writes, std::initializer_list<RnsRange> reads,
                                   const char* message)
        {
            int w = 0, r = 0;
            if (first_overlap(writes.begin(), static_cast<int>(writes.size()), reads.begin(),
                              static_cast<int>(reads.size()), w, r))
                throw std::invalid_argument(message);
        }

        // the region of a scratch that starts byte_offset bytes in, as words
        template <typename T> T* words_at(void* scratch, std::uint64_t byte_offset)
        {
            return reinterpret_cast<T*>(static_cast<char*>(scratch) + byte_offset);
        }
    } // namespace host
} // namespace gpuntt
