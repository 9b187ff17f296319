// rns_call_check.cpp -- csrc/rns_call.hpp on the host, no GPU: the overlap refusal against a brute-force definition over
// small synthetic address ranges (no address is ever read), the "may be exactly this write" permission, null operands,
// list order and messages, and the alignment, int-batch, null-pointer and scratch-region helpers at their edges.
//   clang++ -std=c++17 -fsanitize=address,undefined -I gpu-ntt_amd/csrc tests/cpp/rns_call_check.cpp
// prints "OK <checks>"; the first mismatch prints "WRONG ..." and exits 1.  An argument names one scenario.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rns_call.hpp"

using namespace gpuntt::host;

static unsigned long long checks = 0;
#define CHECK(cond, ...)                                                                                                 \
    do                                                                                                                   \
    {                                                                                                                    \
        checks++;                                                                                                        \
        if (!(cond))                                                                                                     \
        {                                                                                                                \
            std::printf("WRONG %s:%d %s: ", __FILE__, __LINE__, #cond);                                                  \
            std::printf(__VA_ARGS__);                                                                                    \
            std::printf("\n");                                                                                           \
            std::exit(1);                                                                                                \
        }                                                                                                                \
    } while (0)

static const std::uintptr_t BASE = 0x10000; // 256-byte aligned
static const void* at(std::uintptr_t offset) { return reinterpret_cast<const void*>(BASE + offset); }

// The definition: two ranges overlap when they share a byte.  A range of no bytes shares none; rns_overlap counts it as
// overlapping where it lies strictly inside the other range (between two of its bytes), and so does this
static bool brute(std::uintptr_t a, std::uint64_t la, std::uintptr_t b, std::uint64_t lb)
{
    bool bytes_a[64] = {}, hit = false;
    for (std::uint64_t i = 0; i < la; i++)
        bytes_a[a + i] = true;
    for (std::uint64_t i = 0; i < lb; i++)
        hit = hit || bytes_a[b + i];
    if (la == 0 && lb > 0)
        return b < a && a < b + lb;
    if (lb == 0 && la > 0)
        return a < b && b < a + la;
    return hit;
}

// the message refuse_overlap throws, "" when it accepts
static std::string refusal(std::initializer_list<RnsRange> writes, std::initializer_list<RnsRange> reads, const char* message)
{
    try
    {
        refuse_overlap(writes, reads, message);
    }
    catch (const std::invalid_argument& e)
    {
        return e.what();
    }
    return "";
}

// every pair of ranges of 0 .. 6 bytes in a window of 16: adjacent, nested, identical, zero-length, the same start with
// another length
static void every_small_pair()
{
    for (std::uintptr_t a = 0; a < 16; a++)
        for (std::uint64_t la = 0; la <= 6; la++)
            for (std::uintptr_t b = 0; b < 16; b++)
                for (std::uint64_t lb = 0; lb <= 6; lb++)
                {
                    const bool want = brute(a, la, b, lb);
                    CHECK(rns_overlap(at(a), la, at(b), lb) == want, "rns_overlap %d+%d %d+%d", (int) a, (int) la, (int) b,
                          (int) lb);
                    CHECK((refusal({{at(a), la}}, {{at(b), lb}}, "m") == "m") == want, "refuse %d+%d %d+%d", (int) a,
                          (int) la, (int) b, (int) lb);
                    // the permission holds for the same start only, whatever the lengths
                    const bool permitted = want && a != b;
                    CHECK((refusal({{at(a), la}}, {{at(b), lb, true}}, "m") == "m") == permitted, "exact %d+%d %d+%d",
                          (int) a, (int) la, (int) b, (int) lb);
                }
}

static void named_cases()
{
    CHECK(refusal({{at(0), 8}}, {{at(8), 8}}, "m") == "", "adjacent ranges do not overlap");
    CHECK(refusal({{at(8), 8}}, {{at(0), 8}}, "m") == "", "adjacent ranges, the other way");
    CHECK(refusal({{at(0), 8}}, {{at(7), 8}}, "m") == "m", "one shared byte");
    CHECK(refusal({{at(0), 16}}, {{at(4), 4}}, "m") == "m", "nested");
    CHECK(refusal({{at(4), 4}}, {{at(0), 16}}, "m") == "m", "nested, the other way");
    CHECK(refusal({{at(0), 8}}, {{at(0), 8}}, "m") == "m", "identical without the permission");
    CHECK(refusal({{at(0), 8}}, {{at(0), 8, true}}, "m") == "", "identical with the permission");
    CHECK(refusal({{at(0), 8}}, {{at(0), 4, true}}, "m") == "", "the same start, shorter, with the permission");
    CHECK(refusal({{at(0), 8}}, {{at(0), 4}}, "m") == "m", "the same start, shorter, without it");
    CHECK(refusal({{at(0), 8}}, {{at(1), 8, true}}, "m") == "m", "one byte off despite the permission");
    CHECK(refusal({{at(0), 0}}, {{at(0), 8}}, "m") == "", "no bytes at the start of a range");
    CHECK(refusal({{at(8), 0}}, {{at(0), 8}}, "m") == "", "no bytes at the end of a range");
    CHECK(refusal({{at(4), 0}}, {{at(0), 8}}, "m") == "m", "no bytes strictly inside a range: as rns_overlap counts it");
    CHECK(refusal({{at(4), 0}}, {{at(4), 0}}, "m") == "", "two ranges of no bytes");
}

static void null_operands()
{
    // an absent optional operand is skipped whatever its length says, as a write and as a read
    CHECK(refusal({{at(0), 8}}, {{nullptr, ~0ull}}, "m") == "", "a null read");
    CHECK(refusal({{nullptr, ~0ull}}, {{at(0), 8}}, "m") == "", "a null write");
    CHECK(refusal({{nullptr, 8}}, {{nullptr, 8}}, "m") == "", "both null");
    CHECK(refusal({{at(0), 8}}, {{nullptr, 8}, {at(4), 8}}, "m") == "m", "a null read does not hide the next one");
    CHECK(refusal({{nullptr, 8}, {at(0), 8}}, {{at(4), 8}}, "m") == "m", "a null write does not hide the next one");
    CHECK(refusal({{at(0), 8}}, {{nullptr, 8, true}}, "m") == "", "a null read with the permission");
}

static void lists_and_order()
{
    const RnsRange writes[] = {{at(0), 8}, {at(16), 8}, {at(32), 8}};
    const RnsRange apart[] = {{at(8), 8}, {at(24), 8}, {at(40), 8}};
    int w = -1, r = -1;
    CHECK(!first_overlap(writes, 3, apart, 3, w, r) && w == -1 && r == -1, "three writes against three reads, all apart");
    // two offending pairs: (write 1, read 2) and (write 2, read 0); writes are outermost, so (1, 2) is the first
    const RnsRange reads[] = {{at(36), 2}, {at(60), 2}, {at(20), 2}};
    CHECK(first_overlap(writes, 3, reads, 3, w, r) && w == 1 && r == 2, "the first pair in list order: got (%d, %d)", w, r);
    // within one write the reads go in their order
    const RnsRange both[] = {{at(60), 2}, {at(18), 2}, {at(20), 2}};
    CHECK(first_overlap(writes, 3, both, 3, w, r) && w == 1 && r == 1, "reads in their order: got (%d, %d)", w, r);
    // the permission is per read: read 0 may be exactly write 0, read 1 may not
    const RnsRange same[] = {{at(0), 8, true}, {at(16), 8}};
    CHECK(first_overlap(writes, 3, same, 2, w, r) && w == 1 && r == 1, "the permission is per read: got (%d, %d)", w, r);
    // ... and only against the write it starts with: write 1 overlaps read 0 from another start
    const RnsRange shifted[] = {{at(0), 20, true}};
    CHECK(first_overlap(writes, 3, shifted, 1, w, r) && w == 1 && r == 0, "exact against one write only: got (%d, %d)", w, r);
    CHECK(!first_overlap(writes, 0, reads, 3, w, r) && !first_overlap(writes, 3, reads, 0, w, r), "empty lists");
    // the message is the caller's, word for word; the first refusing call of a sequence decides it
    CHECK(refusal({{at(0), 8}, {at(16), 8}}, {{at(4), 2}, {at(18), 2}}, "out or the scratch overlaps an operand!") ==
              "out or the scratch overlaps an operand!",
          "the caller's words");
    std::string got;
    try
    {
        refuse_overlap({{at(0), 8}}, {{at(8), 8}}, "first");
        refuse_overlap({{at(0), 8}}, {{at(4), 8}}, "second");
        refuse_overlap({{at(0), 8}}, {{at(0), 8}}, "third");
    }
    catch (const std::invalid_argument& e)
    {
        got = e.what();
    }
    CHECK(got == "second", "the first refusing call decides: %s", got.c_str());
}

template <typename F> static std::string thrown(F&& f)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument& e)
    {
        return e.what();
    }
    return "";
}

static void alignment_and_batch()
{
    const char* aligned = "The scratch is not 256-byte aligned!";
    CHECK(thrown([] { need_aligned_scratch(at(0)); }) == "", "BASE is aligned");
    CHECK(thrown([] { need_aligned_scratch(at(255)); }) == aligned, "255");
    CHECK(thrown([] { need_aligned_scratch(at(256)); }) == "", "256");
    CHECK(thrown([] { need_aligned_scratch(at(257)); }) == aligned, "257");
    CHECK(thrown([] { need_aligned_scratch(at(8)); }) == aligned, "8");
    CHECK(thrown([] { need_aligned_scratch(nullptr); }) == "", "the null check is need_pointers'");
    CHECK(thrown([] { need_int_batch(0, "Invalid count!"); }) == "", "0");
    CHECK(thrown([] { need_int_batch(0x7FFFFFFFull, "Invalid count!"); }) == "", "0x7FFFFFFF");
    CHECK(thrown([] { need_int_batch(0x80000000ull, "Invalid count!"); }) == "Invalid count!", "0x80000000");
    CHECK(thrown([] { need_int_batch(~0ull, "Invalid stacks!"); }) == "Invalid stacks!", "the caller's words");
    CHECK(rns_align(255) == 256 && rns_align(256) == 256 && rns_align(257) == 512 && rns_align(0) == 0, "rns_align");
}

static void pointers_and_regions()
{
    const char* null = "null pointer argument";
    const int i = 0;
    const double d = 0;
    const int* const list[] = {&i, nullptr};
    const void* v = &d;
    CHECK(thrown([&] { need_pointers(&i); }) == "", "one pointer");
    CHECK(thrown([&] { need_pointers(&i, &d, v, list); }) == "", "pointers of four types");
    CHECK(thrown([&] { need_pointers(static_cast<const int*>(nullptr)); }) == null, "one null pointer");
    CHECK(thrown([&] { need_pointers(&i, &d, static_cast<const void*>(nullptr)); }) == null, "the last one null");
    CHECK(thrown([&] { need_pointers(static_cast<const int*>(nullptr), &d); }) == null, "the first one null");
    CHECK(thrown([&] { need_pointers(list[0]); }) == "" && thrown([&] { need_pointers(list[1]); }) == null, "list entries");
    alignas(256) static unsigned char scratch[1024];
    CHECK(reinterpret_cast<unsigned char*>(words_at<std::uint64_t>(scratch, 0)) == scratch, "offset 0");
    CHECK(reinterpret_cast<unsigned char*>(words_at<std::uint32_t>(scratch, 768)) == scratch + 768, "offset 768");
    words_at<std::uint64_t>(scratch, 256)[3] = 7; // a typed region is usable memory
    CHECK(scratch[256 + 24] == 7, "word 3 of the region at byte 256");
}

int main(int argc, char** argv)
{
    const struct
    {
        const char* name;
        void (*run)();
    } scenarios[] = {{"every_small_pair", every_small_pair},       {"named_cases", named_cases},
                     {"null_operands", null_operands},             {"lists_and_order", lists_and_order},
                     {"alignment_and_batch", alignment_and_batch}, {"pointers_and_regions", pointers_and_regions}};
    int ran = 0;
    for (const auto& s : scenarios)
        if (argc < 2 || std::strcmp(argv[1], s.name) == 0)
        {
            s.run();
            ran++;
        }
    if (ran == 0)
    {
        std::printf("WRONG no scenario named %s\n", argv[1]);
        return 1;
    }
    std::printf("OK %llu\n", checks);
    return 0;
}
