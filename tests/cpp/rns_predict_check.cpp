// rns_predict_check.cpp -- host check of csrc/rns_predict.hpp (no GPU, no library): the rules by which host::rns_guess
// predicts the lazy family of a drop-in RNS call.  This program plays the device: between calls it writes into a slot's
// word the state a finished call of that stack would publish (kern::prep_twiddles: *host_state = state) -- or leaves the
// word alone, for a call that has not finished.  Compiled for the host with AddressSanitizer and UBSan
// (tests/test_rns_predict_host.py).  Prints "OK <checks>" and returns 0, or the first mismatch and 1.
//
// What a stack publishes: 60-bit primes GO_LAZY (forward, every 31 q < 2^64: GO_LAZY_31Q), a 61-bit prime GO_LAZY_8Q, a
// 62-bit prime GO_LAZY_4Q, a modulus outside the domain GO_GENERIC.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rns_predict.hpp"

namespace pr = gpuntt::host::predict;

static unsigned long long checks = 0;
#define REQUIRE(cond, ...)                                                                                               \
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

namespace
{
    constexpr unsigned W60 = pr::GO_LAZY, W60_31 = pr::GO_LAZY_31Q, W61 = pr::GO_LAZY_8Q, W62 = pr::GO_LAZY_4Q,
                       OUT = pr::GO_GENERIC;
    constexpr int U64_FWD = 8, U64_INV = 8 | 0x100, U32_FWD = 4, U64_4STEP = 8 | 0x40;

    // one process: the rules, the word pools of two devices (filled with a value no rule may ever read as a state) and
    // a supply of moduli buffer addresses that are never dereferenced
    struct World
    {
        pr::Table table;
        std::vector<unsigned> pool[2];
        std::vector<char> addresses;
        size_t next_address = 0;
        World() : addresses(1 << 16)
        {
            for (auto& p : pool)
                p.assign(pr::MAX_KEYS * pr::STRIDE, 0xdeadbeefu);
        }
        const void* fresh_buffer() { return &addresses.at(next_address++); }
        pr::Answer call(const void* moduli, int mod_count = 5, int word_dir = U64_FWD, const void* order = nullptr,
                        int dev = 0, bool exact = false)
        {
            const pr::Answer a = table.guess(pool[dev].data(), dev, moduli, order, mod_count, word_dir, exact);
            REQUIRE(a.word >= 0 && static_cast<size_t>(a.word) < pr::MAX_KEYS, "word %d", a.word);
            REQUIRE((a.state >= pr::GO_LAZY && a.state <= pr::GO_LAZY_31Q) || exact, "state %u is no family", a.state);
            return a;
        }
        // the call that got answer `a` has finished: its preparation kernel found `state`
        void finish(const pr::Answer& a, unsigned state, int dev = 0) { pool[dev][a.word * pr::STRIDE] = state; }
        unsigned word(const pr::Answer& a, int dev = 0) const { return pool[dev][a.word * pr::STRIDE]; }
        // a call on a buffer never seen before that finishes before the next one starts
        pr::Answer fresh_call(unsigned stack, int mod_count = 5, int word_dir = U64_FWD, const void* order = nullptr,
                              int dev = 0)
        {
            const pr::Answer a = call(fresh_buffer(), mod_count, word_dir, order, dev);
            REQUIRE(a.unsure, "a buffer never seen before must be unsure (large rings cast the wide net on it)");
            finish(a, stack, dev);
            return a;
        }
    };

    void fresh_buffer_per_call()
    {
        World w;
        pr::Answer a = w.call(w.fresh_buffer());
        REQUIRE(a.state == pr::GO_LAZY && a.unsure, "call 1: state %u unsure %d", a.state, a.unsure);
        REQUIRE(w.word(a) == pr::STATE_UNKNOWN, "a new slot's word reads unknown");
        w.finish(a, W61);
        for (int i = 2; i <= 40; i++)
        {
            a = w.fresh_call(W61);
            REQUIRE(a.state == pr::GO_LAZY_8Q, "call %d on a fresh buffer: state %u, want the 8 q family", i, a.state);
        }
    }

    void word_not_yet_written()
    {
        World w;
        const pr::Answer a1 = w.call(w.fresh_buffer());
        const pr::Answer a2 = w.call(w.fresh_buffer()); // call 1 has not finished
        REQUIRE(a2.state == pr::GO_LAZY && a2.unsure, "call 2 before call 1 finished: state %u", a2.state);
        const pr::Answer a3 = w.call(w.fresh_buffer());
        REQUIRE(a3.state == pr::GO_LAZY && a3.unsure, "call 3: state %u", a3.state);
        w.finish(a1, W61); // now it has; an older value is as good
        const pr::Answer a4 = w.call(w.fresh_buffer());
        REQUIRE(a4.state == pr::GO_LAZY_8Q && a4.unsure, "call 4 after call 1 finished: state %u", a4.state);
        // more calls in flight than the hint looks back on: nothing is learnt from the forgotten ones, nothing is wrong
        World v;
        std::vector<pr::Answer> flight;
        for (int i = 0; i < 3 * pr::HINT_RECENT; i++)
            flight.push_back(v.call(v.fresh_buffer()));
        for (const pr::Answer& f : flight)
            v.finish(f, W62);
        REQUIRE(v.call(v.fresh_buffer()).state == pr::GO_LAZY_4Q, "the last calls of the burst are heard");
    }

    void a_hint_does_not_hide_a_wider_stack()
    {
        World w;
        w.fresh_call(W61);
        REQUIRE(w.fresh_call(W61).state == pr::GO_LAZY_8Q, "shape hinted 8 q");
        const pr::Answer a = w.fresh_call(W62);
        REQUIRE(a.state == pr::GO_LAZY_8Q, "the 62-bit stack's own call is predicted from the hint: %u", a.state);
        REQUIRE(w.fresh_call(W62).state == pr::GO_LAZY_4Q, "the next fresh buffer gets the 4 q family");
        REQUIRE(w.fresh_call(W61).state == pr::GO_LAZY_4Q, "and one narrower call does not take it back");
    }

    void narrowing()
    {
        for (const int restart_at : {-1, 7})
        {
            World w;
            w.fresh_call(W61);
            pr::Answer a = w.fresh_call(W60); // hears the 61-bit stack: 8 q
            REQUIRE(a.state == pr::GO_LAZY_8Q, "hinted 8 q: %u", a.state);
            int narrow_seen = 0; // 60-bit observations the hint has heard in a row; one more waits in a's word
            for (int i = 0; i < 40; i++)
            {
                const bool wide = i == restart_at;
                a = w.fresh_call(wide ? W61 : W60); // hears the call before it
                narrow_seen++;
                const bool narrowed = narrow_seen >= pr::NARROW_AFTER;
                REQUIRE(a.state == (narrowed ? pr::GO_LAZY : pr::GO_LAZY_8Q), "restart %d, call %d after %d narrow observations: %u",
                        restart_at, i, narrow_seen, a.state);
                if (narrowed)
                    break;
                if (wide)
                    narrow_seen = -1; // the next call hears the 61-bit one: the count starts again at 0
            }
            REQUIRE(narrow_seen == pr::NARROW_AFTER, "narrowed after %d observations", narrow_seen);
        }
        // the hint narrows to the WIDEST family of the streak
        World w;
        w.fresh_call(W62);
        for (int i = 0; i < pr::NARROW_AFTER; i++)
            REQUIRE(w.fresh_call(i == 3 ? W61 : W60_31).state == pr::GO_LAZY_4Q, "i %d", i);
        REQUIRE(w.fresh_call(W60_31).state == pr::GO_LAZY_8Q, "16 narrower observations, the widest a 61-bit stack");
    }

    void alternating_stacks()
    {
        World w;
        w.fresh_call(W60);
        w.fresh_call(W61);
        for (int i = 0; i < 100; i++)
            REQUIRE(w.fresh_call(i % 2 ? W61 : W60).state == pr::GO_LAZY_8Q, "call %d", i);
    }

    void shape_isolation()
    {
        World w;
        static const int order_array[5] = {0, 1, 2, 3, 4};
        w.fresh_call(W62);
        REQUIRE(w.fresh_call(W62).state == pr::GO_LAZY_4Q, "the shape itself is hinted");
        REQUIRE(w.fresh_call(W60, 4).state == pr::GO_LAZY, "another mod_count");
        REQUIRE(w.fresh_call(W60, 5, U64_INV).state == pr::GO_LAZY, "the other direction");
        REQUIRE(w.fresh_call(W60, 5, U32_FWD).state == pr::GO_LAZY, "the other word size");
        REQUIRE(w.fresh_call(W60, 5, U64_4STEP).state == pr::GO_LAZY, "the 4-step entry");
        REQUIRE(w.fresh_call(W60, 5, U64_FWD, order_array).state == pr::GO_LAZY, "an ordered call");
        REQUIRE(w.fresh_call(W60, 5, U64_FWD, nullptr, 1).state == pr::GO_LAZY, "another device");
        REQUIRE(w.fresh_call(W60, 5, U64_FWD, order_array).state == pr::GO_LAZY, "ordered calls have a hint of their own");
        REQUIRE(w.fresh_call(W62).state == pr::GO_LAZY_4Q, "and none of them touched the first shape's");
        // one buffer, two directions: two slots
        const void* buf = w.fresh_buffer();
        const pr::Answer f = w.call(buf, 3, U64_FWD), i = w.call(buf, 3, U64_INV);
        REQUIRE(f.word != i.word, "forward and inverse calls of one buffer share word %d", f.word);
    }

    void out_of_domain()
    {
        World w;
        // per slot: remembered as unsure, never a family
        const void* buf = w.fresh_buffer();
        pr::Answer a = w.call(buf);
        w.finish(a, OUT);
        for (int i = 0; i < 20; i++)
        {
            a = w.call(buf);
            REQUIRE(a.state == pr::GO_LAZY && a.unsure, "out of domain, call %d: state %u unsure %d", i, a.state, a.unsure);
        }
        // through the hint
        for (int i = 0; i < 20; i++)
        {
            a = w.fresh_call(OUT);
            REQUIRE(a.state == pr::GO_LAZY && a.unsure, "out of domain through the hint, call %d: state %u", i, a.state);
        }
        // a family the slot knew stays its prediction while the buffer holds an out-of-domain stack
        buf = w.fresh_buffer();
        a = w.call(buf, 2);
        w.finish(a, W61);
        a = w.call(buf, 2);
        REQUIRE(a.state == pr::GO_LAZY_8Q && !a.unsure, "known stack");
        w.finish(a, OUT);
        a = w.call(buf, 2);
        REQUIRE(a.state == pr::GO_LAZY_8Q && a.unsure, "rewritten with an out-of-domain stack: %u %d", a.state, a.unsure);
        w.finish(a, W61);
        a = w.call(buf, 2);
        REQUIRE(a.state == pr::GO_LAZY_8Q && !a.unsure, "and back");
        // the hint keeps its family too, and an out-of-domain call does not count towards narrowing
        World v;
        v.fresh_call(W61);
        for (int i = 0; i < 40; i++)
            REQUIRE(v.fresh_call(OUT).state == pr::GO_LAZY_8Q, "call %d", i);
    }

    void lru_recycling()
    {
        World w;
        std::vector<const void*> bufs;
        std::vector<pr::Answer> first;
        for (size_t i = 0; i < pr::MAX_KEYS; i++)
        {
            bufs.push_back(w.fresh_buffer());
            first.push_back(w.call(bufs.back(), 2));
            REQUIRE(first.back().word == static_cast<int>(i), "words are handed out in order");
            w.finish(first.back(), W61);
        }
        REQUIRE(w.table.slots() == pr::MAX_KEYS, "slots %zu", w.table.slots());
        w.call(bufs[0], 2); // buffer 0 is used again: buffer 1 is the least recently used now
        // the 257th key, of ANOTHER shape, takes buffer 1's word, and the word reads unknown
        pr::Answer a = w.call(w.fresh_buffer(), 7);
        REQUIRE(a.word == first[1].word, "the 257th key took word %d, not the least recently used %d", a.word, first[1].word);
        REQUIRE(w.word(a) == pr::STATE_UNKNOWN && a.unsure && a.state == pr::GO_LAZY, "a recycled word reads unknown");
        REQUIRE(w.table.slots() == pr::MAX_KEYS, "slots %zu", w.table.slots());
        REQUIRE(w.call(bufs[0], 2).word == first[0].word && !w.call(bufs[0], 2).unsure, "buffer 0 kept its slot");
        a = w.call(bufs[1], 2); // buffer 1 lost its slot: a new one (which takes buffer 2's word), unsure again
        REQUIRE(a.unsure && a.word == first[2].word, "buffer 1 after losing its word");
        // hint learning must not read a recycled word as the old stack's
        World v;
        const pr::Answer old = v.call(v.fresh_buffer(), 3); // shape A, still in flight
        for (size_t i = 1; i < pr::MAX_KEYS; i++)
            v.finish(v.call(v.fresh_buffer(), 2), W60); // shape B fills the table
        const pr::Answer thief = v.call(v.fresh_buffer(), 2); // shape B takes shape A's word ...
        REQUIRE(thief.word == old.word, "expected the in-flight slot's word to be recycled");
        v.finish(thief, W62); // ... and its call publishes a 62-bit stack there
        a = v.call(v.fresh_buffer(), 3);
        REQUIRE(a.state == pr::GO_LAZY, "shape A read shape B's word as its own: %u", a.state);
        REQUIRE(v.call(v.fresh_buffer(), 2).state == pr::GO_LAZY_4Q, "shape B heard its own call");
    }

    void reset_predictions()
    {
        World w;
        const void* buf = w.fresh_buffer();
        w.finish(w.call(buf), W62);
        REQUIRE(w.call(buf).state == pr::GO_LAZY_4Q && w.fresh_call(W62).state == pr::GO_LAZY_4Q, "slot and hint learnt");
        w.table.reset();
        REQUIRE(w.table.slots() == 0, "slots %zu", w.table.slots());
        pr::Answer a = w.call(w.fresh_buffer());
        REQUIRE(a.state == pr::GO_LAZY && a.unsure && a.word == 0, "the hint survived a reset: %u, word %d", a.state, a.word);
        a = w.call(buf);
        REQUIRE(a.state == pr::GO_LAZY && a.unsure, "the slot survived a reset: %u", a.state);
    }

    void per_slot_rules()
    {
        World w;
        const void* buf = w.fresh_buffer();
        pr::Answer a = w.call(buf, 3);
        REQUIRE(a.state == pr::GO_LAZY && a.unsure, "first call");
        w.finish(a, W60_31);
        a = w.call(buf, 3);
        REQUIRE(a.state == pr::GO_LAZY_31Q && !a.unsure, "the first state seen is taken as it stands: %u", a.state);
        w.finish(a, W62);
        a = w.call(buf, 3);
        REQUIRE(a.state == pr::GO_LAZY_4Q && !a.unsure, "widen at once: %u", a.state);
        w.finish(a, W60);
        for (int i = 1; i <= pr::NARROW_AFTER + 2; i++)
        {
            if (i == 5)
                w.finish(a, W61); // the widest of the streak
            if (i == 6)
                w.finish(a, W60);
            a = w.call(buf, 3);
            REQUIRE(a.state == (i < pr::NARROW_AFTER ? pr::GO_LAZY_4Q : pr::GO_LAZY_8Q), "narrowing, call %d: %u", i, a.state);
        }
        // a call of the predicted family in between restarts the count
        const void* buf2 = w.fresh_buffer();
        a = w.call(buf2, 2);
        w.finish(a, W61);
        for (int i = 1; i <= 3 * pr::NARROW_AFTER; i++)
        {
            a = w.call(buf2, 2);
            REQUIRE(a.state == pr::GO_LAZY_8Q, "call %d: %u", i, a.state);
            w.finish(a, i % (pr::NARROW_AFTER - 1) == 0 ? W61 : W60);
        }
        // a word that holds no state is ignored
        w.finish(a, 77u);
        REQUIRE(w.call(buf2, 2).state == pr::GO_LAZY_8Q, "garbage in the word");
        // exact (the 4-step entry): the state seen last, as it stands, GO_GENERIC included
        const void* buf3 = w.fresh_buffer();
        a = w.call(buf3, 1, U64_4STEP, nullptr, 0, true);
        REQUIRE(a.state == pr::GO_LAZY && a.unsure, "4-step, first call");
        for (const unsigned s : {W62, W60, W61, OUT, W60_31})
        {
            w.finish(a, s);
            a = w.call(buf3, 1, U64_4STEP, nullptr, 0, true);
            REQUIRE(a.state == s && !a.unsure, "exact: saw %u, predicts %u", s, a.state);
        }
        a = w.call(w.fresh_buffer(), 1, U64_4STEP, nullptr, 0, true);
        REQUIRE(a.state == W60_31 && a.unsure, "exact through the hint: %u", a.state);
    }
} // namespace

// rns_predict_check [scenario]: every scenario, or the one named
int main(int argc, char** argv)
{
    const struct
    {
        const char* name;
        void (*run)();
    } scenarios[] = {{"fresh_buffer_per_call", fresh_buffer_per_call},
                     {"word_not_yet_written", word_not_yet_written},
                     {"a_hint_does_not_hide_a_wider_stack", a_hint_does_not_hide_a_wider_stack},
                     {"narrowing", narrowing},
                     {"alternating_stacks", alternating_stacks},
                     {"shape_isolation", shape_isolation},
                     {"out_of_domain", out_of_domain},
                     {"lru_recycling", lru_recycling},
                     {"reset_predictions", reset_predictions},
                     {"per_slot_rules", per_slot_rules}};
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
