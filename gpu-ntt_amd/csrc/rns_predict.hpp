// rns_predict.hpp -- the decision rules of host::rns_guess (prep.hip), host code with no HIP call in it: which lazy family
// will a drop-in RNS call need?  prep.hip owns the pinned, host-mapped words the preparation kernel reports to and hands them
// in as a plain array; tests/cpp/rns_predict_check.cpp plays the device and walks the rules without a GPU.
//
//   * one SLOT per (device, moduli buffer, mod_order, mod_count, word size | entry | direction), one WORD per slot.  A slot
//     predicts the family its word named last: widen at once, narrow after NARROW_AFTER calls in a row that needed less
//     (`exact`, the 4-step entry: the state seen last, as it stands).
//   * a slot whose word has named nothing yet is UNSURE; so is one whose last finished call found a modulus outside the lazy
//     families' domain (GO_GENERIC), which is remembered as that and never becomes a family.
//   * MAX_KEYS words per device; when they are all taken the least recently used slot gives up its word.
//   * the SHAPE HINT: what stacks of the same shape (device, mod_count, word size | entry | direction, ordered or not)
//     needed, whatever buffer they lived in.  It learns from every word of its shape that names a family: the slot's own
//     word on a repeated call, and -- when a slot is created for a buffer never seen before -- the words of the last
//     HINT_RECENT slots created for that shape (a bounded look, nothing waits: a word its call has not written yet is
//     looked at again next time).  The hint follows the same widen-at-once / narrow-after-16 rule and is the first
//     prediction of a new slot, which stays unsure until its own word has spoken.
#ifndef GPUNTT_RNS_PREDICT_HPP
#define GPUNTT_RNS_PREDICT_HPP

#include <array>
#include <cstddef>
#include <map>
#include <tuple>

namespace gpuntt
{
    namespace host
    {
        namespace predict
        {
            // the go-flag states of merge_lazy_kernels.hpp (kern::GO_*; prep.hip asserts that they are the same numbers)
            constexpr unsigned GO_GENERIC = 0u, GO_LAZY = 1u, GO_LAZY_8Q = 2u, GO_LAZY_4Q = 3u, GO_LAZY_31Q = 4u;
            constexpr unsigned STATE_UNKNOWN = 0xffffffffu;
            constexpr std::size_t MAX_KEYS = 256; // words (= slots) per device
            constexpr std::size_t STRIDE = 16;    // words are one cache line apart
            constexpr int NARROW_AFTER = 16;
            constexpr int HINT_RECENT = 4;

            // generality of a lazy family (kern::family_rank): a family serves every stack a narrower one serves
            constexpr int family_rank(unsigned state)
            {
                return state == GO_LAZY_31Q ? 0 : (state == GO_LAZY ? 1 : (state == GO_LAZY_8Q ? 2 : (state == GO_LAZY_4Q ? 3 : -1)));
            }

            struct Family
            {
                unsigned predicted = GO_LAZY;
                bool have = false;              // some finished call has named a state
                int streak = 0;                 // observations in a row that needed a narrower family than the predicted one
                unsigned streak_state = GO_LAZY; // the widest of them
                // the enqueued family serves every narrower stack too, so: widen at once, narrow after NARROW_AFTER
                // observations in a row that needed less
                void observe(unsigned seen, bool exact)
                {
                    const int r_seen = family_rank(seen), r_now = family_rank(predicted);
                    if (!have || r_seen > r_now || exact)
                    {
                        predicted = seen;
                        streak = 0;
                    }
                    else if (r_seen == r_now)
                        streak = 0;
                    else
                    {
                        if (streak == 0 || r_seen > family_rank(streak_state))
                            streak_state = seen;
                        if (++streak >= NARROW_AFTER)
                        {
                            predicted = streak_state;
                            streak = 0;
                        }
                    }
                    have = true;
                }
            };

            struct Answer
            {
                unsigned state = GO_LAZY; // the family to enqueue
                bool unsure = true;
                int word = -1; // index of the slot's word: the preparation kernel writes words[word * STRIDE]
            };

            class Table
            {
              public:
                // (device, moduli, mod_order, mod_count, word size | 4-step entry | direction): forward and inverse calls of
                // one stack may need different families (31 q serves forward transforms only), a *_Modulus_Ordered call uses
                // the subset its order array names; the Merge entry points otherwise share one slot per stack
                using Key = std::tuple<int, const void*, const void*, int, int>;
                using Shape = std::tuple<int, int, int, bool>;

                // forgets every slot and hint (the words stay where they are: graphs captured earlier keep writing to theirs)
                void reset()
                {
                    slots_.clear();
                    hints_.clear();
                    devs_.clear();
                    clock_ = 0;
                }

                // words: the pool of device `dev`, MAX_KEYS words STRIDE apart, written by the device at any time and read
                // here as they stand (an older value is as good).  Never waits.
                Answer guess(volatile unsigned* words, int dev, const void* moduli, const void* order, int mod_count,
                             int word_dir, bool exact)
                {
                    const Key key = std::make_tuple(dev, moduli, order, mod_count, word_dir);
                    Hint& hint = hints_[std::make_tuple(dev, mod_count, word_dir, order != nullptr)];
                    Device& d = devs_[dev];
                    auto it = slots_.find(key);
                    if (it == slots_.end())
                    {
                        learn(hint, d, words, exact);
                        Slot slot;
                        std::size_t on_dev = 0;
                        auto oldest = slots_.end();
                        for (auto jt = slots_.begin(); jt != slots_.end(); ++jt)
                            if (std::get<0>(jt->first) == dev)
                            {
                                on_dev++;
                                if (oldest == slots_.end() || jt->second.last_use < oldest->second.last_use)
                                    oldest = jt;
                            }
                        if (on_dev < MAX_KEYS)
                            slot.word = static_cast<int>(on_dev); // words are handed out in order and only recycled below
                        else
                        {
                            slot.word = oldest->second.word; // table full: the least recently used stack gives up its word
                            slots_.erase(oldest);
                        }
                        words[slot.word * STRIDE] = STATE_UNKNOWN;
                        d.generation[slot.word]++; // whoever remembers the word under its old generation must not read it
                        d.spoken[slot.word] = false;
                        if (hint.family.have)
                            slot.family.predicted = hint.family.predicted; // (have stays false: unsure until its own word speaks)
                        slot.generic_seen = hint.generic_seen;
                        hint.recent[hint.next] = Recent{slot.word, d.generation[slot.word]};
                        hint.next = (hint.next + 1) % HINT_RECENT;
                        it = slots_.emplace(key, slot).first;
                    }
                    Slot& s = it->second;
                    s.last_use = ++clock_;
                    const unsigned seen = words[s.word * STRIDE];
                    if (seen != STATE_UNKNOWN && seen <= GO_LAZY_31Q && (exact || seen != GO_GENERIC))
                    {
                        // the state some earlier call of this stack found (the last one that has finished)
                        s.family.observe(seen, exact);
                        s.generic_seen = false;
                        d.spoken[s.word] = true; // the hint hears it here, not a second time through `recent`
                        teach(hint, seen, exact);
                    }
                    else if (seen == GO_GENERIC)
                    {
                        s.generic_seen = true;
                        hint.generic_seen = true;
                    }
                    Answer a;
                    a.state = s.family.predicted;
                    a.unsure = !s.family.have || s.generic_seen;
                    a.word = s.word;
                    return a;
                }

                std::size_t slots() const { return slots_.size(); }

              private:
                struct Slot
                {
                    int word = -1; // index of the slot's word in its device's pool of host-mapped words
                    Family family;
                    unsigned long long last_use = 0;
                    bool generic_seen = false; // the last finished call found a modulus outside the lazy families' domain
                };
                struct Recent
                {
                    int word = -1;
                    unsigned generation = 0;
                };
                struct Hint
                {
                    Family family;
                    bool generic_seen = false;
                    std::array<Recent, HINT_RECENT> recent{}; // the slots created last for this shape, oldest at `next`
                    int next = 0;
                };
                struct Device
                {
                    std::array<unsigned, MAX_KEYS> generation{}; // bumped whenever the word goes to a new slot
                    std::array<bool, MAX_KEYS> spoken{};         // the slot of the word has read a state from it itself
                };

                static void teach(Hint& hint, unsigned seen, bool exact)
                {
                    if (seen == GO_GENERIC) // out of domain: remembered as unsure, never as a family
                    {
                        hint.generic_seen = true;
                        return;
                    }
                    hint.family.observe(seen, exact);
                    hint.generic_seen = false;
                }
                // the words of the last HINT_RECENT slots created for this shape, oldest first: each finished call is heard
                // once; a word that was recycled meanwhile belongs to another stack and is not read
                static void learn(Hint& hint, Device& d, volatile unsigned* words, bool exact)
                {
                    for (int i = 0; i < HINT_RECENT; i++)
                    {
                        Recent& r = hint.recent[(hint.next + i) % HINT_RECENT];
                        if (r.word < 0)
                            continue;
                        if (d.generation[r.word] != r.generation || d.spoken[r.word])
                        {
                            r.word = -1;
                            continue;
                        }
                        const unsigned seen = words[r.word * STRIDE];
                        if (seen == STATE_UNKNOWN)
                            continue; // its call has not finished: look again when the next slot is created
                        r.word = -1;
                        if (seen <= GO_LAZY_31Q)
                            teach(hint, seen, exact);
                    }
                }

                std::map<Key, Slot> slots_;
                std::map<Shape, Hint> hints_;
                std::map<int, Device> devs_;
                unsigned long long clock_ = 0;
            };
        } // namespace predict
    } // namespace host
} // namespace gpuntt
#endif
