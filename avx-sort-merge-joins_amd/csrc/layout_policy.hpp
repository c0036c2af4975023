#pragma once
// layout_policy.hpp -- which intermediate layout a sort or join attempts, and
// where it goes after a void attempt.  Plain host C++ (no HIP headers): the
// launches live in device_bucket (capi.hip), the decisions here, driven on
// the CPU by tests/test_layout_policy.py through tests/layout_host.
//
// An attempt partitions the relations into one layout and runs the tile and
// group passes on it.  It is void when a region of the sampled partition
// overflowed (status word 0) or a tuple did not fit the layout (status word 1,
// kBad*); the call then goes on to a wider rung.  A guessed plan (keys 1..n)
// that a key falls outside of is replaced and the ladder restarts.
#include <stdint.h>

namespace smj {

// bits of a partition's "bad tuple" flag (status word 1 of a join)
constexpr uint32_t kBadPayload = 1;  // a payload does not fit a packed word
constexpr uint32_t kBadRange = 2;    // a key lies outside the plan range
constexpr uint32_t kBadPayload48 = 4;  // ... fits a 64-bit word, not a 48-bit one
constexpr uint32_t kBadPayload32 = 8;  // ... fits a 48-bit word, not a 32-bit one

// The rungs of the ladder, narrowest first ("narrower than" is <): sampled
// partitions into 32-bit words, 48-bit words in two planes, 64-bit words,
// then whatever holds any payload (Sampled), then the exact partition of
// tuples (no sample, no overflow).
enum class Rung : int { P32, P48, Words, Sampled, Exact };

// What the partition buffers hold (LayTup, LayPacked, LayP48, LayP32, LayP96),
// numbered as SMJ_LAYOUT_USED_* of smj.h (capi.hip asserts it).
enum class Layout : int { Tuples = 0, Words = 1, P48 = 2, P32 = 3, P96 = 4 };

// Sampled: 12-byte elements where the plan allows them, else tuples
inline Layout layout_of(Rung r, bool p96_ok) {
    return r == Rung::P32 ? Layout::P32 : r == Rung::P48 ? Layout::P48
         : r == Rung::Words ? Layout::Words
         : r == Rung::Sampled && p96_ok ? Layout::P96 : Layout::Tuples;
}

// What the plan and the workspace's layout policy allow (device_bucket fills
// it from the host plan, smj_workspace_set_layouts and the partition count).
struct LayoutCaps {
    bool sampled;       // the sampled partition applies (up to 1024 partitions)
    bool plan_on_host;  // the host knows the plan: words can be packed
    bool can_pack;      // 64-bit words (16-byte tuples)
    bool p32_usable;    // 32-bit words, whatever their payloads
    bool p48_ok;        // 48-bit words, whatever their payloads
    // payloads within the key span fit a 48-bit word: from the first plan of
    // the call, kept when a guessed plan is replaced
    bool p48_fits;
    bool p96_ok;        // Sampled means 12-byte elements
};

// What the last sorts and joins of one shape (relation sizes) learnt about
// their payloads:
//   rung: the rung the last call reached after leaving the narrower ones for
//     its payloads (P32: none), with a re-probe from the top every 16th call
//     (calls);
//   p32_fail: its payloads did not fit 32-bit words, so its calls start at
//     the wider layouts (no re-probe: the 32-bit words are for relations with
//     tiny payloads, e.g. the sort's).
struct ShapeHint {
    uint64_t shape = ~0ull;
    Rung rung = Rung::P32;
    uint32_t calls = 0;
    bool p32_fail = false;
    uint64_t used = 0;  // LRU clock
};

// The rung the plan itself starts at.  32-bit words are tried first: nothing
// tells the payloads' width beforehand.  48-bit words only where row-id
// payloads would fit (p48_fits): a 48-bit attempt that fails on them
// partitions a second time.
inline Rung plan_rung(const LayoutCaps& c, const ShapeHint& h) {
    if (c.p32_usable && !h.p32_fail) return Rung::P32;
    if (c.p48_ok && c.p48_fits) return Rung::P48;
    return c.can_pack ? Rung::Words : (c.sampled ? Rung::Sampled : Rung::Exact);
}

// The rung an attempt sequence starts at: plan_rung, or past it the rung the
// shape's last call was sent to by its payloads -- its partition would only
// be repeated.  *hinted: the hint moved the start.  Data-dependent like the
// fallback it skips; the results are the same in every layout.
inline Rung first_rung(const LayoutCaps& c, ShapeHint& h, bool* hinted) {
    const Rung m = plan_rung(c, h);
    *hinted = false;
    // (the call counter advances only where the hint lies above the plan's rung)
    if (h.rung <= m || ++h.calls % 16 == 0) return m;
    const Rung wide = c.sampled ? Rung::Sampled : Rung::Exact;
    const Rung r = h.rung == Rung::Words && c.can_pack ? Rung::Words : wide;
    *hinted = r > m;
    return r > m ? r : m;
}

// After a void attempt at `rung` (why[0]: region overflow, why[1]: kBad*).
struct Next {
    enum What { Run, Restart, Stop } what;
    Rung rung;  // Run: the rung to attempt next
};
// Restart: `guessed` and a key outside the plan -- the caller replaces the
// plan by the exact one, fills the caps again and calls first_rung.
// *payload_fb: the rung a payload-only failure (no overflow, no kBadRange) of
// the 48- or 64-bit words sent this call to; end_hint stores it.
inline Next after_void(Rung rung, const LayoutCaps& c, const uint32_t why[2], bool guessed,
                       ShapeHint& h, Rung* payload_fb) {
    const uint32_t bad = why[1];
    const bool pay = !why[0] && !(bad & kBadRange);  // nothing but payloads, if anything
    const bool restart = guessed && (bad & kBadRange);
    if (rung == Rung::P32 && !restart) {
        // payloads too wide for 32 bits: the narrowest wider words that hold
        // them; anything else (overflow, a key outside the plan) as from
        // 64-bit words
        if (pay && (bad & (kBadPayload | kBadPayload48 | kBadPayload32))) h.p32_fail = true;
        if (pay && !(bad & (kBadPayload | kBadPayload48)) && c.p48_ok)
            return {Next::Run, Rung::P48};
        if (pay && !(bad & kBadPayload) && c.can_pack) return {Next::Run, Rung::Words};
        return {Next::Run, Rung::Sampled};
    }
    if (rung == Rung::P48 && !restart) {
        // payloads too wide for 48 bits only: 64-bit words; anything else
        // (overflow, unpackable) as from 64-bit words
        const Rung to = (bad & kBadPayload48) && !(bad & kBadPayload) && !why[0] && c.can_pack
            ? Rung::Words : Rung::Sampled;
        if (pay && (bad & (kBadPayload | kBadPayload48))) *payload_fb = to;
        return {Next::Run, to};
    }
    if (restart) return {Next::Restart, rung};
    if (rung == Rung::Words && pay && (bad & kBadPayload)) *payload_fb = Rung::Sampled;
    // (the exact partition has no overflow and no flags: its attempt is never void)
    if (rung == Rung::Exact) return {Next::Stop, rung};
    return {Next::Run, (Rung)((int)rung + 1)};
}

// The call's end.  payload_fb: P32 = no payload fallback in this call;
// started_hinted: first_rung's *hinted of the call's first choice.
inline void end_hint(ShapeHint& h, Rung payload_fb, bool started_hinted) {
    if (payload_fb >= Rung::Words)
        h.rung = payload_fb;
    else if (!started_hinted)
        h.rung = Rung::P32;  // the narrow layouts held (or failed for other reasons)
}

}  // namespace smj
