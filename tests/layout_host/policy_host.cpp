// C entry points over csrc/layout_policy.hpp for tests/test_layout_policy.py.
// Rungs and layouts cross as the enums' integers, the caps as bits
// (kCaps order below), the hint as three plain fields.
#include "../../avx-sort-merge-joins_amd/csrc/layout_policy.hpp"

using namespace smj;

struct HintC {
    int rung;
    uint32_t calls;
    int p32_fail;
};

static LayoutCaps caps_of(uint32_t b) {
    LayoutCaps c;
    c.sampled = b & 1;
    c.plan_on_host = b & 2;
    c.can_pack = b & 4;
    c.p32_usable = b & 8;
    c.p48_ok = b & 16;
    c.p48_fits = b & 32;
    c.p96_ok = b & 64;
    return c;
}

static ShapeHint hint_in(const HintC* h) {
    ShapeHint s;
    s.rung = (Rung)h->rung;
    s.calls = h->calls;
    s.p32_fail = h->p32_fail != 0;
    return s;
}

static void hint_out(const ShapeHint& s, HintC* h) {
    h->rung = (int)s.rung;
    h->calls = s.calls;
    h->p32_fail = s.p32_fail;
}

extern "C" {

int lp_layout_of(int rung, int p96_ok) { return (int)layout_of((Rung)rung, p96_ok != 0); }

int lp_first_rung(uint32_t caps, HintC* h, int* hinted) {
    ShapeHint s = hint_in(h);
    bool hi = false;
    const Rung r = first_rung(caps_of(caps), s, &hi);
    hint_out(s, h);
    *hinted = hi;
    return (int)r;
}

// returns Next::what (0 run, 1 restart, 2 stop); *next_rung for a run
int lp_after_void(int rung, uint32_t caps, uint32_t why0, uint32_t why1, int guessed, HintC* h,
                  int* payload_fb, int* next_rung) {
    ShapeHint s = hint_in(h);
    const uint32_t why[2] = {why0, why1};
    Rung fb = (Rung)*payload_fb;
    const Next n = after_void((Rung)rung, caps_of(caps), why, guessed != 0, s, &fb);
    hint_out(s, h);
    *payload_fb = (int)fb;
    *next_rung = (int)n.rung;
    return (int)n.what;
}

void lp_end_hint(HintC* h, int payload_fb, int started_hinted) {
    ShapeHint s = hint_in(h);
    end_hint(s, (Rung)payload_fb, started_hinted != 0);
    hint_out(s, h);
}

}  // extern "C"
