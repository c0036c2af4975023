"""CPU tests of the single-GPU layout ladder (csrc/layout_policy.hpp).

device_bucket (capi.hip) asks the header which layout to attempt first, where
to go after a void attempt and what to remember for the next call of the
shape.  Here the header is built alone with g++ (tests/layout_host) and

* compared, over every combination of its inputs, with a restatement of the
  code it replaced: device_bucket as it stood before the header existed,
  which numbered the rungs -2 (32-bit words) to 2 (exact tuples) in a local
  `mode`, chose the start in two lambdas (first_mode, hinted_mode) and wrote
  the transitions after a void attempt in terms of `mode == -2`, `mode == -1`
  and `mode++` (old_* below: that text, statement by statement);
* walked through the case table of test_gpu_layout_matrix.py with simulated
  status words, to the layout the table (confirmed on the GPU) expects.
"""
import collections
import ctypes as C
import itertools
import os
import subprocess

import pytest

import test_gpu_layout_matrix as M
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "layout_host", "policy_host.cpp")
BAD_PAYLOAD, BAD_RANGE, BAD_PAYLOAD48, BAD_PAYLOAD32 = 1, 2, 4, 8  # kBad*
P32, P48, WORDS, SAMPLED, EXACT = range(5)                       # Rung
RUN, RESTART, STOP = range(3)                                    # Next::What
LAYOUT_NAME = {0: "tuples", 1: "words", 2: "p48", 3: "p32", 4: "p96"}  # Layout = SMJ_LAYOUT_USED_*
CAPS = ("sampled", "plan_on_host", "can_pack", "p32_usable", "p48_ok", "p48_fits", "p96_ok")
Caps = collections.namedtuple("Caps", CAPS)


class HintC(C.Structure):
    _fields_ = [("rung", C.c_int), ("calls", C.c_uint32), ("p32_fail", C.c_int)]


@pytest.fixture(scope="session")
def policy(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("layout_host") / "libpolicy_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           SRC, "-o", out])
    lib = C.CDLL(out)
    lib.lp_layout_of.argtypes = [C.c_int, C.c_int]
    lib.lp_first_rung.argtypes = [C.c_uint32, C.POINTER(HintC), C.POINTER(C.c_int)]
    lib.lp_after_void.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                  C.POINTER(HintC), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.lp_end_hint.argtypes = [C.POINTER(HintC), C.c_int, C.c_int]
    lib.lp_end_hint.restype = None
    return lib


def caps_bits(c):
    return sum(1 << i for i, v in enumerate(c) if v)


class Hint:
    """Workspace::ShapeHint as it was: mode_hint -2..2, calls, p32_fail."""

    def __init__(self, mode_hint=-2, calls=0, p32_fail=False):
        self.mode_hint, self.calls, self.p32_fail = mode_hint, calls, p32_fail

    def c(self):
        return HintC(self.mode_hint + 2, self.calls, int(self.p32_fail))

    def same(self, h):
        return (self.mode_hint + 2, self.calls, int(self.p32_fail)) == (h.rung, h.calls, h.p32_fail)


# ---------------------------------------------------------------------------
# the replaced code, restated (modes -2..2; c: the lambdas' conditions)
# ---------------------------------------------------------------------------
def old_first_mode(c, H):
    if c.p32_usable and not H.p32_fail:  # sampled && plan_on_host && ... LayP32::usable
        return -2
    if c.p48_ok and c.p48_fits:
        return -1
    return 0 if c.can_pack else (1 if c.sampled else 2)


def old_hinted_mode(m, c, H):
    """-> (mode, hinted)"""
    if not H.mode_hint <= m:
        H.calls = (H.calls + 1) & 0xFFFFFFFF
    if H.mode_hint <= m or H.calls % 16 == 0:
        return m, False
    wide = 1 if c.sampled else 2
    h = (0 if c.can_pack else wide) if H.mode_hint == 0 else wide
    return (h if h > m else m), h > m


def old_after_false(mode, c, why, guessed, H, payload_fb):
    """The loop body after bucket_sort returned false -> (what, mode,
    payload_fb); what RESTART: the caller replaces the plan and takes
    hinted_mode(first_mode()); STOP: `while (mode <= 2)` ends."""
    if mode == -2 and not (guessed and (why[1] & BAD_RANGE)):
        pay = not why[0] and not (why[1] & BAD_RANGE)
        if pay and (why[1] & (BAD_PAYLOAD | BAD_PAYLOAD48 | BAD_PAYLOAD32)):
            H.p32_fail = True
        if pay and not (why[1] & (BAD_PAYLOAD | BAD_PAYLOAD48)) and c.p48_ok:
            mode = -1
        elif pay and not (why[1] & BAD_PAYLOAD) and c.can_pack:
            mode = 0
        else:
            mode = 1
        return RUN, mode, payload_fb
    if mode == -1 and not (guessed and (why[1] & BAD_RANGE)):
        mode = 0 if ((why[1] & BAD_PAYLOAD48) and not (why[1] & BAD_PAYLOAD) and not why[0]
                     and c.can_pack) else 1
        if not why[0] and (why[1] & (BAD_PAYLOAD | BAD_PAYLOAD48)) and not (why[1] & BAD_RANGE):
            payload_fb = mode
        return RUN, mode, payload_fb
    if guessed and (why[1] & BAD_RANGE):
        return RESTART, mode, payload_fb
    if mode == 0 and not why[0] and (why[1] & BAD_PAYLOAD) and not (why[1] & BAD_RANGE):
        payload_fb = 1
    mode += 1
    return (RUN if mode <= 2 else STOP), mode, payload_fb


def old_end(H, payload_fb, started_hinted):
    if payload_fb >= 0:
        H.mode_hint = payload_fb
    elif not started_hinted:
        H.mode_hint = -2


ALL_CAPS = [Caps(*b) for b in itertools.product((False, True), repeat=len(CAPS))]


def test_layout_of(policy):
    for rung, p96 in itertools.product(range(5), (0, 1)):
        want = ("p32", "p48", "words", "p96" if p96 else "tuples", "tuples")[rung]
        assert LAYOUT_NAME[policy.lp_layout_of(rung, p96)] == want


def test_first_rung_exhaustive(policy):
    """Every caps x stored rung x p32_fail x calls % 16 (and one counter about
    to wrap): the rung, `hinted` and the hint's counter."""
    n = 0
    for c in ALL_CAPS:
        bits = caps_bits(c)
        for hint, fail, calls in itertools.product(range(-2, 3), (False, True),
                                                   list(range(16)) + [0xFFFFFFFF]):
            H = Hint(hint, calls, fail)
            want = old_hinted_mode(old_first_mode(c, H), c, H)
            h = Hint(hint, calls, fail).c()
            hinted = C.c_int(-1)
            got = policy.lp_first_rung(bits, C.byref(h), C.byref(hinted))
            assert (got - 2, bool(hinted.value)) == want, (c, hint, fail, calls)
            assert H.same(h), (c, hint, fail, calls)
            n += 1
    assert n == 128 * 5 * 2 * 17


def test_after_void_exhaustive(policy):
    """Every rung x kBad* bits x overflow x guessed x caps x p32_fail, on two
    stored hints: what comes next, the rung, the payload fallback and the
    hint (only p32_fail may change)."""
    n = 0
    for c in ALL_CAPS:
        bits = caps_bits(c)
        for mode, bad, ovf, guessed, fail, (hint, calls) in itertools.product(
                range(-2, 3), range(16), (0, 1), (False, True), (False, True),
                ((-2, 0), (1, 15))):
            for fb0 in (-2, 1):  # a fallback recorded by an earlier attempt stays
                H = Hint(hint, calls, fail)
                what, m, fb = old_after_false(mode, c, (ovf, bad), guessed, H, fb0)
                h = Hint(hint, calls, fail).c()
                pfb, nxt = C.c_int(fb0 + 2), C.c_int(-1)
                got = policy.lp_after_void(mode + 2, bits, ovf, bad, int(guessed), C.byref(h),
                                           C.byref(pfb), C.byref(nxt))
                where = (c, mode, bad, ovf, guessed, fail)
                assert got == what, where
                if what == RUN:
                    assert nxt.value - 2 == m, where
                assert pfb.value - 2 == fb, where
                assert H.same(h), where
                n += 1
    assert n > 128 * 5 * 16 * 2 * 2 * 2 * 2


def test_end_hint_exhaustive(policy):
    for hint, fb, started in itertools.product(range(-2, 3), (-2, 0, 1), (False, True)):
        H = Hint(hint, 7, True)
        old_end(H, fb, started)
        h = Hint(hint, 7, True).c()
        policy.lp_end_hint(C.byref(h), fb + 2, int(started))
        assert H.same(h), (hint, fb, started)


# ---------------------------------------------------------------------------
# the case table of test_gpu_layout_matrix.py, walked on the CPU
# ---------------------------------------------------------------------------
WORD_BITS = {P32: 32, P48: 48, WORDS: 64}


def host_caps(width, plan, flags, on_host, p48_fits):
    def u(lay):
        return bool(M.layout_usable(lay, width, plan, flags, on_host))
    sampled = not (flags & M.NO_SAMPLED) and plan.D1 <= 10
    return Caps(sampled, on_host, u("words"), u("p32"), u("p48"), p48_fits, u("p96"))


def p48_fits(plan):
    return 1 <= plan.s1 <= 32 and plan.span < 1 << (48 - plan.s1)


def status_word(case, width, rung, lay, plan, guessed):
    """why[1] of an attempt: the payload bits of the rung's words (each Pack
    flags its own and every wider word the payload does not fit) and kBadRange
    where the partition checks keys (`check` of device_bucket) and one lies
    outside the plan.  No overflow: the walk leaves those cases out."""
    bad = 0
    if rung in WORD_BITS:
        bits = case.pay_bits(width)
        if bits is None:                       # "full": the whole payload field
            bits = 32 if width == 8 else 64
        for w, flag in ((32, BAD_PAYLOAD32), (48, BAD_PAYLOAD48), (64, BAD_PAYLOAD)):
            if w >= WORD_BITS[rung] and bits > w - plan.s1:
                bad |= flag
    check = lay != "tuples" or (guessed and rung == SAMPLED)
    if check and rung != EXACT and case.key_span is not None:
        lo, hi = case.key_span[width]
        if lo < plan.base or hi > plan.base + plan.span:
            bad |= BAD_RANGE
    return bad


def walk(policy, case, width, hint):
    """One call of device_bucket for the case, the launches replaced by
    status_word: the layout it ends in.  The re-choice of level widths for
    16-byte tuples (tuple_plan) is ignored: it needs more than 192 x 8192
    tuples a bucket, which no walked case has."""
    levels = M.choose_levels(max(case.ns), case.fanout)
    sampled = not (case.flags & M.NO_SAMPLED) and levels[1] <= 10
    sample_plan = bool(case.flags & M.SAMPLE_PLAN)
    rng, guessed = case.hint, False
    if rng is None and case.kind == "sort" and sampled and not sample_plan:
        rng, guessed = (1, max(case.nR, 1)), True
    if rng is None and not sample_plan and max(case.ns) > 0:
        rng = case.key_span[width]             # key_range: one exact pass
    on_host = rng is not None
    plan = M.make_plan(*(rng or (1, 0)), levels)
    fits = p48_fits(plan)                      # once a call, from the first plan
    hinted, pfb, nxt = C.c_int(), C.c_int(P32), C.c_int()
    caps = host_caps(width, plan, case.flags, on_host, fits)
    rung = policy.lp_first_rung(caps_bits(caps), C.byref(hint), C.byref(hinted))
    started_hinted = hinted.value
    for _ in range(16):
        lay = LAYOUT_NAME[policy.lp_layout_of(rung, caps.p96_ok)]
        bad = status_word(case, width, rung, lay, plan, guessed)
        if not bad:
            break
        what = policy.lp_after_void(rung, caps_bits(caps), 0, bad, guessed, C.byref(hint),
                                    C.byref(pfb), C.byref(nxt))
        assert what != STOP
        rung = nxt.value
        if what == RESTART:
            guessed = False
            plan = M.make_plan(*case.key_span[width], levels)
            caps = host_caps(width, plan, case.flags, True, fits)
            rung = policy.lp_first_rung(caps_bits(caps), C.byref(hint), C.byref(hinted))
    else:
        raise AssertionError("the ladder does not end")
    policy.lp_end_hint(C.byref(hint), pfb.value, started_hinted)
    return lay


def walkable(case, width):
    """What a host can predict: no shard overflow ("x!", and the words of
    (16, d2_7) that overflow in the middle of the ladder), no sort of nothing."""
    e = case.expect[width]
    if e is None or "!" in e or e == "none":
        return False
    return not (width == 16 and case.name in ("A-p32-d2_7", "A-p48-d2_7", "A-words-d2_7"))


def test_case_table_walk(policy):
    """Calls 0 and 1 of every walkable (case, width) on one hint end in the
    layouts the table expects."""
    seen, two_call, n = set(), 0, 0
    for case in M.all_cases():
        for width in (8, 16):
            if not walkable(case, width):
                continue
            hint = HintC(P32, 0, 0)
            for call in range(2):
                got = walk(policy, case, width, hint)
                assert got == case.layout(width, call), (case.name, width, call, got)
                seen.add(got)
            two_call += "," in case.expect[width]
            n += 1
    assert n >= 186, n
    assert seen == {"p32", "p48", "words", "p96", "tuples"}
    assert two_call >= 2
