"""tools/scan_waits.py --store-waits on two hand-written assembly texts: a
prefetch drained in front of a store loop (reported) and the same kernel
with the wait relaxed to the number of loads (not reported).  Nothing is
compiled."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scanner():
    spec = importlib.util.spec_from_file_location(
        "scan_waits", os.path.join(ROOT, "tools", "scan_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HEAD = """\
\t.text
_Z9k_examplePKmPm:                      ; @_Z9k_examplePKmPm
; %bb.0:
\ts_load_dwordx4 s[0:3], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tglobal_atomic_add_x2 v[20:21], v0, v[2:3], s[2:3] sc0
\tglobal_load_dwordx4 v[4:7], v1, s[0:1]
\tv_add_u32_e32 v1, 0x4000, v1
\tglobal_load_dwordx4 v[8:11], v1, s[0:1]
\tv_add_u32_e32 v1, 0x4000, v1
\tglobal_load_dwordx4 v[12:15], v1, s[0:1]
\tv_add_u32_e32 v1, 0x4000, v1
\tglobal_load_dwordx4 v[16:19], v1, s[0:1] nt
\ts_barrier
\tds_write_b64 v30, v[22:23]
"""
TAIL = """\
\ts_barrier
.LBB0_2:                                ; =>This Inner Loop Header: Depth=1
\tds_read_b64 v[24:25], v31
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dwordx2 v32, v[24:25], s[2:3]
\ts_cbranch_execnz .LBB0_2
; %bb.3:
\ts_waitcnt vmcnt(0)
\tv_mov_b32_e32 v40, v4
\ts_endpgm
"""
# the wait for the atomic alone drains the four loads behind it
DRAINED = HEAD + "\ts_waitcnt vmcnt(0)\n" + TAIL
# at most four operations pending: the atomic has returned, the loads fly on
RELAXED = HEAD + "\ts_waitcnt vmcnt(4)\n" + TAIL


def test_drained_prefetch_is_listed():
    found = _scanner().scan_store_waits(DRAINED.splitlines())
    assert found == [("_Z9k_examplePKmPm", 16, 4, 0, "global_store_dwordx2")]


def test_relaxed_wait_is_not_listed():
    assert _scanner().scan_store_waits(RELAXED.splitlines()) == []


def test_partial_drain_and_what_does_not_count():
    sc = _scanner()
    # vmcnt(2) behind four loads still waits for two of them
    part = HEAD + "\ts_waitcnt vmcnt(2)\n" + TAIL
    assert [(k, n) for _, _, k, n, _ in sc.scan_store_waits(part.splitlines())] == [(4, 2)]
    # three loads are no prefetch run (k >= 4)
    three = DRAINED.replace("\tglobal_load_dwordx4 v[16:19], v1, s[0:1] nt\n", "")
    assert sc.scan_store_waits(three.splitlines()) == []
    # a load between the wait and the store: the wait served that load's
    # consumers, the store is not what it stands in front of
    between = DRAINED.replace(".LBB0_2:", "\tglobal_load_dword v50, v1, s[0:1]\n.LBB0_2:")
    assert sc.scan_store_waits(between.splitlines()) == []
    # the wait behind the stores (bb.3) is followed by no store: never listed
    assert all(no == 16 for _, no, _, _, _ in sc.scan_store_waits(DRAINED.splitlines()))
    # a second kernel starts from nothing
    two = DRAINED + RELAXED.replace("_Z9k_examplePKmPm", "_Z9k_relaxedPKmPm")
    assert [f for f, *_ in sc.scan_store_waits(two.splitlines())] == ["_Z9k_examplePKmPm"]
