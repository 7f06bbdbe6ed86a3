"""The WAL replay's case list (tests/wal_cases.py) on the CPU: the census, a
restatement of wal.hip's decisions in Python integers, must reproduce the
oracle's serial chase in every case, keep every modelled load and store
inside the device's buffers, and reach the paths the case list claims, each
exactly as often as COVERAGE says, so that editing a case cannot silently
lose a path.  The mutant table is checked the same way: the model predicts
which cases each value-only change to wal.hip turns red.
"""
import functools

import numpy as np
import pytest

import wal_cases as wc

NAMES = [c.name for c in wc.CASES]


@functools.lru_cache(maxsize=None)
def census_of(name):
    return wc.census(wc.BY_NAME[name])


@pytest.mark.parametrize("name", NAMES)
def test_census_equals_the_oracle(name):
    case = wc.BY_NAME[name]
    c = census_of(name)                      # raises Unsafe on any modelled access out of bounds
    st, d = wc.expected(case, case.cap)
    assert (c.status, c.nrec) == (st, len(d))
    assert np.array_equal(c.descriptors(), d)
    full_st, full = wc.expected(case)
    if case.cap is not None and len(full) > case.cap:
        # the capacity contract (include/lsm_gpu.h): more records than slots
        # is LSM_ST_CAPACITY whatever follows them in the log
        assert st == wc.ST_CAPACITY and len(d) == case.cap and np.array_equal(d, full[:case.cap])
    else:
        assert st == full_st and len(d) == len(full)


@pytest.mark.parametrize("h", [0, 1, 15])
def test_census_at_every_start_misalignment(h):
    """The start's misalignment moves the LDS copy's window, never the result."""
    for case in wc.CASES:
        if len(case.log) > wc.MAX_LOG:
            continue
        assert wc.verdict(case, wc.census(case, h=h)), case.name


def test_sizes():
    for c in wc.CASES:
        nseg = -(-len(c.log) // wc.kWalSeg)
        if c.name.startswith("group1"):
            assert 66 <= nseg <= 68, (c.name, nseg)
        elif c.name == "escaped-keys":
            assert max(int(x) for x in wc.expected(c)[1]["key_len"]) >= 1 << 18
        else:
            assert len(c.log) <= wc.MAX_LOG, c.name


# (case, tag, how often the case reaches it)
COVERAGE = [
    # the segment's guess and its two phases
    ("pass-through-shares-serial", "guess:found", 1),
    ("tail-1025", "guess:found", 1),
    ("tail-1", "guess:none", 1),
    ("tail-7", "guess:none", 1),
    ("tail-1", "guess:g+4>len", 1),
    ("cap-full", "guess:g+4>len", 1),
    ("short-in-long-grid", "phase1:dead", 1),
    ("error-after-long-record", "phase1:dead", 1),
    ("tail-1", "phase1:pass-through", 1),
    ("tail-7", "phase1:pass-through", 1),
    ("pass-through-shares-serial", "phase1:live", 1),
    ("tail-1025", "phase1:live", 1),
    ("last-segment-inside-a-value", "log:fast:pass-through-chosen", 1),
    ("zeros-phase1", "log:fast:pass-through-chosen", 1),
    # share widths
    ("tail-1", "width:full:W=272:last=60", 1),
    ("tail-7", "width:full:W=272:last=60", 1),
    ("tail-1", "width:tail=1:W=16:last=0", 1),
    ("tail-7", "width:tail=7:W=16:last=0", 1),
    ("tail-8", "width:tail=8:W=16:last=0", 1),
    ("tail-63", "width:tail=63:W=16:last=3", 1),
    ("tail-64", "width:tail=64:W=16:last=3", 1),
    ("tail-65", "width:tail=65:W=16:last=4", 1),
    ("tail-1025", "width:tail=1025:W=48:last=21", 1),
    ("exact-multiple", "log:len%16384==0", 1),
    ("zeros", "log:len%16384==0", 1),
    # share guesses
    ("short-in-long-grid", "share:guess:none", 3),
    ("error-after-long-record", "share:guess:none", 38),
    ("short-in-long-grid", "share:guess:e1-pass-through", 2),
    ("error-after-long-record", "share:guess:e1-pass-through", 2),
    ("pass-through-shares", "share:fast:pass-through-chosen", 30),
    ("edge-h1", "share:fast:pass-through-chosen", 1),
    ("pass-through-shares", "share:fast:pass-through-handed-on", 30),
    ("error-after-long-record", "share:guess:at-ss", 1),
    ("tail-1", "share:guess:at-ss", 5),
    ("error-after-long-record", "share:guess:at-se-1", 1),
    ("pass-through-shares-serial", "share:guess:at-se-1", 1),
    ("share-edges", "share:guess:at-se-1", 1),
    # share stitch
    ("tail-1", "share:fast", 2),
    ("tail-7", "share:fast", 2),
    ("tail-1", "share:fast:chain0", 29),
    ("tail-7", "share:fast:chain0", 29),
    ("tail-1", "share:fast:chain1", 31),
    ("tail-7", "share:fast:chain1", 31),
    ("tail-1", "share:fast:k=0", 2),
    ("tail-7", "share:fast:k=0", 2),
    ("edge-h15", "share:fast:k>0", 2),
    ("edge-h15-one-past", "share:fast:k>0", 2),
    ("tail-1", "share:fast:k==last", 1),
    ("tail-7", "share:fast:k==last", 1),
    ("tail-1", "share:fast:error-in-entry-share", 1),
    ("tail-7", "share:fast:error-in-entry-share", 1),
    ("tail-1", "share:fast:error-in-later-share", 1),
    ("tail-7", "share:fast:error-in-later-share", 1),
    ("short-in-long-grid", "share:serial", 1),
    ("error-after-long-record", "share:serial", 1),
    ("short-in-long-grid", "share:serial:entry-share", 1),
    ("error-after-long-record", "share:serial:entry-share", 1),
    ("short-in-long-grid", "share:serial:reuse-chain0", 1),
    ("error-after-long-record", "share:serial:reuse-chain0", 6),
    ("short-in-long-grid", "share:serial:reuse-chain1", 1),
    ("pass-through-shares-serial", "share:serial:reuse-chain1", 8),
    ("short-in-long-grid", "share:serial:re-chase", 1),
    ("error-after-long-record", "share:serial:re-chase", 2),
    ("short-in-long-grid", "share:serial:error", 1),
    ("error-after-long-record", "share:serial:error", 1),
    ("short-in-long-grid", "share:record-longer-than-a-share", 3),
    ("error-after-long-record", "share:record-longer-than-a-share", 8),
    ("ff-value", "share:record-longer-than-a-segment", 1),
    ("serial-phase1", "share:record-longer-than-a-segment", 2),
    ("big-keys", "share:key>1024", 23),
    ("edge-h15", "share:key>1024", 1),
    # reads: the LDS copy and the buffer resource, at each start misalignment
    ("short-in-long-grid", "read:lds:s=0", 34),
    ("tail-7", "read:lds:s>0", 2),
    ("tail-8", "read:lds:s>0", 2),
    ("big-keys", "read:buffer:s=0", 4),
    ("ff-value", "read:buffer:s=0", 3),
    ("edge-h15", "read:buffer:s>0", 5),
    ("edge-h15-one-past", "read:buffer:s>0", 8),
    ("big-keys", "read:buffer:wholly-past:s=0", 4),
    ("edge-h0", "read:buffer:wholly-past:s>0", 6),
    ("edge-h1", "read:buffer:wholly-past:s>0", 4),
    ("edge-h15", "read:buffer:wholly-past:s>0", 5),
    ("edge-h0", "read:lds:o+8==s0+sz:s>0", 3),
    ("edge-h1", "read:lds:o+8==s0+sz:s>0", 3),
    ("edge-h15", "read:lds:o+8==s0+sz:s>0", 3),
    ("edge-h0-one-past", "read:buffer:o+8==s0+sz+1:s>0", 3),
    ("edge-h1-one-past", "read:buffer:o+8==s0+sz+1:s>0", 3),
    ("edge-h15-one-past", "read:buffer:o+8==s0+sz+1:s>0", 3),
    # log stitch
    ("short-in-long-grid", "log:fast", 1),
    ("short-in-long-grid", "log:fast:phase0", 1),
    ("pass-through-shares-serial", "log:fast:phase1", 1),
    ("tail-1025", "log:fast:phase1", 1),
    ("short-in-long-grid", "log:fast:error", 1),
    ("error-after-long-record", "log:fast:error", 1),
    ("tail-63", "log:serial", 1),
    ("tail-64", "log:serial", 1),
    ("tail-63", "log:serial:phase0", 1),
    ("tail-64", "log:serial:phase0", 1),
    ("big-keys", "log:serial:phase1", 1),
    ("serial-phase1", "log:serial:phase1", 2),
    ("tail-63", "log:serial:phase2", 1),
    ("tail-64", "log:serial:phase2", 1),
    ("ff-value", "log:serial:skipped-segment", 1),
    ("serial-phase1", "log:serial:skipped-segment", 1),
    ("tail-63", "log:serial:error", 1),
    ("tail-64", "log:serial:error", 1),
    ("group1-clean", "log:group1:after-clean", 1),
    ("group1-after-miss", "log:group1:after-miss", 1),
    ("group1-after-error", "log:group1:after-error", 1),
    ("empty", "log:empty", 1),
    ("over-max-len", "log:len>max_len", 1),
    ("cap-over-max-len", "log:len>max_len", 1),
    ("empty", "log:segs>nseg", 1),
    ("short-in-long-grid", "log:segs>nseg", 1),
    # compact
    ("short-in-long-grid", "compact:packed", 1),
    ("error-after-long-record", "compact:packed", 1),
    ("tail-63", "compact:full", 1),
    ("tail-64", "compact:full", 1),
    ("tail-63", "compact:last-vl-from-exit-past-segment", 1),
    ("tail-64", "compact:last-vl-from-exit-past-segment", 1),
    ("error-after-miss", "compact:2048-records", 1),
    ("zeros", "compact:2048-records", 3),
    ("escaped-keys", "compact:escaped-key-length", 2),
    ("cap-packed", "capacity:gridded", 1),
    ("cap-short-and-error", "capacity:gridded", 1),
    ("cap-over-max-len", "capacity:len>max_len", 1),
    ("cap-packed", "compact:packed:capacity-guard", 1),
    ("cap-short-and-error", "compact:packed:capacity-guard", 1),
    ("cap-full", "compact:full:capacity-guard", 1),
]

# Two paths wal.hip writes out cannot be reached by any log, and the census
# says why: a share's first guess e0 is plausible, so e0 + 8 + u32(e0) <= len
# and its second guess e1 = e0 + 4 + u32(e0) always exists; and the serial
# share stitch skips a share once the chain is at or past its end, so it never
# consults a pass-through chain (a guess at or past the share's end).
UNREACHED = ["share:guess:e1-absent", "share:serial:pass-through-chosen"]


@pytest.mark.parametrize("name,tag,count", COVERAGE)
def test_coverage(name, tag, count):
    assert census_of(name).tags[tag] == count


def test_unreached_paths():
    for name in NAMES:
        for tag in UNREACHED:
            assert census_of(name).tags[tag] == 0, (name, tag)


@pytest.mark.parametrize("mutant", list(wc.MUTANTS))
def test_mutants(mutant):
    red, unsafe = [], []
    for case in wc.CASES:
        try:
            if not wc.verdict(case, wc.census(case, mutant=mutant)):
                red.append(case.name)
        except wc.Unsafe:
            unsafe.append(case.name)
    assert unsafe == wc.MUTANT_NOT_CLEARED.get(mutant, [])
    if not unsafe:
        assert sorted(red) == sorted(wc.MUTANT_RED[mutant])
