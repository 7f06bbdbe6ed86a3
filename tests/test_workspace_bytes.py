"""The workspace-size functions return what they returned before the workspace
layouts were folded (one cursor, one layout function per call).

tests/golden/workspace_bytes.json holds, per function, [arguments, bytes]
recorded from the library built at the commit before that change: zero, one,
one below / at / above each tile, segment or alignment boundary of the
function's formula, and a large value (including the 32-bit wrap the plan
formula has always had).  A caller sizes its allocation with these functions,
so a changed value is an ABI change.

lsm_merge_kvs_workspace_bytes includes rocprim's radix-sort temporary size,
which rocprim answers from the device's tuning: with no device it gives other
numbers (2,612,992 against 2,662,144 bytes for n = 4,095).  Its values were
recorded on an MI355X and are checked in the GPU suite."""
import json
import os

import pytest

from lsmgpu import _lib

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "workspace_bytes.json")))

ANY_MACHINE = {
    "lsm_memtable_order_workspace_bytes",
    "lsm_decode_schedule_workspace_bytes",
    "lsm_wal_replay_workspace_bytes",
    "lsm_decode_sst_workspace_bytes",
    "lsm_plan_workspace_bytes",
    "lsm_build_sst_stream_workspace_bytes",
    "lsm_gather_kvs_workspace_bytes",
}


def _check(section, name):
    fn = getattr(_lib.load(), name)
    want = GOLDEN[section][name]
    assert len(want) >= 5
    assert [[args, int(fn(*args))] for args, _ in want] == want


def test_every_function_is_pinned():
    assert set(GOLDEN["any_machine"]) == ANY_MACHINE
    assert set(GOLDEN["gfx950"]) == {"lsm_merge_kvs_workspace_bytes"}


@pytest.mark.parametrize("name", sorted(ANY_MACHINE))
def test_workspace_bytes_unchanged(name):
    _check("any_machine", name)


@pytest.mark.gpu
def test_merge_workspace_bytes_unchanged(ctx):
    _check("gfx950", "lsm_merge_kvs_workspace_bytes")
