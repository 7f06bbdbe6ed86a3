"""The C++ mirror's memtable search (golsm::memtables::SearchWALs,
go-lsm_amd/host/golsm.h) run through tests/cpp/memtable_search_mirror_test:
Manager.Search over the memtables recovered from their WALs, against std::maps
playing the skiplists, and its database.Get (golsm::database::GetFromWALs over
lsm_db_get) against those maps plus a lookup in the tables' pairs, in both
modes.  On CPU only the host-only cases run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "memtable_search_mirror_test")


def _run(args, timeout):
    # built by __graft_entry__.build(); a tree built another way builds it here
    subprocess.run(["make", "-C", CPP, "-f", "memtable_search.mk"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout + p.stderr


def test_mirror_search_of_no_logs_and_no_keys_is_host_only():
    rc, out = _run(["TestSearchNothing"], 60)
    assert rc == 0 and "PASS TestSearchNothing" in out, out


def test_mirror_get_of_no_keys_or_no_logs_and_no_tables_is_host_only():
    rc, out = _run(["TestGetNothing"], 60)
    assert rc == 0 and "PASS TestGetNothing" in out, out


@pytest.mark.gpu
def test_mirror_search_all_cases_gpu():
    rc, out = _run([], 120)
    print(out)
    assert rc == 0 and "FAIL" not in out and "PASS TestSearchVsMaps" in out, out
    assert "PASS TestGetVsMaps" in out, out
