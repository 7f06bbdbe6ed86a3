"""The C++ mirror's database scan (golsm::database::ScanFromWALs,
go-lsm_amd/host/golsm.h) run through tests/cpp/db_scan_mirror_test: range scans
over lsm_db_scan against the logs and the tree restated with std::maps, both
modes, memtable-over-memtable and memtable-over-table shadowing, tombstones, an
empty and a failed log, the memtables alone and the tree alone.  On CPU only
the host-only case runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "db_scan_mirror_test")


def _run(args, timeout):
    # built by __graft_entry__.build(); a tree built another way builds it here
    subprocess.run(["make", "-C", CPP, "-f", "db_scan.mk"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout + p.stderr


def test_mirror_scan_of_nothing_is_host_only():
    rc, out = _run(["TestScanNothing"], 60)
    assert rc == 0 and "PASS TestScanNothing" in out, out


@pytest.mark.gpu
def test_mirror_scan_all_cases_gpu():
    rc, out = _run([], 120)
    print(out)
    assert rc == 0 and "FAIL" not in out and "PASS TestScanVsMaps" in out, out
