"""The C++ mirror's range scan (golsm::sstable::ScanImages,
go-lsm_amd/host/golsm.h) run through tests/cpp/tree_scan_mirror_test: range
scans over lsm_tree_scan against the tree restated with std::maps, both modes,
level-0 shadowing, tombstones and boundary keys.  On CPU only the host-only
case runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "tree_scan_mirror_test")


def _run(args, timeout):
    # built by __graft_entry__.build(); a tree built another way builds it here
    subprocess.run(["make", "-C", CPP, "-f", "tree_scan.mk"], check=True, stdout=subprocess.DEVNULL)
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
