"""The C++ mirror's packed database scan (golsm::database::ScanFromWALsPacked,
go-lsm_amd/host/golsm.h) run through tests/cpp/pack_mirror_test: the entries
read out of lsm_pack_results's two arenas against ScanFromWALs's, which slices
the host's logs and images, entry for entry on db_scan_mirror_test's
databases, both modes.  On CPU only the host-only case runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "pack_mirror_test")


def _run(args, timeout):
    # built by __graft_entry__.build(); a tree built another way builds it here
    subprocess.run(["make", "-C", CPP, "-f", "pack.mk"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout + p.stderr


def test_mirror_packed_scan_of_nothing_is_host_only():
    rc, out = _run(["TestPackedNothing"], 60)
    assert rc == 0 and "PASS TestPackedNothing" in out, out


@pytest.mark.gpu
def test_mirror_packed_scan_equals_sliced_scan_gpu():
    rc, out = _run([], 120)
    print(out)
    assert rc == 0 and "FAIL" not in out and "PASS TestPackedVsSliced" in out, out
