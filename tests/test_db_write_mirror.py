"""The C++ mirror's write path (golsm::database::WriteBatch,
go-lsm_amd/host/golsm.h) run through tests/cpp/db_write_mirror_test:
database.Put / Delete of a batch over lsm_db_write against memtable.Manager
restated with std::maps playing the skiplists, one call and two chained calls.
On CPU only the host-only case runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "db_write_mirror_test")


def _run(args, timeout):
    # built by __graft_entry__.build(); a tree built another way builds it here
    subprocess.run(["make", "-C", CPP, "-f", "db_write.mk"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout + p.stderr


def test_mirror_write_of_no_ops_is_host_only():
    rc, out = _run(["TestWriteNothing"], 60)
    assert rc == 0 and "PASS TestWriteNothing" in out, out


@pytest.mark.gpu
def test_mirror_write_all_cases_gpu():
    rc, out = _run([], 120)
    print(out)
    assert rc == 0 and "FAIL" not in out and "PASS TestWriteVsMaps" in out, out
