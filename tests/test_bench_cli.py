"""bench.py's command line: a plain run does the timed steps only, --full adds
the passes of their own, --dump-outputs writes the last step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
NBLK = 3000
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", str(NBLK)]


def test_options_default_off_and_dump_configs():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True
    with pytest.raises(SystemExit):
        bench.parse(["--config", "sst", "--dump-outputs", "d"])
    with pytest.raises(SystemExit):
        bench.parse(["--e2e", "--dump-outputs", "d"])


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """Four small benchmark runs (3,000 config-2 blocks, 3 timed steps) in one
    child process of their own, so that the benchmark's allocations (and the
    cold pass's empty_cache) stay out of the test process: two plain runs that
    dump into a/ and b/, a --full run, a --full run without its two optional
    legs.  -> (the four result lines, the directory)."""
    d = tmp_path_factory.mktemp("bench")
    runs = [SMALL + ["--dump-outputs", str(d / "a")],
            SMALL + ["--dump-outputs", str(d / "b")],
            SMALL + ["--full", "--cpu-seconds", "0.2"],
            SMALL + ["--full", "--no-cpu-baseline", "--no-cold"]]
    code = "import sys, json, bench\nfor a in json.loads(sys.argv[1]):\n    bench.main(a)\n"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-c", code, json.dumps(runs)], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == len(runs), p.stdout
    return out, d


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_output(lines):
    """The plain line carries the headline fields and none of --full's; two
    runs write identical float arrays; the sampled descriptors are the closed
    form (record j of block b at 4096 b + 124 j, 16 B key, 100 B value)."""
    (j, _, _, _), d = lines
    assert all(k in j for k in HEADLINE) and j["steps"] == 3 and j["warmup"] == 1
    assert j["unit"] == "GiB/s" and j["dtype"] == "u8" and j["higher_is_better"] is True
    assert j["value"] > 0 and j["ms_per_step"] > 0
    for k in ("roofline", "cold_input", "cpu_baseline"):
        assert k not in j
    names = sorted(os.listdir(d / "a"))
    assert names == sorted(os.listdir(d / "b"))
    assert names == ["desc_key_len.npy", "desc_rec_off.npy", "desc_val_len.npy", "nrec.npy",
                     "sample_blocks.npy", "status.npy"]
    arr = {}
    for n in names:
        x, y = np.load(d / "a" / n), np.load(d / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
        arr[n[:-4]] = x
    assert sum(x.nbytes for x in arr.values()) <= 64 << 20
    assert np.array_equal(arr["nrec"], np.full(NBLK, 33, np.float32))
    assert not arr["status"].any()
    s = arr["sample_blocks"].astype(np.int64)
    assert s.size and np.array_equal(s, np.unique(s)) and s.max() < NBLK
    want = (s[:, None] * 4096 + np.arange(33)[None, :] * 124).reshape(-1)
    assert np.array_equal(arr["desc_rec_off"], want.astype(np.float64))
    assert (arr["desc_key_len"] == 16).all() and (arr["desc_val_len"] == 100).all()


@pytest.mark.gpu
def test_full_run_adds_roofline_cold_pass_and_cpu_baseline(lines):
    (_, _, j, k), _ = lines
    assert all(f in j for f in HEADLINE)
    assert j["roofline"]["kernel_ms"] > 0 and j["cold_input"]["value"] > 0
    assert j["cpu_baseline"]["value"] > 0
    assert "roofline" in k and "cold_input" not in k and "cpu_baseline" not in k
