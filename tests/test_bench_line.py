"""bench.py's two kinds of line on one GPU: the plain run (headline only — set up, warm up, the timed steps, --dump-outputs, the line)
and --full (the same headline plus the sustained repeat, the parity spot check, the CPU baseline and the other configs' legs).
Both write the same --dump-outputs files for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "20000"]
MOVED = ("sustained", "cpu_baseline", "configs1", "configs3", "configs4", "mixed", "e2e", "pcie_inclusive", "host_fed")
DUMPED = ("record_index", "record_bytes", "record_byte_sums", "sample_index", "sample_record_bytes")


def _line(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "S5BENCH_ALIAS_DEVICES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def _headline(j):
    assert j["metric"] == "blow5_encode_raw_signal_throughput" and j["unit"] == "GB/s" and j["higher_is_better"] is True
    assert j["dtype"] == "int16->u8" and j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["kernel_ms"]["encode"] > 0
    assert j["config"]["reads_per_gpu"] == 20000 and 0 < j["bytes_per_sample"] < 1.2


def test_plain_line_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    plain = _line(SMALL + ["--dump-outputs", str(tmp_path / "plain")])
    _headline(plain)
    assert plain["full"] is False and plain["parity_spot_check"] is None
    assert all(plain[k] is None for k in MOVED), {k: plain[k] for k in MOVED}
    assert plain["dump_outputs"]["files"]["record_bytes"] == [20000]

    full = _line(SMALL + ["--full", "--dump-outputs", str(tmp_path / "full"), "--long-reads", "512", "--cpu-seconds", "0.3",
                          "--cpu-sweep-seconds", "0", "--get-reads", "20000", "--min-leg-seconds", "0.2", "--min-leg-steps-svb", "4",
                          "--min-leg-steps-long", "2", "--mixed-reads", "8192", "--no-e2e"])
    _headline(full)
    assert full["full"] is True and full["parity_spot_check"] is True and full["sustained"]["value"] > 0
    assert full["cpu_baseline"]["value"] > 0
    assert full["configs1"]["parity_spot_check"] is True and full["configs3"]["parity_spot_check"] is True
    assert full["configs4"]["roundtrip_identical"] is True and full["configs4"]["cpu_baseline"]["value"] > 0
    assert full["mixed"]["parity_spot_check"] is True
    assert full["e2e"] is None and full["pcie_inclusive"] is None and full["host_fed"] is None      # --no-e2e; host_fed is N > 1 only
    # the timed steps are the same in both runs: so is what they leave behind
    assert full["bytes_per_sample"] == plain["bytes_per_sample"]
    for name in DUMPED:
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype == b.dtype and np.array_equal(a, b), name
