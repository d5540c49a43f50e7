"""bench.py command line on real hardware: the plain run's result line and
--dump-outputs arrays, and the --full extras (tiny batch: 3 pairs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from dgraph_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 3


def run_bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--pairs", str(PAIRS), *extra],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "bench must print exactly one result line"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    steps = 3
    d = run_bench("--steps", str(steps), "--warmup", "1",
                  "--dump-outputs", str(tmp_path))
    assert d["steps"] == steps and d["unit"] == "pairs/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u64"
    assert d["cpu_baseline"] is None  # lives behind --full
    # value and ms_per_step describe the same timed region.  bench.py prints
    # ms_per_step rounded to 4 decimals and value to 2, so the two agree to
    # half a unit of ms_per_step's last place (value's own rounding moves
    # ms by < 1e-8).  A relative bound is wrong here: at this batch's
    # ~0.045 ms the rounding alone is up to 1.1e-3 relative, while at the
    # headline's 0.7 ms this absolute bound is 7e-5 relative.
    assert d["ms_per_step"] == pytest.approx(PAIRS / d["value"] * 1e3,
                                             abs=0.5e-4 + 1e-6)

    lens = np.load(tmp_path / "lens.npy")
    out = np.load(tmp_path / "out.npy")
    assert lens.dtype == np.float64 and out.dtype == np.float64
    assert lens.tolist() == [bench.OVERLAP] * PAIRS
    rng = np.random.default_rng(synth.SEED)
    _, _, common0 = synth.gen_pair(rng, bench.LIST_LEN, bench.LIST_LEN,
                                   bench.OVERLAP, bench.LIMIT)
    want = np.concatenate([synth.offset_pair(common0, common0, common0, p)[2]
                           for p in range(PAIRS)])
    assert np.array_equal(out.astype(np.uint64), want)


@pytest.mark.gpu
def test_full_run_adds_cpu_baseline():
    d = run_bench("--steps", "2", "--warmup", "0", "--full",
                  "--cpu-seconds", "0.2")
    assert d["ms_per_step"] > 0
    assert d["cpu_baseline"]["unit"] == "pairs/s"
    assert d["cpu_baseline"]["value"] > 0
