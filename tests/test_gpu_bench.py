"""GPU: bench.py's plain run and --dump-outputs.  A plain run prints the one
JSON line with `ms_per_step` and none of the --full legs; --dump-outputs
writes the last timed step's sorted keys and permuted values at the seeded
sample rows, which must be the oracle's sort of that step's input exactly --
here the last step of a run whose steps outnumber its input buffers, so the
refill between timed groups is what produced that input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_plain_bench_dumps_the_last_steps_output(gpu, tmp_path):
    n, steps = (1 << 20) + 4099, 3          # more rows than a dump holds: sampled
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c3",
                        "--n", str(n), "--steps", str(steps), "--warmup", "1", "--max-inputs", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Gkeys/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    # value = keys / ms_per_step (both rounded in the line: 1e-4 ms of a step of at least 0.02 ms, < 1 %)
    assert abs(line["value"] - n / line["ms_per_step"] / 1e6) <= 1e-2 * line["value"]
    assert line["timing"]["timed_groups"] == 2
    for leg in ("roofline", "cpu_baseline", "vendor", "reference_gpu"):
        assert line[leg] is None, leg
    files = sorted(os.listdir(out))
    assert files == ["keys.npy", "sample_index.npy", "values.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    keys, vals, idx = (np.load(out / f) for f in ("keys.npy", "values.npy", "sample_index.npy"))
    assert keys.dtype == vals.dtype == idx.dtype == np.float64
    assert keys.shape == vals.shape == idx.shape == (1 << 20,)
    rows = idx.astype(np.int64)
    assert rows[0] == 0 and rows[-1] == n - 1 and np.all(np.diff(rows) >= 0)
    # step r sorts draws r*n+1 .. (r+1)*n with the row index as payload
    keys_in = O.randomize_np(O.U32, O.splitmix64_stream((steps - 1) * n, n))
    ek, ev = O.lsd_sort(O.U32, keys_in, np.arange(n, dtype=np.uint32))
    assert np.array_equal(keys, ek[rows].astype(np.float64))
    assert np.array_equal(vals, ev[rows].astype(np.float64))
