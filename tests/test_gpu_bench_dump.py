"""bench.py on the GPU, a plain run at a small workload: --steps sets the timed steps, the
line carries ms_per_step and none of --full's legs, and --dump-outputs writes the last
timed step's aggregate — the same bytes from run to run, and the bytes a direct call of
the timed path gives on the same seeded records."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FULL_ONLY = {"cpu_baseline", "e2e_host_inclusive", "configs", "metric_literal_config",
             "reference_speedup", "exp5", "next_rows", "oram_tree", "detail"}


def _run(capsys, out_dir, steps, warmup):
    import bench
    bench.main(["--gpus", "1", "--workload", "mnist30", "--steps", str(steps), "--warmup",
                str(warmup), "--dump-outputs", str(out_dir)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return line, np.load(os.path.join(out_dir, "aggregate.npy"))


def test_plain_run_dumps_the_last_step(tmp_path, capsys):
    import torch

    import bench
    import bench_legs
    from fltee import device as D
    steps, warmup = 3, 2
    line, a = _run(capsys, tmp_path / "a", steps, warmup)
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "client-params/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32"
    assert not FULL_ONLY & set(line)
    w = bench_legs.WORKLOADS["mnist30"]
    n, d = w["n"], w["d"]
    assert a.dtype == np.float32 and a.shape == (d,) and a.nbytes <= bench.DUMP_MAX_BYTES
    assert os.listdir(tmp_path / "a") == ["aggregate.npy"]
    # the last timed step read input buffer (warmup + steps - 1) % 3, seeded 17 + that
    dev = torch.device("cuda", 0)
    rec = bench_legs.make_records(torch, n, d, None, 17 + (warmup + steps - 1) % 3, dev)
    ref = D.aggregate(w["alg"], rec, n, d, d, dense=True).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), ref.view(np.uint32))
    # same arguments, same inputs, same output
    _, b = _run(capsys, tmp_path / "b", steps, warmup)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
