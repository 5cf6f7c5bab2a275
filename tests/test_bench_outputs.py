"""bench.py --dump-outputs and --full, on the CPU: the dump holds the verdict
of every record of the last step in record order (float32), is the same file
from run to run, and of a batch over DUMP_MAX records it is a fixed seeded
sample; a plain run's options parse with and without --full."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    return {k: v for k, v in os.environ.items()
            if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HKV_BENCH_SPAWNED")}


def test_dump_outputs_unpacks_the_bitmap_in_record_order(tmp_path):
    import bench
    from hkv.records import bits_from_bools
    n = 64 * 5 + 13
    want = bench.mock_pattern(np.arange(n)).astype(bool)
    d = tmp_path / "new" / "dir"  # (created by the dump)
    bench.dump_outputs(str(d), bits_from_bools(want), n)
    assert sorted(os.listdir(d)) == ["verdicts.npy"]
    got = np.load(d / "verdicts.npy")
    assert got.dtype == np.float32 and got.shape == (n,)
    assert (got == want.astype(np.float32)).all()


def test_dump_outputs_samples_a_large_batch(tmp_path, monkeypatch):
    import bench
    from hkv.records import bits_from_bools
    monkeypatch.setattr(bench, "DUMP_MAX", 100)
    n = 1000
    want = bench.mock_pattern(np.arange(n)).astype(bool)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), bits_from_bools(want), n)
    a, b = np.load(tmp_path / "a" / "verdicts.npy"), np.load(tmp_path / "b" / "verdicts.npy")
    assert a.dtype == np.float32 and a.shape == (100,) and (a == b).all()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, 100, replace=False))
    assert len(set(idx.tolist())) == 100 and (a == want[idx].astype(np.float32)).all()
    # at the bound itself nothing is sampled
    bench.dump_outputs(str(tmp_path / "c"), bits_from_bools(want[:100]), 100)
    assert (np.load(tmp_path / "c" / "verdicts.npy") == want[:100].astype(np.float32)).all()


def test_bench_run_writes_its_last_step(tmp_path):
    """The run itself (the --mock-cpu leg: the same step, timing and dump as
    the GPU run, a pattern writer instead of hkv_verify_device), with and
    without --full: the same verdicts, and --steps sets the timed steps."""
    n = 4096 + 65
    outs = []
    for name, extra in (("plain", []), ("full", ["--full"])):
        d = tmp_path / name
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--mock-cpu", "--steps", "3", "--warmup", "1",
                            "--config4-n", str(n), "--dump-outputs", str(d)] + extra,
                           capture_output=True, text=True, timeout=240, env=_env())
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert line["steps"] == 3 and line["mismatches"] == 0
        outs.append(np.load(d / "verdicts.npy"))
    import bench
    assert outs[0].dtype == np.float32 and outs[0].shape == (n,)
    assert (outs[0] == outs[1]).all()
    assert (outs[0] == bench.mock_pattern(np.arange(n)).astype(np.float32)).all()
