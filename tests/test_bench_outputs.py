"""bench.py's plain run and `--dump-outputs DIR`: a plain run times exactly `--steps` steps on one index build and leaves every
`--full` leg out of the line; the dump is what the last timed step returned, in float64 / float32, at most 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_types_and_size_cap(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rows = np.arange(3 * 100, dtype=np.int64).reshape(3, 100)
    scores = np.linspace(1, 0, 300, dtype=np.float32).reshape(3, 100)
    bench.dump_outputs(str(tmp_path / "small"), rows, scores, np.full(3, 100, np.int32))
    r, s, c = (np.load(tmp_path / "small" / f"{n}.npy") for n in ("rows", "scores", "counts"))
    assert r.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64
    assert np.array_equal(r, rows) and np.array_equal(s, scores) and np.array_equal(c, [100, 100, 100])
    # above 64 MB: a fixed, seeded sample of the queries (the same one every time), whole lists
    nq, k = 64, 100_000
    rows = np.arange(nq * k, dtype=np.int64).reshape(nq, k)
    scores = np.zeros((nq, k), np.float32)
    counts = np.full(nq, k, np.int32)
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), rows, scores, counts)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64 << 20
    a, b = np.load(tmp_path / "big1" / "rows.npy"), np.load(tmp_path / "big2" / "rows.npy")
    assert a.shape[1] == k and 1 <= a.shape[0] < nq and np.array_equal(a, b)
    assert np.array_equal(a, rows[(a[:, 0] // k).astype(np.int64)])


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_run_times_the_steps_asked_for_and_dumps_the_exact_answer(tmp_path, gpus):
    """gpus = 2: two ranks pinned to device 0 over gloo (RCCL refuses two ranks on one device), 100 000 rows each under weak
    scaling: the same 200 000-row corpus, so the same answer."""
    from oracle import oracle_c as oc
    import bench
    rows_n, dim, k, steps = 200_000, 768, 100, 7
    env = dict(os.environ)
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NMN_BENCH_DEVICE"):
        env.pop(key, None)
    if gpus > 1:
        env.update(NMN_BENCH_DEVICE="0", NMN_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", str(steps), "--warmup", "2",
                        "--rows", str(rows_n // gpus), "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       timeout=600, env=env)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == gpus and d["config"]["rows_total"] == rows_n
    assert d["steps"] == steps and d["warmup"] == 2 and d["rebuilds"]["n"] == 1
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for leg in ("parity", "cpu_baseline", "mirror_legs", "batched", "concurrent_callers", "other_configs", "next_rows"):
        assert d[leg] is None, leg
    # the last timed step's query is query set (steps - 1) % 16 of the bench's seeded generator, over the seeded corpus
    A = oc.synth(bench.SEED_CORPUS, 0, rows_n, dim)
    q = oc.synth(bench.SEED_QUERY, (steps - 1) % 16, 1, dim)[0]
    er, es = oc.search(A, q, k, oc.COSINE)
    got_r, got_s, got_c = (np.load(tmp_path / f"{n}.npy") for n in ("rows", "scores", "counts"))
    assert got_r.shape == (1, k) and got_s.dtype == np.float32 and got_c.tolist() == [k]
    assert np.array_equal(got_r[0].astype(np.uint64), er) and np.array_equal(got_s[0], es)
