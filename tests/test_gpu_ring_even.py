"""The ring sweep with its tiles split over long workgroups and a tail of short ones (nmn_scan_ring.hip, ring_even_grid): workgroup
ranges no longer match the wmax groups select_kernel reads, so a group shared by two or more workgroups is joined by atomicMax into
an entry the launching stream zeroed.  Rows and scores must be the oracle's for every metric, on shards just above and at the
4096-tile threshold, with a partial last tile, under the default grid, under a grid forced to many tiny workgroups (every group
shared) and under NMN_NO_RING_EVEN=1 (one workgroup per group, the previous form).  The grid knobs are read once per process, so
each grid runs in a child process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
TILES = 4096 * 64  # rows of the smallest shard the ring sweep takes

# (rows, dim, k): just above the threshold with a partial last tile, exactly at it, just below it (scan_kernel), and row lengths
# 128 .. 1536 (1000: stride padded to 1024)
SHAPES = [(TILES + 64 + 5, 768, 100), (TILES, 128, 10), (TILES - 64, 768, 20), (TILES + 3 * 64 + 1, 1536, 50),
          (TILES + 777, 1000, 30), (TILES + 640, 384, 100)]


def _child(grid):
    """Runs in a child process: every shape and metric against the oracle; prints one JSON line."""
    from neumann_amd import GpuFlatIndex
    from oracle import oracle_c as oc
    out = []
    for n, d, k in SHAPES:
        A = oc.synth(7100 + d, 0, n, d, nthreads=8)
        Q = oc.synth(7200 + d, 0, 2, d)
        Q[1] = A[n - 1]                 # a stored row in the last (partial) tile
        with GpuFlatIndex(d, n) as idx:
            idx.set_mirror(0)
            idx.fill_synthetic(7100 + d, n)
            for metric in (0, 1, 2):
                for qi in range(2):
                    rows, scores, counts, st = idx.search(Q[qi], k, metric, with_stats=True)
                    er, es = oc.search(A, Q[qi], k, metric, nthreads=8, partial=True, native=True)
                    c = er.size
                    ok = (counts[0] == c and np.array_equal(rows[0, :c], er) and bool(np.all(scores[0, :c] == es))
                          and bool(np.all(rows[0, c:] == U64_MAX)))
                    out.append({"n": n, "d": d, "metric": metric, "q": qi, "ok": bool(ok), "sweep": st.sweep,
                                "bytes": int(st.bytes_scanned), "rows": int(st.rows_scanned)})
    print(json.dumps({"grid": grid, "results": out}))


def _run(env_extra):
    env = dict(os.environ)
    for key in ("NMN_NO_RING_EVEN", "NMN_RING_MAIN", "NMN_RING_TAIL", "NMN_NO_RING"):
        env.pop(key, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(env_extra)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])["results"]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [{}, {"NMN_RING_MAIN": "1", "NMN_RING_TAIL": "31"}, {"NMN_RING_MAIN": "16", "NMN_RING_TAIL": "0"},
                                  {"NMN_NO_RING_EVEN": "1"}], ids=["default", "tiny_tail", "even_no_tail", "one_per_group"])
def test_ring_grid_matches_oracle(grid):
    res = _run(grid)
    assert len(res) == len(SHAPES) * 6
    for r in res:
        assert r["ok"], r
        ring = r["n"] >= TILES
        assert r["sweep"] == ("ring_f32" if ring else "valu_f32"), r
        assert r["rows"] == r["n"] and r["bytes"] == r["n"] * r["d"] * 4, r


if __name__ == "__main__":
    _child(json.loads(sys.argv[1]) if len(sys.argv) > 1 else {})
