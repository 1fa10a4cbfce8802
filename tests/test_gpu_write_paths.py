"""Every row-write path against the mirrors it must keep current (docs/exactness.md, "Writes").

A flat shard answers from a mirror (8-bit codes or bf16) and re-scores the candidates exactly.  That is the reference's answer
only while every mirror row is the rounding of the CURRENT f32 row and the measured error maxima cover EVERY row the mirror
holds — established when rows arrive, and to be kept by every later write: rows_written() of nmn_api.hip picks among the fused
ingest kernels, the separate norms / half_patch / q8_patch passes and the lazy extension of search_enqueue by stride, dim % 8,
the mirrors that exist and where the write lands.  A row left stale or a maximum that did not rise shifts no score: a true
top-k row drops out of the candidate list, for queries near that row only.

1. `test_write_script_*`: a numpy model of the shard, one script of writes over every path (upload, append, set_row, overwrite
   across tile borders, two appends behind a mirror that lags and an overwrite across its end, fill_synthetic into the middle,
   upload_device, a bulk upload over a live mirror, set_rows down, an append there, set_rows up), and after every step the
   same battery of searches against the oracle on the model: rows, counts, score bits, unused slots, no exact fallback, the
   sweep and its element size.  Every write plants WINNERS — rows that enter the top-k of the single query and of one query
   of the batch under all three metrics: a stale mirror row loses one, a stale magnitude shows in the score bits.
2. `test_attack_that_arrives_by_write`: the worst-case corpora of tests/_margin_attack.py where the worst-case rows arrive
   AFTER the mirror and its maxima exist (written_attack; tests/test_margin_attack_cpu.py proves that the maxima measured
   before the write lose the target and the true ones keep it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _margin_attack as ma
from tests.test_gpu_margin_attack import _batch, _check

pytestmark = pytest.mark.gpu
F = np.float32
COS, L2, DOT = ma.COS, ma.L2, ma.DOT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
CAP = 8192               # rows of every shard here: above the 8-bit mirror's smallest shard (4096 rows)

# dim -> (row stride, the mirror built while the rows arrive, the write path of rows_written)
SHAPES = {256: (256, "i8", "fused ingest_q8_kernel"),
          120: (128, "i8", "fused, 8 zero padding columns that must stay zero"),
          250: (256, "i8", "norms_kernel + q8_patch (dim % 8 != 0)"),
          2176: (2176, "i8", "ingest_kernel + q8_patch (stride > 2048)"),
          320: (320, "bf16", "ingest_kernel with the half"),
          100: (104, "bf16", "norms_kernel + half_patch")}
ELEM_BYTES = {"valu_i8": 1, "mfma_i8": 1, "valu_bf16": 2, "mfma_bf16": 2, "valu_f32": 4, "mfma_f32": 4}


def expected_sweep(dim, stride, mode, nq, n_rows):
    """The sweep search_enqueue picks for a pass of nq queries (1, 2 or 8 here) over n_rows rows of this shape under
    set_mirror(mode) — from the conditions it states: the matrix cores from 5 queries on (3 on rows of >= 768 elements)
    over rows of 1-6, 8, 10, 12, 16, 24 or 32 stages of 128; the 8-bit mirror from 4096 rows on, for 1-2 queries over rows
    of whole 128-element halves and for batches over rows of 256 .. 1536 or 2048 elements in 256-element groups; else the
    bf16 mirror (strides of whole 8-element groups); mode 0 reads the f32 rows."""
    kc = stride // 128
    mfma = nq >= (3 if dim >= 768 else 5) and stride % 128 == 0 and (1 <= kc <= 6 or kc in (8, 10, 12, 16, 24, 32))
    if mode == 0:
        return "mfma_f32" if mfma else "valu_f32"
    if mfma:
        i8 = stride % 256 == 0 and (stride <= 1536 or stride in (2048, 3072))
    else:
        i8 = nq <= 2 and stride % 128 == 0 and stride <= 4096
    if mode == 1 and n_rows >= 4096 and i8:
        return "mfma_i8" if mfma else "valu_i8"
    assert stride % 8 == 0
    return "mfma_bf16" if mfma else "valu_bf16"


# ---------------------------------------------------------------------------------------------- 1. the write script
class Shard:
    """The index under test, its numpy model, and the data both are written with."""

    def __init__(self, idx, dim, mode, seed):
        self.idx, self.dim, self.mode, self.stride = idx, dim, mode, idx.row_stride
        self.rng = np.random.default_rng(seed)
        self.M = np.zeros((CAP, dim), F)
        self.n = 0
        self.level = 0
        self.q0 = self.rng.standard_normal(dim).astype(F)
        self.Qb = self.rng.standard_normal((8, dim)).astype(F)
        self.searches = 0

    # -- data ---------------------------------------------------------------------------------------------------------
    def ordinary(self, n):
        return self.rng.standard_normal((n, self.dim)).astype(F)

    def winner(self, q):
        """A row that outranks every ordinary row and every earlier winner of q under all three metrics: q (1 + eps) + noise
        orthogonal to q, eps growing (the dot product) and the noise shrinking faster (cosine, distance) from winner to winner."""
        s, self.level = self.level, self.level + 1
        q64 = q.astype(np.float64)
        noise = self.rng.standard_normal(self.dim)
        noise -= (noise @ q64) / (q64 @ q64) * q64
        return (q64 * (1.0 + 0.0005 * s) + noise * 0.5 * 0.9 ** s).astype(F)

    def rows_with_winners(self, lo, hi):
        """Ordinary rows for [lo, hi) with four winners: of the single query at both ends, of query 5 of the batch in the
        middle and on the first tile border inside (else next to the start)."""
        X = self.ordinary(hi - lo)
        border = (lo // 64 + 1) * 64
        at = {"q0": [lo, hi - 1], "qb": sorted({lo + (hi - lo) // 2, border if lo < border < hi - 1 else lo + 1})}
        for key, q in (("q0", self.q0), ("qb", self.Qb[5])):
            for r in at[key]:
                X[r - lo] = self.winner(q)
        return X, at

    # -- the battery --------------------------------------------------------------------------------------------------
    def check(self, Q, k, metric, mode, mask=None, kept=None, tag=""):
        A = self.M[:self.n]
        rows, scores, counts, st = self.idx.search(Q, k, metric, mask=mask, with_stats=True)
        self.searches += 1
        where = (tag, self.dim, "mode", mode, "metric", metric, "nq", Q.shape[0], "k", k, "masked" if mask is not None else "")
        want = []
        for i in range(Q.shape[0]):
            er, es = oc.search(A, Q[i], k, metric, mask=mask, nthreads=8, partial=True, native=True)
            c = er.size
            want.append(er)
            assert counts[i] == c, (where, i, int(counts[i]), c)
            assert np.array_equal(rows[i, :c], er), (where, i, rows[i, :c], er)
            assert np.array_equal(scores[i, :c].view(np.uint32), es.view(np.uint32)), (where, i, scores[i, :c], es)
            assert np.all(rows[i, c:] == U64_MAX) and np.all(np.isneginf(scores[i, c:])), (where, i)
            assert np.all(rows[i, :c] < np.uint64(self.n)), (where, i)
        sweep = expected_sweep(self.dim, self.stride, mode, Q.shape[0], self.n)
        assert st.fallback_queries == 0, (where, st.fallback_queries, "the exact scan would hide a stale mirror")
        assert st.sweep == sweep, (where, st.sweep, sweep)
        scanned = self.n if kept is None else kept          # (a host bitmap: the rows it keeps, the others are never read)
        assert st.rows_scanned == scanned and st.bytes_scanned == scanned * self.dim * ELEM_BYTES[sweep], (where, st.rows_scanned, st.bytes_scanned)
        return want

    def battery(self, tag, winners=None, modes=None):
        """1 query (k = 10), 2 (k = 37) and 8 (k = 10) under every metric, and the single query under a 30 % bitmap that keeps
        this step's winners; the winners of the step must be in the oracle's own answers (a condition on the inputs)."""
        for mode in (modes or [self.mode]):
            if modes:
                self.idx.set_mirror(mode)
            for metric in (COS, L2, DOT):
                w1 = self.check(self.q0[None, :], 10, metric, mode, tag=tag)
                self.check(self.Qb[4:6], 37, metric, mode, tag=tag)
                w8 = self.check(self.Qb, 10, metric, mode, tag=tag)
                if winners:
                    assert set(winners["q0"]) <= set(w1[0].tolist()), (tag, metric, winners["q0"], w1[0])
                    assert set(winners["qb"]) <= set(w8[5].tolist()), (tag, metric, winners["qb"], w8[5])
            keep = np.random.default_rng(self.searches).random(self.n) < 0.3
            if winners:
                keep[[r for r in winners["q0"] if r < self.n]] = True
            self.check(self.q0[None, :], 10, (COS, L2, DOT)[self.searches % 3], mode, mask=oc.mask_from_bool(keep), kept=int(keep.sum()),
                       tag=tag + " bitmap")
        if modes:
            self.idx.set_mirror(self.mode)

    # -- writes -------------------------------------------------------------------------------------------------------
    def put(self, lo, X):
        self.M[lo:lo + X.shape[0]] = X
        self.n = max(self.n, lo + X.shape[0])

    def upload(self, lo, hi):
        X, at = self.rows_with_winners(lo, hi)
        self.idx.upload(X, row0=lo)
        self.put(lo, X)
        return at

    def merge(self, *ats):
        return {key: [r for at in ats for r in at[key]] for key in ("q0", "qb")}


def run_script(dim, variant):
    """The script of the issue, the same for every shape.  variant: "default"; "bf16" (set_mirror(2) from the start); "late"
    (set_mirror(0) before the rows, set_mirror(1) after step 5: the whole mirror is built lazily over rows that were already
    overwritten); "both" (both mirrors alive: from step 2 on every battery runs under modes 1 and 2)."""
    import torch
    from neumann_amd import GpuFlatIndex
    stride, first, path = SHAPES[dim]
    mode = {"default": 1, "bf16": 2, "late": 0, "both": 1}[variant]
    with GpuFlatIndex(dim, CAP, single_launch=False) as idx:
        assert idx.row_stride == stride, (dim, idx.row_stride, stride, path)
        if mode != 1:
            idx.set_mirror(mode)
        s = Shard(idx, dim, mode, seed=0x5C21 + dim)
        modes = None
        # 1. not bulk: no mirror while the rows arrive
        at = s.upload(0, 3000)
        s.battery("1 upload [0, 3000)", at)
        # 2. append
        at = s.upload(3000, 8000)
        s.battery("2 append [3000, 8000)", at)
        if variant == "both":
            modes = [1, 2]
            s.battery("2 both mirrors", at, modes)
        # 3. set_row at rows 0, 63, 64 and the last row; then the current best row becomes an ordinary one
        at = {"q0": [0, 64], "qb": [63, s.n - 1]}
        for key, q in (("q0", s.q0), ("qb", s.Qb[5])):
            for r in at[key]:
                v = s.winner(q)
                idx.set_row(r, v)
                s.M[r] = v
        s.battery("3 set_row 0, 63, 64, last", at, modes)
        best = int(oc.search(s.M[:s.n], s.q0, 1, COS)[0][0])
        assert best == 64
        v = s.ordinary(1)[0]
        idx.set_row(best, v)
        s.M[best] = v
        s.battery("3 set_row over the best row", None, modes)
        # 4. an overwrite across three tile borders
        at = s.upload(1000, 1200)
        s.battery("4 overwrite [1000, 1200)", at, modes)
        # 5. two appends with no search between (the patch paths' mirror lags twice), an overwrite across the mirror's end
        a1 = s.upload(8000, 8100)
        a2 = s.upload(8100, CAP)
        a3 = s.upload(7990, 8110)
        at = s.merge(a3, {"q0": [r for r in a1["q0"] + a2["q0"] if not 7990 <= r < 8110],
                          "qb": [r for r in a1["qb"] + a2["qb"] if not 7990 <= r < 8110]})
        s.battery("5 appends [8000, 8100), [8100, 8192), overwrite [7990, 8110)", at, modes)
        if variant == "late":
            s.mode = 1
            idx.set_mirror(1)
            s.battery("5 set_mirror(1): the mirror built lazily", at)
        # 6. synthetic rows into the middle
        idx.fill_synthetic(0xF111 + dim, 600, row0=4000)
        s.put(4000, oc.synth(0xF111 + dim, 4000, 600, dim))
        s.battery("6 fill_synthetic [4000, 4600)", None, modes)
        # 7. upload_device as an overwrite, then a host search
        X, at = s.rows_with_winners(2000, 2100)
        t = torch.from_numpy(X).cuda()
        idx.upload_device(t, row0=2000)
        s.put(2000, X)
        s.battery("7 upload_device [2000, 2100)", at, modes)
        del t
        # 8. a bulk upload over a live mirror
        at = s.upload(0, 5000)
        s.battery("8 upload [0, 5000)", at, modes)
        # 9. set_rows moves the row count and touches nothing else
        idx.set_rows(6000)
        s.n = 6000
        assert idx.rows == 6000
        s.battery("9 set_rows(6000)", None, modes)
        at = s.upload(6000, 6050)
        assert idx.rows == 6050 and s.n == 6050
        s.battery("9 upload [6000, 6050)", at, modes)
        idx.set_rows(CAP)
        s.n = CAP
        s.battery("9 set_rows(8192): rows 6050.. are back, in the corpus and the mirror alike", None, modes)
        return s.searches


@pytest.mark.parametrize("dim", list(SHAPES), ids=[f"{d}-stride{SHAPES[d][0]}-{SHAPES[d][1]}" for d in SHAPES])
def test_write_script_in_the_default_mode(dim):
    run_script(dim, "default")


@pytest.mark.parametrize("variant", ["bf16", "late", "both"])
def test_write_script_under_other_mirror_modes(variant):
    run_script(256, variant)


@pytest.mark.parametrize("dim", [256, 320])
def test_write_script_with_the_separate_pass_kernels_in_a_child_process(dim):
    """NMN_NO_INGEST=1 (read once per process): norms_kernel + half_patch + q8_patch on the shapes the fused kernels serve"""
    code = (
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from tests import test_gpu_write_paths as t\n"
        f"print('SCRIPT-OK', t.run_script({dim}, 'default'))\n"
    )
    env = dict(os.environ, NMN_NO_INGEST="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SCRIPT-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---------------------------------------------------------------------------------------------- 2. attacks that arrive by write
def _same(idx, M, Q, k, metric):
    rows, scores, counts = idx.search(Q, k, metric)
    for i in range(Q.shape[0]):
        er, es = oc.search(M, Q[i], k, metric, nthreads=8, partial=True, native=True)
        assert counts[i] == er.size and np.array_equal(rows[i, :er.size], er), (i, rows[i], er)
        assert np.array_equal(scores[i, :er.size].view(np.uint32), es.view(np.uint32)), (i, scores[i], es)


def _write(idx, A, planted, kind):
    lo, hi = int(planted.min()), int(planted.max()) + 1
    if kind == "set_row":
        for r in planted:
            idx.set_row(int(r), A[r])
    elif kind == "upload":
        idx.upload(A[lo:hi], row0=lo)
    else:
        import torch
        t = torch.from_numpy(A[lo:hi]).cuda()
        idx.upload_device(t, row0=lo)
        torch.cuda.synchronize()


def _attack_cases():
    out = []

    def add(name, metric, kw, flow, sweep, model, layouts):
        for lay in layouts:
            for kind in ("set_row", "upload", "upload_device"):
                kws = "".join(f"-{k}{v}" for k, v in sorted(kw.items()))
                out.append(pytest.param(name, metric, kw, flow, sweep, model, lay, kind,
                                        id=f"{flow}-{sweep}-{name}-{'cos l2 dot'.split()[metric]}{kws}-{lay}-{kind}"))

    for m in (COS, DOT, L2):
        add("rows_bf16", m, {}, "mode2", "valu_bf16", "valu_bf16", ["1"])
    for m in (COS, L2):
        add("rows_bf16", m, {}, "mode2", "mfma_bf16", "mfma_bf16", ["8b"])
    # the bf16 mirror built first, set_mirror(0) afterwards: the f32 matrix-core sweep takes half_err_bits, which the write must have raised
    add("rows_bf16", COS, {}, "mode2then0", "mfma_f32", "mfma_bf16", ["8b"])
    for m in (COS, DOT, L2):
        add("rows_i8", m, {}, "mode1", "valu_i8", "valu_i8", ["1", "2b"])
    add("rows_i8", DOT, {}, "mode1", "mfma_i8", "mfma_i8", ["8a"])
    add("rows_i8", COS, {"planes": 1}, "mode1", "mfma_i8", "mfma_i8_one", ["8a"])
    # both mirrors: the 8-bit one while the rows arrive, bf16 on demand; the write is the fused 8-bit branch's, half_patch behind it
    add("rows_bf16", COS, {}, "both", "valu_bf16", "valu_bf16", ["1"])
    return out


@pytest.mark.parametrize("name,metric,kw,flow,sweep,model,layout,kind", _attack_cases())
def test_attack_that_arrives_by_write(name, metric, kw, flow, sweep, model, layout, kind):
    """Upload the shard without its planted rows (B), search once (the mirror and its maxima exist, measured on the bulk), write
    the planted rows, and hold the answer to the oracle on A as tests/test_gpu_margin_attack.py does: the sweep named, no exact
    fallback, no more rows re-scored than planted.
    (Euclidean on the 8-bit VALU sweep: the search on B leaves a threshold distance of 566 against |q| = 558.5, so qprep_kernel
    gives the attacked search estimator B, |q|^2 + |v|^2 - 2 q~.v~, while the model's figures are estimator A's.  The query is
    parallel to the rows' error on G as well: target and k-th decoy are 4 |q_G . e_G| = 4 * 34 * 0.5 * 246 = 16 728 of squared
    distance apart against a margin of 2 * 1.001 * 2 |q| e_abs = 17 550 with the true e_abs 7.85 and 4 680 with the stale 2.09.)"""
    from neumann_amd import GpuFlatIndex
    B, A, q, k, planted, info = ma.written_attack(name, metric, **kw)
    v = info["by_sweep"][model]
    print(f"{name}: sharpness {v['sharpness']:.4f}, with the maxima from before the write {info['stale_sharpness'][model]:.3f} "
          f"({info['stale_err_sharpness'][model]:.3f} with the current largest magnitude)")
    assert info["floor"] <= v["sharpness"] < 1.0 < min(info["stale_sharpness"][model], info["stale_err_sharpness"][model])
    Q, _ = _batch(q, layout)
    with GpuFlatIndex(A.shape[1], A.shape[0], single_launch=False) as idx:
        idx.set_mirror(1 if flow in ("mode1", "both") else 2)
        idx.upload(B)
        _same(idx, B, Q, k, metric)
        if flow == "both":
            idx.set_mirror(2)
            _same(idx, B, Q, k, metric)          # builds the bf16 mirror beside the 8-bit one, its maxima from the bulk
            idx.set_mirror(1)
        if flow == "mode2then0":
            idx.set_mirror(0)
        _write(idx, A, planted, kind)
        if flow == "both":
            idx.set_mirror(2)
        _check(idx, A, Q, k, metric, sweep, planted.size)
