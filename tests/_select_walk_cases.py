"""The cases of tests/test_gpu_select_walk.py: select_kernel's three-level walk (wave maxima -> tile maxima -> row scores) at its
edges, on shards small enough for a test.  numpy and the oracle only: the CPU test (tests/test_select_walk_cases_cpu.py) checks
every construction, the GPU worker (tests/_select_walk_worker.py) and the GPU test run them.

FORCED cases are small shards searched with NMN_NO_FLAT_SELECT=1 (read once per process: a child process), NATURAL cases are
shards of just over 16 384 tiles on which launch_select itself picks the walk.

The wave geometry of every sweep is restated from search_enqueue (nmn_api.hip) in geometry(): which tiles share a scan wave
decides which planted rows meet at the wave level, and which of the walk's three gathers of the tile maxima a case reaches:
  dense    nA * tpw * 2 >= n_tiles (nA: waves whose maximum reaches the wave-level bound): the tile maxima read linearly, 16 B a lane
  quads    else, contiguous ranges of tpw >= 8 tiles: the passing waves' ranges, 16 B a lane
  generic  else (tpw < 8, or the strided numbering of masked VALU sweeps: tile j of wave w is j * W + w)
The library does not report the gather; wave_share() computes the share of the waves that reach the k-th largest wave maximum
from the oracle's exact scores, and a case that names a gather must be far from the kernel's 0.5 (>= 0.7 dense, <= 0.3 else)."""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle_c as oc
from tests import _margin_attack as ma
from tests import _corpora

F = np.float32
COS, L2, DOT = 0, 1, 2
TILE = 64
MAX_SCAN_WAVES = 4096       # kMaxScanWaves
FLAT_TILES = 16384          # kFlatTiles: launch_select's flat path up to here
SPLIT_MAX_K, SPLIT_MAX_NQ = 256, 4
LIST_CAP = 4096             # kListCap
BAIL_TILES = 1024           # kBailTiles: more tiles than this within the margin hand over to the crowd kernels
CAND_CAP = 4096             # default candidate capacity per query
CROWD_MIN_ROWS = 1 << 18    # shards from here on have the crowd kernels and the f32 retry behind the selection
ELEM_BYTES = {"ring_f32": 4, "valu_f32": 4, "mfma_f32": 4, "valu_bf16": 2, "mfma_bf16": 2, "valu_i8": 1, "mfma_i8": 1}


# ---------------------------------------------------------------------------------------------- geometry
@dataclass(frozen=True)
class Geometry:
    n_tiles: int
    tpw: int            # tiles per scan wave (matrix-core sweeps: per workgroup; ring: per group of the wave-maximum level)
    W: int              # scan waves that own tiles
    strided: bool       # tile j of wave w is j * W + w (masked VALU sweeps); else w * tpw + j

    def wave_of_tile(self, t):
        return t % self.W if self.strided else t // self.tpw

    def wave_of_row(self, r):
        return self.wave_of_tile(r // TILE)

    def tiles_of_wave(self, w):
        t = [j * self.W + w for j in range(self.tpw)] if self.strided else range(w * self.tpw, (w + 1) * self.tpw)
        return [x for x in t if x < self.n_tiles]


def row_stride(d):
    """ld of include/neumann_gpu.h: dim rounded up to 8, or to the next multiple of 128 if that is at most 1/8 more."""
    up128 = (d + 127) // 128 * 128
    return up128 if up128 * 8 <= d * 9 else (d + 7) // 8 * 8


def geometry(n_rows, d, sweep, masked):
    """search_enqueue's ScanParams::tiles_per_wave / strided and SelectParams::n_waves for a sweep kind (default knobs)."""
    n_tiles = -(-n_rows // TILE)
    cdiv = lambda a, b: max(1, -(-a // b))  # noqa: E731
    if sweep.startswith("mfma"):
        tpw = cdiv(n_tiles, 1024)                         # 1024 workgroups
    elif sweep == "ring_f32":
        tpw = cdiv(n_tiles, MAX_SCAN_WAVES)
    else:
        tpw = cdiv(n_tiles, MAX_SCAN_WAVES)
        nbytes = n_rows * row_stride(d) * ELEM_BYTES[sweep]
        if not masked and (128 << 20) <= nbytes < (2 << 30):   # sweeps of 0.125 .. 2 GiB run on 768 waves
            tpw = cdiv(n_tiles, 768)
    return Geometry(n_tiles, tpw, -(-n_tiles // tpw), bool(masked) and not sweep.startswith("mfma"))


def expected_form(n_rows, nq, k):
    """launch_select's choice without switches: 'flat', 'split' or 'walk'."""
    n_tiles = -(-n_rows // TILE)
    if n_tiles <= FLAT_TILES:
        return "flat"
    parts = -(-n_tiles // FLAT_TILES)
    return "split" if nq <= SPLIT_MAX_NQ and k <= SPLIT_MAX_K and 2 <= parts <= 16 else "walk"


def keep_bits(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def wave_share(scores, geo, k, keep=None):
    """Share of the scan waves (weighted by their tiles: the kernel compares nA * tpw * 2 with n_tiles) whose maximum reaches the
    k-th largest wave maximum, on exact scores.  Fewer valid waves than k: every valid wave passes."""
    n = scores.size
    s = np.full(geo.n_tiles * TILE, -np.inf)
    s[:n] = np.where(np.isnan(scores), -np.inf, scores.astype(np.float64))
    valid = np.zeros(geo.n_tiles * TILE, bool)
    valid[:n] = True if keep is None else keep
    s[~valid] = -np.inf
    tmax = s.reshape(geo.n_tiles, TILE).max(axis=1)
    tval = valid.reshape(geo.n_tiles, TILE).any(axis=1)
    wave = np.array([geo.wave_of_tile(t) for t in range(geo.n_tiles)]) if geo.n_tiles < 1024 else (
        np.arange(geo.n_tiles) % geo.W if geo.strided else np.arange(geo.n_tiles) // geo.tpw)
    wmax = np.full(geo.W, -np.inf)
    np.maximum.at(wmax, wave, tmax)
    wval = np.zeros(geo.W, bool)
    wval[wave[tval]] = True
    vw = int(wval.sum())
    if vw == 0:
        return 0.0
    thr = -np.inf if vw < k else np.sort(wmax[wval])[::-1][k - 1]
    nA = int((wval & (wmax >= thr)).sum())
    return nA * geo.tpw / geo.n_tiles


# ---------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    id: str
    corpus: tuple               # key of a recipe in build_corpus(): (name, args...)
    nq: int
    k: int
    metric: int
    mode: int                   # set_mirror: 0 f32 rows, 1 smallest mirror (8-bit), 2 bf16
    sweep: str                  # the sweep kind that must serve the call (nmn_search_stats.sweep_kind)
    aims: str                   # the walk behaviour the case aims at (docs/kernels-select-exact-final.md)
    mask: tuple = None          # key of a bitmap recipe in build_mask()
    forced: bool = True
    gather: str = None          # 'dense' / 'quads' / 'generic': checked by wave_share() where stated
    fallback: tuple = (0, 0)    # allowed range of fallback_queries
    rescored_max: int = None    # candidates_rescored <= this (margin attacks: the planted rows)
    rescored_min: int = None    # candidates_rescored >= this (crowds)
    cand_cap: int = 0
    form: str = "walk"
    borders: tuple = ()         # ((row, tile, wave), ...) claimed positions of planted rows under this case's geometry
    tie_len: int = 0            # length of the run of equal scores at the top of query 0's answer (after `lead` better rows)
    lead: int = 0
    crowd_over: tuple = None    # (what, cap): the planted crowd must exceed this cap


@dataclass
class Corpus:
    A: np.ndarray
    q: np.ndarray               # the query the planted rows are about
    planted: np.ndarray = None  # rows planted for q (the oracle's answer starts with them, in some order)
    synthetic: tuple = None     # (seed, [rows overwritten]) when the GPU copy is fill_synthetic + set_row
    ties: np.ndarray = None     # rows that are exact copies of one another
    info: dict = field(default_factory=dict)


def _near_copies(q, j, rng):
    """Near-copy number j of q (the recipe of test_split_selection_on_a_large_shard_matches_oracle): the best rows under all
    three metrics, all different."""
    v = (q * F(1.0 + 0.05 * (j % 3))).astype(F)
    v[rng.integers(0, q.size, size=2)] += F(1e-3 * (j + 1))
    return v


def _synth_with_plants(seed, n, d, rows):
    A = oc.synth(seed, 0, n, d, nthreads=8)
    q = oc.synth(seed + 1, 0, 1, d)[0]
    rng = np.random.default_rng(seed)
    for j, r in enumerate(rows):
        A[r] = _near_copies(q, j, rng)
    planted = np.array(sorted(rows), np.int64)
    return Corpus(A, q, planted, synthetic=(seed, [int(r) for r in planted]))


def _tie_vectors(q, rng):
    """b2 > b1 > c under all three metrics (c is the vector of the copies): c = 0.9 q + e, b1 = 0.95 q + e / 2, b2 = q with e
    orthogonal to q, |e| = 0.3 |q|."""
    e = rng.standard_normal(q.size)
    e -= (e @ q.astype(np.float64)) / float(q.astype(np.float64) @ q) * q
    e *= 0.3 * np.linalg.norm(q) / np.linalg.norm(e)
    return q.copy(), (0.95 * q + 0.5 * e).astype(F), (0.9 * q + e).astype(F)


@functools.lru_cache(maxsize=2)
def build_corpus(key):
    name = key[0]
    if name == "natural":
        return build_natural(key)
    if name == "borders":                 # (name, seed, n, d, rows): near-copies of q at `rows`
        _, seed, n, d, rows = key
        return _synth_with_plants(seed, n, d, rows)
    if name == "plain":                   # (name, seed, n, d): synthetic rows, nothing planted
        _, seed, n, d = key
        return Corpus(oc.synth(seed, 0, n, d, nthreads=8), oc.synth(seed + 1, 0, 1, d)[0], synthetic=(seed, []))
    if name == "ties":                    # (name, seed, n, d, copy rows): two better rows, then exact copies
        _, seed, n, d, rows = key
        rng = np.random.default_rng(seed)
        A = oc.synth(seed, 0, n, d, nthreads=8)
        q = oc.synth(seed + 1, 0, 1, d)[0]
        b2, b1, c = _tie_vectors(q, rng)
        lead = [100, n - 1000]
        A[lead[0]], A[lead[1]] = b2, b1
        A[list(rows)] = c
        ties = np.array(sorted(rows), np.int64)
        return Corpus(A, q, np.concatenate([lead, ties]), synthetic=(seed, lead + list(rows)), ties=ties)
    if name == "attack":                  # (name, construction, metric, sorted kwargs): tests/_margin_attack.py
        _, cname, metric, kw = key
        A, q, k, _, planted, info = ma.build(cname, metric, **dict(kw))
        return Corpus(A, q, planted, info=dict(k=k, by_sweep=info["by_sweep"], floor=info["floor"]))
    if name == "straddle":                # every row tiny, near-ties of one row around the cut (test_gpu_underflow's corpus, smaller)
        _, n, d = key
        A, tie = _corpora.straddle_corpus(np.random.default_rng(0x0DF1), n, d)
        return Corpus(A, A[tie[1]].copy())
    if name == "mixed":                   # normal rows, tiny rows whose inflated cosines (> 1) belong at the top
        _, n, d = key
        rng = np.random.default_rng(0x0DF7)
        A = rng.standard_normal((n, d)).astype(F)
        q = rng.standard_normal(d).astype(F)
        plant = rng.choice(np.arange(8, n), 60, replace=False)
        A[plant] = _corpora.tiny_rows_along(rng, q, 60)
        return Corpus(A, q, info=dict(tiny=np.sort(plant)))
    if name == "tiny":                    # a whole shard scaled to 1e-21: squares underflow
        _, n, d = key
        rng = np.random.default_rng(0x0DF8)
        return Corpus((rng.standard_normal((n, d)) * 1e-21).astype(F), rng.standard_normal(d).astype(F))
    if name == "identical":               # every row the same (test_large_shard_exact_fallback_uses_the_device_wide_select)
        _, n, d = key
        A, q = _corpora.identical_rows(n, d)
        return Corpus(A, q, ties=np.arange(n))
    if name == "dup_tiles":               # one exact copy of a row in each of `tiles` tiles, normal rows around them
        _, n, d, tiles = key
        rng = np.random.default_rng(12)
        A = rng.standard_normal((n, d)).astype(F)
        dup = np.arange(tiles) * TILE + (np.arange(tiles) * 7) % TILE
        A[dup] = A[dup[0]]
        return Corpus(A, A[dup[0]].copy(), ties=dup, info=dict(other=rng.standard_normal(d).astype(F)))
    if name == "crowd_attack":            # test_crowd_list_takes_the_rows_inside_the_margin
        _, n, d, decoys = key
        A, q, k, _, planted, info = ma.build("rows_bf16", COS, n_rows=n, d=d, n_decoys=decoys, bulk_scale=1.0, seed=4711)
        return Corpus(A, q, planted, info=dict(k=k, by_sweep=info["by_sweep"], floor=info["floor"]))
    if name == "nonfinite":               # rows whose dot product with q is +inf, -inf and NaN
        _, seed, n, d = key
        A = oc.synth(seed, 0, n, d, nthreads=8)
        q = np.abs(oc.synth(seed + 1, 0, 1, d)[0]).astype(F) + F(0.1)
        A[70, 7] = np.inf
        A[n - 3, 100] = -np.inf
        A[4000, 5] = np.nan               # (an input NaN, which every arithmetic passes on; the sign of a NaN made by inf - inf is the hardware's choice)
        return Corpus(A, q, info=dict(pinf=70, ninf=n - 3, nan=4000))
    raise KeyError(name)


def build_queries(case, corpus):
    """q first ("a" layout), then synthetic companions; a batch of the attack cases puts q LAST among its 3 % neighbours, as
    tests/test_gpu_margin_attack.py's "b" layouts do."""
    d = corpus.q.size
    if case.corpus[0] in ("attack", "crowd_attack") and case.nq > 1:
        rng = np.random.default_rng(5)
        Q = (corpus.q[None, :] * (1.0 + 0.03 * rng.standard_normal((case.nq, d)))).astype(F)
        Q[case.nq - 1] = corpus.q
        return Q
    if case.corpus[0] == "dup_tiles" and case.nq == 2:
        return np.stack([corpus.q, corpus.info["other"]]).astype(F)
    Q = oc.synth(0x5E1EC7 + case.nq, 0, case.nq, d)
    if case.corpus[0] in ("tiny", "straddle"):
        Q = (Q * F(1e-21)).astype(F)
    Q[0] = corpus.q
    return Q


def attack_query_index(case):
    return case.nq - 1 if case.corpus[0] in ("attack", "crowd_attack") else 0


def build_mask(case, corpus, geo):
    """u64 words of the case's bitmap, or None."""
    if case.mask is None:
        return None
    n = corpus.A.shape[0]
    kind = case.mask[0]
    keep = np.zeros(n, bool)
    if kind == "random":                  # (kind, seed, share): planted rows kept
        keep = np.random.default_rng(case.mask[1]).random(n) < case.mask[2]
        if corpus.planted is not None:
            keep[corpus.planted] = True
        for r in (corpus.info.get(x) for x in ("pinf", "ninf", "nan")):
            if r is not None:
                keep[r] = True
    elif kind == "none":
        pass
    elif kind == "rows":                  # (kind, count): that many rows, spread
        keep[np.linspace(0, n - 1, case.mask[1]).astype(np.int64)] = True
    elif kind == "waves":                 # (kind, waves...): every row of every tile of these scan waves
        for w in case.mask[1:]:
            for t in geo.tiles_of_wave(w):
                keep[t * TILE:(t + 1) * TILE] = True
    elif kind == "few_with":              # (kind, count): the non-finite rows and count ordinary ones
        keep[np.linspace(0, n - 1, case.mask[1]).astype(np.int64)] = True
        for x in ("pinf", "ninf", "nan"):
            keep[corpus.info[x]] = True
    else:
        raise KeyError(kind)
    return oc.mask_from_bool(keep)


def _borders(n, d, sweep, masked, rows):
    g = geometry(n, d, sweep, masked)
    return tuple((r, r // TILE, g.wave_of_row(r)) for r in rows)


# shards: 8193 rows = 129 tiles (n_tiles % 4 == 1), the last tile AND the last scan wave hold one row; 8850 rows = 139 tiles
# (% 4 == 3), 18 rows in the last tile; 270 000 x 128 = 4219 tiles (% 4 == 3, >= 4096: the ring sweep), 48 rows in the last tile,
# two tiles per scan wave (the last wave: one), five per matrix-core workgroup (the last: four).
N129, N139, NBIG, D_SMALL, D_BIG = 8193, 8850, 270_000, 256, 128
ROWS129 = (0, 63, 64, 8191, 8192)
ROWS139 = (0, 63, 64, 8831, 8832, 8849)
ROWSBIG = (0, 63, 127, 128, 319, 320, 269_951, 269_952, 269_999)
B129 = ("borders", 0x5E1E01, N129, D_SMALL, ROWS129)
B139 = ("borders", 0x5E1E03, N139, D_SMALL, ROWS139)
BBIG = ("borders", 0x5E1E05, NBIG, D_BIG, ROWSBIG)
NT, DT = 8192, 256
TIES_WAVES = ("ties", 0x5E1E07, NT, DT, tuple(t * TILE + (11 * t) % TILE for t in range(3, 123, 6)))   # 20 copies, a tile each
TIES_TILE = ("ties", 0x5E1E09, NT, DT, tuple(range(17 * TILE + 5, 17 * TILE + 25)))                  # 20 copies in tile 17
N_NAT1 = 1_050_037          # 16 407 tiles: just over the flat path; ring / masked VALU: tpw 5, matrix cores: 17, VALU sweeps: 22
N_NAT2 = 7 * MAX_SCAN_WAVES * TILE + 1 + 36   # 28 673 tiles: the smallest shard whose ring / masked VALU waves hold 8 tiles (quads)
D_NAT = 128


def _nat_rows(n, sweeps_masked):
    """Planted rows at both ends and at a wave border of every geometry in `sweeps_masked`; the border rows of the first geometry
    are exact copies of one another (ties across the border)."""
    rows = [0, 63, n - 1]
    for sweep, masked in sweeps_masked:
        g = geometry(n, D_NAT, sweep, masked)
        w = g.W // 2
        rows += [(w * g.tpw) * TILE - 1, (w * g.tpw) * TILE] if not g.strided else [(w + 1) * TILE - 1, (w + 1) * TILE]
    return tuple(dict.fromkeys(rows))


NAT1_ROWS = _nat_rows(N_NAT1, (("ring_f32", False), ("mfma_bf16", False), ("valu_f32", True)))
NAT2_ROWS = _nat_rows(N_NAT2, (("ring_f32", False), ("mfma_bf16", False), ("valu_f32", True)))
NAT1 = ("natural", 0x5E1E11, N_NAT1, NAT1_ROWS)
NAT2 = ("natural", 0x5E1E13, N_NAT2, NAT2_ROWS)


def build_natural(key):
    """Synthetic bulk, near-copies of q at the planted rows; rows[3] and rows[4] (a wave border) are exact copies of each other."""
    _, seed, n, rows = key
    c = _synth_with_plants(seed, n, D_NAT, rows)
    c.A[rows[4]] = c.A[rows[3]]
    c.ties = np.array([rows[3], rows[4]], np.int64)
    return c


def _mk(id, corpus, nq, k, metric, mode, sweep, aims, **kw):
    return Case(id, corpus, nq, k, metric, mode, sweep, aims, **kw)


def forced_cases():
    out = []
    add = lambda *a, **kw: out.append(_mk(*a, **kw))  # noqa: E731
    rnd = ("random", 17, 0.3)
    # ---- wave borders, tail quads, partial last waves
    add("b129-valu_bf16", B129, 1, 10, COS, 2, "valu_bf16", "n_tiles % 4 == 1; last wave = one tile = one row; generic gather (tpw 1)",
        gather="generic", borders=_borders(N129, D_SMALL, "valu_bf16", False, ROWS129))
    add("b129-mfma_i8-k100", B129, 8, 100, COS, 1, "mfma_i8", "uint4 tail of the dense gather under the 8-bit margin, n_tiles % 4 == 1 (100 of 129 waves pass)",
        gather="dense", borders=_borders(N129, D_SMALL, "mfma_i8", False, ROWS129))
    add("b129-valu_f32-k100", B129, 2, 100, L2, 0, "valu_f32", "100 of 129 waves pass: dense gather, tail quad of 1",
        gather="dense", borders=_borders(N129, D_SMALL, "valu_f32", False, ROWS129))
    add("b139-valu_i8", B139, 2, 10, L2, 1, "valu_i8", "n_tiles % 4 == 3; last tile of 18 rows", gather="generic",
        borders=_borders(N139, D_SMALL, "valu_i8", False, ROWS139))
    add("b139-mfma_f32-k110", B139, 8, 110, DOT, 0, "mfma_f32", "110 of 139 waves pass: dense gather with a tail quad of 3", gather="dense",
        borders=_borders(N139, D_SMALL, "mfma_f32", False, ROWS139))
    add("b139-valu_f32-bitmap", B139, 1, 10, COS, 0, "valu_f32", "strided numbering j * W + w under a bitmap", mask=rnd, gather="generic",
        borders=_borders(N139, D_SMALL, "valu_f32", True, ROWS139))
    add("big-ring_f32", BBIG, 1, 10, COS, 0, "ring_f32", "two tiles per wave, the last wave holds one (lim = n_tiles)", gather="generic",
        borders=_borders(NBIG, D_BIG, "ring_f32", False, ROWSBIG))
    add("big-valu_i8", BBIG, 1, 10, DOT, 1, "valu_i8", "8-bit margin at all three levels, partial last wave", gather="generic",
        borders=_borders(NBIG, D_BIG, "valu_i8", False, ROWSBIG))
    add("big-valu_i8-k4096", BBIG, 2, 4096, COS, 1, "valu_i8", "k 4096 > 2110 waves: no wave bound, dense gather, tail quad of 3, tile-level pick",
        gather="dense", borders=_borders(NBIG, D_BIG, "valu_i8", False, ROWSBIG))
    add("big-mfma_bf16", BBIG, 8, 10, COS, 2, "mfma_bf16", "five tiles per workgroup, the last holds four; skip bound", gather="generic",
        borders=_borders(NBIG, D_BIG, "mfma_bf16", False, ROWSBIG))
    add("big-mfma_bf16-nq64-k1000", BBIG, 64, 1000, L2, 2, "mfma_bf16", "64 queries; k 1000 > 844 workgroups: every wave passes, dense",
        gather="dense", borders=_borders(NBIG, D_BIG, "mfma_bf16", False, ROWSBIG))
    add("big-valu_f32-bitmap", BBIG, 1, 10, COS, 0, "valu_f32", "strided numbering, W = 2110, tile 4219 of the last slot missing", mask=rnd,
        gather="generic", borders=_borders(NBIG, D_BIG, "valu_f32", True, ROWSBIG))
    add("big-mfma_f32-nq5-bitmap", BBIG, 5, 64, L2, 0, "mfma_f32", "five queries under a bitmap (matrix cores: contiguous ranges)", mask=rnd)
    # ---- fewer valid waves than k; empty and nearly empty bitmaps
    add("few-94-tiles-k100", ("plain", 0x5E1E21, 6000, D_SMALL), 1, 100, COS, 2, "valu_bf16", "vw = 94 < k = 100: Tw stays the NaN key", gather="dense")
    add("few-3-waves-mfma", BBIG, 8, 10, COS, 2, "mfma_bf16", "valid rows in 3 waves (15 tiles > k > 3 waves): bound from the tile list",
        mask=("waves", 0, 422, 843))
    add("few-3-waves-strided", BBIG, 1, 4, COS, 0, "valu_f32", "valid rows in 3 strided waves (6 tiles > k = 4 > 3 waves)", mask=("waves", 0, 1000, 2108))
    add("mask-empty", B139, 1, 10, COS, 2, "valu_bf16", "vw == 0: count 0", mask=("none",))
    add("mask-7-rows-k10", B139, 2, 10, DOT, 1, "valu_i8", "fewer rows than k", mask=("rows", 7))
    # ---- ties
    for m, nm in ((COS, "cos"), (L2, "l2"), (DOT, "dot")):
        add(f"ties-a-wave-each-{nm}", TIES_WAVES, 1, 10, m, 2, "valu_bf16", "20 copies, one per scan wave, the cut inside the run: ties at the k-th wave AND tile maximum",
            tie_len=8, lead=2)
    add("ties-a-wave-each-mfma_i8", TIES_WAVES, 8, 10, COS, 1, "mfma_i8", "the same under the batched sweep's skip bound", tie_len=8, lead=2)
    add("ties-one-tile", TIES_TILE, 2, 10, COS, 1, "valu_i8", "20 copies inside one tile: one wave and one tile hold the whole run", tie_len=8, lead=2)
    add("ties-one-tile-k1", TIES_TILE, 1, 1, L2, 0, "valu_f32", "k = 1", tie_len=0, lead=1)
    # ---- crowds and overflow (>= 2^18 rows: crowd kernels and f32 retry behind the selection)
    add("crowd-inside-margin", ("crowd_attack", CROWD_MIN_ROWS, 128, 200), 1, ma.K, COS, 2, "valu_bf16", "201 rows inside the margin, candidate list of 64: overflow -> crowd list",
        cand_cap=64, rescored_min=201, rescored_max=201, crowd_over=("cand_cap", 64))
    for mode, sw in ((2, "valu_bf16"), (1, "valu_i8")):
        add(f"identical-rows-{sw}", ("identical", 300_000, 128), 1, 10, COS, mode, sw, "the same top key in 4688 tiles: hand-over at > 1024 tiles, neither crowd nor retry can help -> exact fallback",
            fallback=(1, 1), crowd_over=("kListCap", LIST_CAP))
    add("dups-4500-tiles-batch", ("dup_tiles", 300_000, 128, 4500), 2, 5, COS, 2, "valu_bf16", "a query with copies in 4500 tiles (> kBailTiles, > cand_cap) next to a normal one",
        rescored_min=4500, crowd_over=("cand_cap", CAND_CAP))     # (the crowd list takes the 4500 copies: no exact fallback)
    # ---- k / nq / mirror / metric: one row per sweep kind, a small and a large k each
    P = ("plain", 0x5E1E31, 270_000, 256)
    for mode, nq, msk, sw, ks, m in ((0, 1, None, "ring_f32", (1, 1000), COS), (0, 1, rnd, "valu_f32", (64, 4096), L2), (0, 2, None, "valu_f32", (1, 1000), DOT),
                                     (2, 1, None, "valu_bf16", (64, 4096), L2), (1, 2, None, "valu_i8", (1, 1000), COS),
                                     (0, 8, None, "mfma_f32", (64, 1000), COS), (2, 5, None, "mfma_bf16", (1, 4096), DOT), (1, 64, None, "mfma_i8", (64, 1000), COS)):
        for k in ks:
            add(f"kind-{sw}{'-bitmap' if msk else ''}-nq{nq}-k{k}", P, nq, k, m, mode, sw, f"{sw}: k {k}, {nq} queries", mask=msk)
    # ---- the margin under attack: every construction tests/test_gpu_margin_attack.py runs at N = 8192, through the walk
    def attack(name, metric, kw, mode, sweep, nq, masked=False):
        kws = tuple(sorted(kw.items()))
        cid = f"attack-{sweep}-{name}-{'cos l2 dot'.split()[metric]}" + "".join(f"-{a}{b}" for a, b in kws) + f"-nq{nq}" + ("-bitmap" if masked else "")
        add(cid, ("attack", name, metric, kws), nq, ma.K, metric, mode, sweep, "margin_key at the wave, tile and row level under a worst-case rounding error",
            mask=("random", 17, 0.2) if masked else None, rescored_max=ma.N_DECOYS + 1)
    for m in (COS, DOT, L2):
        attack("rows_bf16", m, {}, 2, "valu_bf16", 1)
        attack("rows_i8", m, {}, 1, "valu_i8", 1)
    attack("rows_i8", COS, {}, 1, "valu_i8", 2)
    for m in (COS, DOT):
        attack("query_i8", m, {"planes": 2}, 1, "valu_i8", 1)
        attack("rows_bf16", m, {}, 2, "mfma_bf16", 8)
        attack("query_bf16", m, {}, 2, "mfma_bf16", 8)
        attack("rows_bf16", m, {}, 0, "mfma_f32", 8)
    attack("rows_bf16", L2, {}, 2, "mfma_bf16", 8)
    attack("rows_bf16", L2, {}, 0, "mfma_f32", 8)
    attack("both_i8", COS, {}, 1, "valu_i8", 1)
    attack("rows_i8", COS, {"planes": 1}, 1, "mfma_i8", 8)
    attack("query_i8", COS, {"planes": 1}, 1, "mfma_i8", 8)
    attack("rows_i8", DOT, {}, 1, "mfma_i8", 8)
    attack("query_i8", DOT, {"planes": 2}, 1, "mfma_i8", 8)
    for pos in (63, 64, 8191):
        attack("rows_bf16", COS, {"target_row": pos}, 2, "valu_bf16", 1)
        attack("rows_i8", COS, {"target_row": pos}, 1, "valu_i8", 1)
    attack("rows_bf16", COS, {}, 2, "valu_bf16", 1, masked=True)
    attack("rows_i8", COS, {}, 1, "valu_i8", 1, masked=True)
    # ---- the f32 underflow edge.  The guard of qprep_kernel works from the shard's smallest stored element (docs/exactness.md,
    # "The underflow guard"): on these three shards it fires for EVERY query, the normal companions of `mixed` included, so the sweep
    # that served is the one the mode and batch size name and every query of the call is answered by the exact path: fallback == nq.
    # (The control, a guard that must NOT fire: the kind-* cases on normal rows above, fallback == 0.)
    for cname in ("straddle", "mixed", "tiny"):
        for mode, nq, sw in ((1, 1, "valu_i8"), (2, 8, "mfma_bf16")):
            add(f"underflow-{cname}-{sw}", (cname, 8192, 256), nq, 100, COS, mode, sw, "tiny rows: the underflow guard sends all nq queries to the exact path behind the walk",
                fallback=(nq, nq))
    # ---- non-finite scores among the top k
    NF = ("nonfinite", 0x5E1E41, N139, D_SMALL)
    # A row with an infinite element has |v| = inf, which voids the dot-product margin (docs/exactness.md): every row is within it.
    # Unmasked, 8850 rows overflow the candidate list and this shard is too small for crowd kernels or a retry: the exact fallback
    # answers, fallback == 1.  Under the bitmap all 8 kept rows fit the list and are re-scored as candidates: fallback == 0.
    add("nonfinite-top", NF, 1, 10, DOT, 2, "valu_bf16", "+inf first; |v| = inf voids the margin: list overflow -> exact fallback", fallback=(1, 1))
    add("nonfinite-all-kinds", NF, 1, 10, DOT, 0, "valu_f32", "+inf, finite, -inf, NaN: 8 rows under a bitmap, k 10, all of them candidates",
        mask=("few_with", 5), rescored_min=8, rescored_max=8)
    assert len({c.id for c in out}) == len(out)
    first = {}
    for i, c in enumerate(out):
        first.setdefault(c.corpus, i)
    return sorted(out, key=lambda c: first[c.corpus])     # (stable: the cases of a corpus together, one build of it per run)


def natural_cases():
    out = []

    def add(id, corpus, nq, k, metric, mode, sweep, aims, **kw):
        out.append(_mk(id, corpus, nq, k, metric, mode, sweep, aims, forced=False, **kw))

    rnd = ("random", 29, 0.25)
    b = lambda n, sw, masked, rows: _borders(n, D_NAT, sw, masked, rows)  # noqa: E731
    add("nat1-ring-k257", NAT1, 1, 257, COS, 0, "ring_f32", "generic gather, tpw 5, 3282 waves; k just over the split's 256", gather="generic",
        borders=b(N_NAT1, "ring_f32", False, NAT1_ROWS))
    add("nat1-ring-k256-split", NAT1, 1, 256, COS, 0, "ring_f32", "k 256, one query: the split selection, not the walk", form="split")
    add("nat1-mfma_bf16-nq5-k10", NAT1, 5, 10, COS, 2, "mfma_bf16", "quads gather, tpw 17 (5 lanes a wave, tail quad of 1), 966 waves", gather="quads",
        borders=b(N_NAT1, "mfma_bf16", False, NAT1_ROWS))
    add("nat1-mfma_bf16-nq5-k1000", NAT1, 5, 1000, L2, 2, "mfma_bf16", "k 1000 > 966 waves: every wave passes: dense gather, n_tiles % 4 == 3", gather="dense")
    add("nat1-mfma_bf16-nq64-k10", NAT1, 64, 10, COS, 2, "mfma_bf16", "64 queries, quads gather under the skip bound", gather="quads")
    add("nat1-mfma_f32-nq64-k1000", NAT1, 64, 1000, DOT, 0, "mfma_f32", "64 queries, dense gather", gather="dense")
    add("nat1-valu_f32-bitmap-k257", NAT1, 1, 257, COS, 0, "valu_f32", "strided numbering j * 3282 + w, tpw 5; the last slot of most waves is past n_tiles",
        mask=rnd, gather="generic", borders=b(N_NAT1, "valu_f32", True, NAT1_ROWS))
    add("nat1-valu_i8-nq2-k1000", NAT1, 2, 1000, COS, 1, "valu_i8", "VALU sweep on 768 waves: tpw 22, 746 waves < k: dense", gather="dense")
    add("nat2-ring-k257", NAT2, 1, 257, COS, 0, "ring_f32", "quads gather at its smallest: tpw 8 (two lanes a wave), the last wave holds one tile", gather="quads",
        borders=b(N_NAT2, "ring_f32", False, NAT2_ROWS))
    add("nat2-mfma_bf16-nq5-k10", NAT2, 5, 10, COS, 2, "mfma_bf16", "quads gather, tpw 29 (8 lanes a wave, tail quad of 1), 989 waves", gather="quads",
        borders=b(N_NAT2, "mfma_bf16", False, NAT2_ROWS))
    add("nat2-mfma_f32-nq8-k1000", NAT2, 8, 1000, L2, 0, "mfma_f32", "k 1000 > 989 waves: dense gather, n_tiles % 4 == 1", gather="dense")
    add("nat2-valu_f32-bitmap-k300", NAT2, 2, 300, L2, 0, "valu_f32", "strided numbering with tpw 8: strided never takes the quads gather", mask=rnd, gather="generic",
        borders=b(N_NAT2, "valu_f32", True, NAT2_ROWS))
    return out


def case_geometry(case, n, d):
    return geometry(n, d, case.sweep, case.mask is not None) if case.sweep else None


def gather_share_ok(case, share):
    if case.gather == "dense":
        return share >= 0.7
    if case.gather in ("quads", "generic"):
        return share <= 0.3
    return True


def gather_kind(geo, share):
    """The gather the kernel takes for a share on one side of 0.5 (tmax rows are 16-byte aligned in every workspace)."""
    if share >= 0.5:
        return "dense"
    return "quads" if (not geo.strided and geo.tpw >= 8) else "generic"


def oracle_answers(case, corpus, Q, mask):
    return [oc.search(corpus.A, Q[i], case.k, case.metric, mask=mask, nthreads=8, partial=True, native=True) for i in range(Q.shape[0])]
