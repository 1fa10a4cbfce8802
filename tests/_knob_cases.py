"""The table behind tests/test_gpu_knobs.py and tests/test_knob_table_cpu.py: every documented NMN_* switch and geometry knob
(README.md, "Measurement knobs") held to the oracle.  numpy and the oracles only — nothing here touches the GPU.

A PROFILE is an environment and a list of case ids; tests/_knob_worker.py runs one profile per fresh process (nearly every switch
is read once per process).  A CASE is a corpus, a mirror mode, a query batch, k, a metric, a bitmap density, the API entry it goes
through and cand_cap.  The baseline profiles (empty environment) run the same cases in the same worker: they show that the harness
agrees with the oracle and supply the stats the other profiles are compared with (Profile.effects).  OUT_OF_SCOPE maps every
documented name that no profile sets to one sentence of reason.

Grouping (the issue's list, adjusted where the dispatch code says so):
  * NMN_NO_ZERO_COPY and NMN_NO_POLL are TWO children: host_batch_body polls only on the zero-copy block (`poll = zero_copy && ...`),
    so NMN_NO_ZERO_COPY makes NMN_NO_POLL moot for every case.
  * NMN_RING_WGS and NMN_SCAN_WAVES_SMALL cannot reach "fewer units of work than the knob asks for" or "exactly one wave": the
    ring sweep exists from 4096 tiles on and the small-wave band from 128 MiB of sweep on, both far above the knobs' 64 / 256.
    Their cases claim the short last wave only (FULL_CLAIM_KNOBS names the two knobs that cover all three claims).
  * NMN_IVF_NO_LIST_MAJOR needs at least 4096 vectors (ivf_relayout): the issue's 2 000 x 32 corpus never has the list-major copy,
    so a 5 000 x 32 corpus runs beside it.
  * NMN_NO_SAMPLE alone leaves sweep_launches of an unmasked batch at the baseline's 1 (the running bound replaced the sampling
    pass there, and NMN_NO_SAMPLE switches both off): the masked 2^21 case shows it, 3 -> 1."""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import ivf_oracle as io
from oracle import oracle_c as oc
from tests import _select_walk_cases as sw

F = np.float32
COS, L2, DOT = 0, 1, 2
TILE = 64
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)
METRIC_NAMES = {COS: "cos", L2: "l2", DOT: "dot"}


@dataclass(frozen=True)
class Case:
    id: str
    corpus: tuple               # key of a recipe in tests/_select_walk_cases.build_corpus() (flat APIs), or of ivf_setup / engine_setup
    nq: int
    k: int
    metric: int
    mode: int = 1               # set_mirror: 0 f32 rows, 1 smallest mirror, 2 bf16 (set before the rows arrive)
    mask: float = None          # share of the rows a bitmap keeps (None: no bitmap)
    api: str = "search"         # search | pred | threads | engine | ivf
    cand_cap: int = 0
    single_launch: bool = False  # True: the shard may take tiny_search_kernel (NMN_NO_TINY's cases)
    threads: int = 0            # pred / threads: concurrent callers inside the one child (0: one call after another)
    nprobe: int = None          # ivf
    geom: tuple = ()            # ((knob, value, claim), ...): what the launch arithmetic must yield (test_knob_table_cpu.py)
    family: str = None          # "valu" / "mfma" / "ring": the sweep family a geometry claim is about


@dataclass(frozen=True)
class Profile:
    name: str
    env: dict
    cases: tuple                # case ids, in the order the worker runs them
    base: str = None            # the baseline profile that runs the same cases (None: this IS a baseline)
    effects: tuple = ()         # ((case id, field, baseline value, value under this profile), ...): field of the worker's line —
                                #   "sweep", "sweep_launches", "fallback_queries", "aux.<name>"; a value may be ("prefix", "valu_"),
                                #   ("ne", x), ("ge", n), ("differs",) = not the baseline's, or a plain value (equality)
    by_arithmetic: tuple = ()   # knobs of this profile whose effect no counter shows: the child's environment + launch arithmetic
    why: str = ""


# ---------------------------------------------------------------------------------------------- launch arithmetic
def launch_arithmetic(rows, knob):
    """search_enqueue (nmn_api.hip) restated: n_tiles = ceil(rows / 64), tiles_per_wave = max(1, ceil(n_tiles / knob)),
    waves = ceil(n_tiles / tiles_per_wave).  -> (n_tiles, tiles_per_wave, waves, tiles of the last wave)"""
    n_tiles = -(-rows // TILE)
    tpw = max(1, -(-n_tiles // knob))
    waves = -(-n_tiles // tpw)
    return n_tiles, tpw, waves, n_tiles - (waves - 1) * tpw


def claim_holds(claim, rows, knob):
    n_tiles, tpw, waves, last = launch_arithmetic(rows, knob)
    if claim == "short_last":       # at least 2 tiles per wave, the last wave shorter
        return tpw >= 2 and waves >= 2 and 0 < last < tpw
    if claim == "fewer":            # fewer units of work than the knob asks for: several waves of one tile, the rest of the grid idle
        return 1 < n_tiles < knob and tpw == 1 and waves == n_tiles
    if claim == "one":              # exactly one wave
        return waves == 1
    raise KeyError(claim)


CLAIMS = ("short_last", "fewer", "one")
FULL_CLAIM_KNOBS = ("NMN_SCAN_WAVES", "NMN_MFMA_WGS")                 # their cases cover all three claims
SHORT_LAST_ONLY_KNOBS = ("NMN_RING_WGS", "NMN_SCAN_WAVES_SMALL")      # (module docstring: the other two are out of reach)


# ---------------------------------------------------------------------------------------------- corpora, queries, bitmaps
def plain(n, d):
    return ("plain", 0x4B0B00 + 131 * n + d, n, d)


# 4100 tiles: the ring sweep (>= 4096 tiles); ceil(4100 / 64) = 65 tiles per ring group, the last of 64 groups holds 5;
# ceil(4100 / 256) = 17 tiles per wave of the small-wave band, the last of 242 waves holds 3; 262 341 x 128 x 4 B = 128.1 MiB: inside the band
N18 = 4099 * TILE + 5
B18 = plain(N18, 128)
DUPS18 = ("dup_tiles", 1 << 18, 128, 300)     # one exact copy of a row in each of 300 tiles: > cand_cap 64, within the crowd list
SAME18 = ("identical", 1 << 18, 128)          # every row ties: neither crowd list nor retry can help -> exact fallback
N21 = 1 << 21                                 # 32 768 tiles: the smallest shard with the sampled bound (and the in-sweep running bound)
B21 = plain(N21, 128)


def build_corpus(case):
    return sw.build_corpus(case.corpus)


def build_queries(case, corpus):
    return sw.build_queries(case, corpus)


def build_keep(case, n):
    """bool[n]: the rows the case's bitmap keeps (None: no bitmap)."""
    if case.mask is None:
        return None
    return np.random.default_rng(0xB17 + n).random(n) < case.mask


def build_mask(case, n):
    keep = build_keep(case, n)
    return None if keep is None else oc.mask_from_bool(keep)


# ---- predicates (the bitmap oracle of tests/test_gpu_filter.py: integer columns, the selection restated in numpy)
def pred_columns(n):
    """-> (bucket, price): the two integer columns of test_search_pred_one_call_equals_eval_then_search."""
    return np.arange(n) % 13, (np.arange(n) * 7919) % 1000


def pred_programs(n, count):
    """count programs as neutral postfix tuples (op, column, value) and the rows each keeps.  Columns: 0 bucket, 1 price."""
    bucket, price = pred_columns(n)
    out = []
    for j in range(count):
        if j % 4 == 0:
            out.append(((("eq", 0, j % 13),), bucket == j % 13))
        elif j % 4 == 1:
            t = 50 + 20 * j
            out.append(((("lt", 1, t),), price < t))
        elif j % 4 == 2:
            out.append(((("eq", 0, j % 13), ("ge", 1, 300), ("and",)), (bucket == j % 13) & (price >= 300)))
        else:
            out.append(((("gt", 1, 5000),), np.zeros(n, bool)))
    return out


# ---- IVF (oracle/ivf_oracle.py): 2 000 x 32, 16 lists
IVF_FAST = dict(max_iterations=2, convergence_threshold=1.0, seed=42, init_method="random")


@functools.lru_cache(maxsize=2)
def ivf_setup(key):
    """-> (oracle index trained on the first 600 vectors, NOTHING added yet; vectors; queries)"""
    _, seed, n, d, lists = key
    V = oc.synth(seed, 0, n, d)
    V[11] = V[5]                        # duplicates: same list, id order
    V[n - 1] = V[5]
    orc = io.IVFFlat(lists, nprobe=None, kmeans=io.KMeansConfig(**IVF_FAST))
    orc.train(V[:600])
    Q = oc.synth(seed + 1, 0, 8, d)
    Q[0] = V[5]
    return orc, V, Q


@functools.lru_cache(maxsize=2)
def ivf_filled(key):
    orc, V, Q = ivf_setup(key)
    for v in V:
        orc.add(v)
    return orc, V, Q


IVF = ("ivf", 0x4B0F01, 2000, 32, 16)
IVF5 = ("ivf", 0x4B0F05, 5000, 32, 16)    # ivf_relayout builds the list-major copy from 4096 vectors on: NMN_IVF_NO_LIST_MAJOR is moot below


# ---- engine: one collection of 3 000 x 300 (stride 304 tight, 384 wide)
@functools.lru_cache(maxsize=1)
def engine_setup(key):
    _, seed, n, d = key
    return oc.synth(seed, 0, n, d), oc.synth(seed + 1, 0, 4, d)


ENG = ("engine", 0x4B0E01, 3000, 300)


# ---------------------------------------------------------------------------------------------- cases
def _small_cases():
    out = []

    def add(n, d, mode, nq, k, metric, mask=None, geom=(), family=None):
        cid = f"s-{n}x{d}-m{mode}-nq{nq}-k{k}-{METRIC_NAMES[metric]}" + (f"-mask{mask}" if mask else "")
        out.append(Case(cid, plain(n, d), nq, k, metric, mode=mode, mask=mask, geom=geom, family=family))

    W, M = "NMN_SCAN_WAVES", "NMN_MFMA_WGS"
    add(1, 8, 2, 1, 1, COS)
    add(1, 128, 1, 5, 10, DOT)
    add(63, 100, 2, 2, 100, L2)
    add(63, 768, 0, 1, 10, COS, geom=((W, 256, "one"),), family="valu")
    add(63, 128, 2, 17, 10, COS, geom=((M, 64, "one"),), family="mfma")
    add(65, 128, 1, 1, 10, L2)
    add(65, 768, 1, 5, 1, COS)
    add(1000, 768, 1, 2, 10, COS)
    add(1000, 768, 1, 17, 10, COS)
    add(1000, 128, 2, 65, 100, DOT, geom=((M, 64, "fewer"),), family="mfma")
    add(1000, 100, 0, 5, 10, L2, mask=0.3)
    add(1000, 128, 1, 1, 10, DOT, mask=0.02)
    add(4097, 128, 1, 1, 10, COS, geom=((W, 256, "fewer"),), family="valu")
    add(4097, 128, 1, 2, 100, L2, mask=0.3)
    add(4097, 768, 1, 17, 10, COS, geom=((M, 64, "short_last"),), family="mfma")
    add(4097, 768, 1, 5, 10, L2, mask=0.3)
    add(4097, 768, 2, 1, 10, COS)
    add(16400, 128, 0, 2, 10, DOT, geom=((W, 256, "short_last"),), family="valu")
    add(16400, 768, 0, 1, 100, L2, mask=0.3)
    add(16400, 128, 2, 65, 10, COS)
    add(20011, 768, 0, 1, 10, COS, geom=((W, 256, "short_last"),), family="valu")
    add(20011, 768, 2, 2, 10, DOT)
    add(20011, 768, 1, 1, 100, COS, mask=0.02)
    add(20011, 768, 1, 17, 100, L2, geom=((M, 64, "short_last"),), family="mfma")
    add(20011, 768, 0, 5, 10, COS)
    add(20011, 768, 2, 65, 1, DOT, mask=0.3)
    add(20011, 768, 1, 3, 10, COS)
    add(20011, 768, 1, 65, 10, COS)      # more than 64 queries on the 8-bit matrix-core sweep: NMN_MFMA_I8_NO_128's case
    add(20011, 128, 1, 5, 10, COS)
    add(20011, 128, 1, 2, 10, DOT)
    add(20011, 100, 2, 17, 10, L2)
    add(20011, 8, 0, 65, 100, COS, mask=0.3)
    return out


SMALL = _small_cases()

TINY = [
    Case("t-63x100-k100-dot", plain(63, 100), 1, 100, DOT, single_launch=True),
    Case("t-1000x128-k10-cos", plain(1000, 128), 1, 10, COS, single_launch=True),
    Case("t-20011x768-k100-l2", plain(20011, 768), 1, 100, L2, single_launch=True),
]
PRED = [   # row counts that are no multiple of 256; several programs per batch where threads > 0
    Case("p-1000x128-alone", plain(1000, 128), 4, 30, COS, api="pred"),
    Case("p-20011x768-threads8", plain(20011, 768), 8, 30, COS, api="pred", threads=8),
    Case("p-4097x100-threads8", plain(4097, 100), 8, 30, L2, api="pred", threads=8),
]
ENGINE = [Case("e-3000x300-k10-cos", ENG, 4, 10, COS, api="engine")]
THREADS = [
    Case("h-20011x768-m1-threads8", plain(20011, 768), 8, 10, COS, mode=1, api="threads", threads=8),
    Case("h-4097x128-m2-threads8", plain(4097, 128), 8, 10, DOT, mode=2, api="threads", threads=8),
]
IVF_CASES = [
    Case("i-2000x32-nq1-k10", IVF, 1, 10, L2, api="ivf"),
    Case("i-2000x32-nq8-k10", IVF, 8, 10, L2, api="ivf"),
    Case("i-2000x32-nq1-k50-all-lists", IVF, 1, 50, L2, api="ivf", nprobe=16),
    Case("i-5000x32-nq1-k10", IVF5, 1, 10, L2, api="ivf"),
    Case("i-5000x32-nq8-k10", IVF5, 8, 10, L2, api="ivf"),
]
R, S = "NMN_RING_WGS", "NMN_SCAN_WAVES_SMALL"
BIG18 = [
    Case("b-ring-f32", B18, 1, 10, COS, mode=0, geom=((R, 64, "short_last"),), family="ring"),
    Case("b-valu-f32-nq2", B18, 2, 10, L2, mode=0, geom=((S, 256, "short_last"),), family="valu"),
    Case("b-valu-i8-nq1", B18, 1, 10, COS, mode=1),
    Case("b-valu-bf16-nq2-k100", B18, 2, 100, DOT, mode=2),
    Case("b-mfma-bf16-nq8", B18, 8, 10, COS, mode=2),
    Case("b-valu-f32-mask0.3", B18, 1, 10, COS, mode=0, mask=0.3),
    Case("b-valu-i8-mask0.3", B18, 1, 10, DOT, mode=1, mask=0.3),
    Case("b-k5000", B18, 1, 5000, COS, mode=2),
]
CROWD18 = [
    Case("c-dups-capped", DUPS18, 2, 5, COS, mode=2, cand_cap=64),
    Case("c-identical", SAME18, 1, 10, COS, mode=2),
]
BIG21 = [
    Case("g-mfma-bf16-nq8", B21, 8, 10, COS, mode=2),
    Case("g-mfma-bf16-nq8-mask0.3", B21, 8, 10, COS, mode=2, mask=0.3),
    Case("g-mfma-f32-nq8-k100", B21, 8, 100, L2, mode=0),
]
ALL_CASES = SMALL + TINY + PRED + ENGINE + THREADS + IVF_CASES + BIG18 + CROWD18 + BIG21
CASES = {c.id: c for c in ALL_CASES}
assert len(CASES) == len(ALL_CASES)


def _ids(cases):
    return tuple(c.id for c in cases)


def _sid(n, d, mode, nq, k, metric, mask=None):
    cid = f"s-{n}x{d}-m{mode}-nq{nq}-k{k}-{METRIC_NAMES[metric]}" + (f"-mask{mask}" if mask else "")
    assert cid in CASES, cid
    return cid


# ---------------------------------------------------------------------------------------------- profiles
SMALL_IDS, PIPE_IDS, HOST_IDS, IVF_IDS = _ids(SMALL), _ids(TINY + PRED + ENGINE), _ids(THREADS), _ids(IVF_CASES)
B18_IDS, C18_IDS, B21_IDS = _ids(BIG18), _ids(CROWD18), _ids(BIG21)

PROFILES = [
    # ---- baselines: the empty environment, the same worker
    Profile("base-small", {}, SMALL_IDS), Profile("base-pipe", {}, PIPE_IDS), Profile("base-host", {}, HOST_IDS),
    Profile("base-ivf", {}, IVF_IDS), Profile("base-18", {}, B18_IDS + C18_IDS), Profile("base-21", {}, B21_IDS),
    # ---- small shards
    Profile("geometry-min", {"NMN_SCAN_WAVES": "256", "NMN_MFMA_WGS": "64", "NMN_SCAN_NT": "0"}, SMALL_IDS, "base-small",
            by_arithmetic=("NMN_SCAN_WAVES", "NMN_MFMA_WGS", "NMN_SCAN_NT"),
            why="the knobs' lower limits: several tiles per wave, the short last wave, idle waves, one wave; NT=false at 768-element rows"),
    Profile("mfma-forms", {"NMN_MFMA_NO_FOLD": "1", "NMN_MFMA_I8_NO_128": "1", "NMN_MFMA_WAVES": "8"}, SMALL_IDS, "base-small",
            by_arithmetic=("NMN_MFMA_NO_FOLD", "NMN_MFMA_I8_NO_128", "NMN_MFMA_WAVES"),
            why="the unfolded grid, the other 8-bit form and the 8-wave workgroup (dim 768) of the matrix-core sweep"),
    Profile("valu", {"NMN_NO_MFMA": "1", "NMN_NO_WALK": "1"}, SMALL_IDS, "base-small",
            effects=((_sid(20011, 768, 0, 5, 10, COS), "sweep", "mfma_f32", "valu_f32"),
                     (_sid(20011, 768, 1, 17, 100, L2), "sweep", "mfma_i8", ("prefix", "valu_")),
                     (_sid(20011, 768, 2, 65, 1, DOT, 0.3), "sweep", "mfma_bf16", "valu_bf16")),
            by_arithmetic=("NMN_NO_WALK",), why="batches of up to 65 on the VALU sweeps of four; masked 8-bit sweeps tile by tile"),
    Profile("mfma-min-nq", {"NMN_MFMA_MIN_NQ": "1"}, SMALL_IDS, "base-small",
            effects=((_sid(20011, 768, 0, 1, 10, COS), "sweep", "valu_f32", "mfma_f32"),
                     (_sid(20011, 768, 2, 2, 10, DOT), "sweep", "valu_bf16", "mfma_bf16")),
            why="the matrix-core sweep with one and two queries"),
    Profile("tiny-i8", {"NMN_I8_MIN_ROWS": "1", "NMN_I8_TWO_PLANES": "1", "NMN_I8_MIN_ODD_LD": "256"}, SMALL_IDS, "base-small",
            effects=((_sid(1000, 768, 1, 2, 10, COS), "sweep", "valu_bf16", "valu_i8"),
                     (_sid(1000, 768, 1, 17, 10, COS), "sweep", "mfma_bf16", "mfma_i8"),
                     (_sid(4097, 128, 1, 1, 10, COS), "sweep", "valu_i8", "valu_bf16")),   # (NMN_I8_MIN_ODD_LD: 128 is one half)
            by_arithmetic=("NMN_I8_TWO_PLANES",), why="the 8-bit mirror on shards of 1 .. 4095 rows; both query planes; odd strides off"),
    Profile("route-no-i8-mfma", {"NMN_NO_I8_MFMA": "1"}, SMALL_IDS, "base-small",
            effects=((_sid(20011, 768, 1, 17, 100, L2), "sweep", "mfma_i8", "mfma_bf16"),
                     (_sid(20011, 768, 1, 1, 100, COS, 0.02), "sweep", "valu_i8", "valu_i8")),
            why="batches stay on the bf16 mirror, single queries keep the 8-bit one"),
    Profile("route-masked-half", {"NMN_NO_I8_MASKED_MFMA": "1", "NMN_NO_HALF": "1"}, SMALL_IDS, "base-small",
            effects=((_sid(4097, 768, 1, 5, 10, L2, 0.3), "sweep", "mfma_i8", "mfma_bf16"),
                     (_sid(4097, 768, 1, 17, 10, COS), "sweep", "mfma_i8", "mfma_i8"),
                     (_sid(4097, 768, 2, 1, 10, COS), "sweep", "valu_bf16", "valu_f32")),
            why="bitmap batches on the bf16 mirror, unmasked ones unchanged; 1-2 query sweeps over the f32 rows"),
    Profile("route-no-i8", {"NMN_NO_I8": "1"}, SMALL_IDS, "base-small",
            effects=((_sid(20011, 768, 1, 17, 100, L2), "sweep", "mfma_i8", "mfma_bf16"),
                     (_sid(4097, 128, 1, 1, 10, COS), "sweep", "valu_i8", "valu_bf16")),
            why="never the 8-bit mirror"),
    Profile("pipeline", {"NMN_NO_TINY": "1", "NMN_PRED_TICKET": "1", "NMN_ENGINE_TIGHT_ROWS": "1"}, PIPE_IDS, "base-pipe",
            effects=(("t-1000x128-k10-cos", "sweep", "exact", ("prefix", "valu_")),
                     ("t-20011x768-k100-l2", "sweep", "exact", ("prefix", "valu_"))),
            by_arithmetic=("NMN_PRED_TICKET", "NMN_ENGINE_TIGHT_ROWS"),
            why="small shards through the general pipeline; the predicate count by the last block's ticket; engine rows at stride 304"),
    Profile("host-copy", {"NMN_NO_ZERO_COPY": "1"}, SMALL_IDS, "base-small", by_arithmetic=("NMN_NO_ZERO_COPY",),
            why="staged H2D / D2H copies around the chain"),
    Profile("host-sync", {"NMN_NO_POLL": "1"}, SMALL_IDS, "base-small", by_arithmetic=("NMN_NO_POLL",),
            why="hipStreamSynchronize instead of the polled done word (polling needs the zero-copy block: a child of its own)"),
    Profile("host-no-coalesce", {"NMN_NO_COALESCE": "1"}, HOST_IDS, "base-host",
            effects=(("h-20011x768-m1-threads8", "aux.merged_calls", ("ge", 0), 0),),
            why="eight concurrent callers, one sweep each"),
    Profile("host-inflight", {"NMN_HOST_INFLIGHT": "1", "NMN_GATHER_US": "0"}, HOST_IDS, "base-host",
            by_arithmetic=("NMN_HOST_INFLIGHT", "NMN_GATHER_US"), why="eight concurrent callers behind ONE batch in flight, no gather window"),
    Profile("ivf-bitmap", {"NMN_IVF_NO_LIST_MAJOR": "1"}, IVF_IDS, "base-ivf",
            effects=(("i-5000x32-nq1-k10", "aux.list_major_rows", 5000, 0), ("i-2000x32-nq1-k10", "aux.list_major_rows", 0, 0)),
            why="every probe through the per-row bitmap (the list-major copy exists from 4096 vectors on: the 5 000-vector cases)"),
    Profile("ivf-host-scans", {"NMN_IVF_NO_BATCHED_SCANS": "1", "NMN_IVF_NO_DIRECT": "1"}, IVF_IDS, "base-ivf",
            by_arithmetic=("NMN_IVF_NO_BATCHED_SCANS", "NMN_IVF_NO_DIRECT"),
            why="list scans of 8 queries one by one; a lone query's scans through the host path"),
    # ---- shards of 2^18 rows
    Profile("fused-tail", {"NMN_FUSED_TAIL": "1"}, B18_IDS + C18_IDS, "base-18", by_arithmetic=("NMN_FUSED_TAIL",),
            why="rescore_final_kernel ends the short chain; a flagged query is still followed up by the whole chain"),
    Profile("long-chain", {"NMN_NO_SHORT_CHAIN": "1", "NMN_NO_EXACT_ROWS": "1", "NMN_NO_GRID_SELECT": "1"}, B18_IDS + C18_IDS, "base-18",
            effects=(("c-identical", "fallback_queries", 1, 1),),
            by_arithmetic=("NMN_NO_SHORT_CHAIN", "NMN_NO_EXACT_ROWS", "NMN_NO_GRID_SELECT"),
            why="the 11-launch chain at once; exact scores by eight lanes per row (fallback and k > 4096); the one-workgroup fallback select"),
    Profile("no-crowd", {"NMN_NO_CROWD": "1"}, C18_IDS, "base-18",
            effects=(("c-dups-capped", "fallback_queries", 0, ("ge", 1)), ("c-dups-capped", "candidates_rescored", ("ge", 300), ("differs",))),
            why="an overflowing list goes to the f32 retry and the exact fallback instead of the crowd list"),
    Profile("ring-geometry", {"NMN_RING_WGS": "64", "NMN_SCAN_WAVES_SMALL": "256"}, B18_IDS, "base-18",
            effects=(("b-ring-f32", "sweep", "ring_f32", "ring_f32"), ("b-valu-f32-nq2", "sweep", "valu_f32", "valu_f32")),
            by_arithmetic=("NMN_RING_WGS", "NMN_SCAN_WAVES_SMALL"), why="64 ring groups of 65 tiles (the last: 5); 242 waves of 17 tiles (the last: 3)"),
    Profile("no-ring", {"NMN_NO_RING": "1", "NMN_SCAN_WAVES_SMALL": "0"}, B18_IDS, "base-18",
            effects=(("b-ring-f32", "sweep", "ring_f32", "valu_f32"),), by_arithmetic=("NMN_SCAN_WAVES_SMALL",),
            why="one unmasked f32 query on scan_kernel, on the full grid"),
    Profile("wgs-per-cu", {"NMN_SCAN_I8_WGS_PER_CU": "2", "NMN_SCAN_WGS_PER_CU": "0"}, ("b-valu-f32-mask0.3", "b-valu-i8-mask0.3"), "base-18",
            by_arithmetic=("NMN_SCAN_I8_WGS_PER_CU", "NMN_SCAN_WGS_PER_CU"), why="the residency limit of masked sweeps: off for f32 rows, on for the 8-bit mirror"),
    # ---- one shard of 2^21 x 128, batches of 8
    Profile("sample-reread", {"NMN_NO_RUN_BOUND": "1", "NMN_SAMPLE_REREAD": "1", "NMN_REFINE_MIN_NQ": "3"}, B21_IDS, "base-21",
            effects=(("g-mfma-bf16-nq8", "sweep_launches", 1, 5), ("g-mfma-bf16-nq8-mask0.3", "sweep_launches", 3, 5),
                     ("g-mfma-f32-nq8-k100", "sweep_launches", 1, 5)),
            by_arithmetic=("NMN_SAMPLE_REREAD",), why="sampling pass (tile maxima only) + bound + two-launch refinement from 3 queries on"),
    Profile("no-refine", {"NMN_NO_RUN_BOUND": "1", "NMN_NO_REFINE": "1", "NMN_SAMPLE_AHEAD_OF_CHAIN": "1"}, B21_IDS, "base-21",
            effects=(("g-mfma-bf16-nq8", "sweep_launches", 1, 3), ("g-mfma-f32-nq8-k100", "sweep_launches", 1, 3)),
            by_arithmetic=("NMN_SAMPLE_AHEAD_OF_CHAIN",), why="sampling pass ahead of the chain's wait, one main launch"),
    Profile("no-sample", {"NMN_NO_SAMPLE": "1"}, B21_IDS, "base-21",
            effects=(("g-mfma-bf16-nq8", "sweep_launches", 1, 1), ("g-mfma-bf16-nq8-mask0.3", "sweep_launches", 3, 1)),
            why="no sampling pass and no running bound: the batched sweep writes every tile's scores"),
]
PROFILE = {p.name: p for p in PROFILES}
assert len(PROFILE) == len(PROFILES)
BASELINES = [p for p in PROFILES if p.base is None]
KNOB_PROFILES = [p for p in PROFILES if p.base is not None]

# ---------------------------------------------------------------------------------------------- what no profile sets
OUT_OF_SCOPE = {
    "NMN_SAMPLE_STEP": "needs at least 4M rows before a coarser sample still has 1024 tiles",
    "NMN_NO_SWEEP_CHAIN": "the sweep chain exists for sweeps of at least 2 GiB",
    "NMN_RUN_BOUND_DEBUG": "measurement only: parts of the running-bound machinery off",
    "NMN_MEASURE_DEVICE_SHORT_CHAIN": "measurement only: an overflowed query comes back with count 0xFFFFFFFF by design",
    "NMN_MIRROR_RESERVE_MB": "decides whether a mirror is built from the device's free memory, which a shared GPU does not pin down",
    "NMN_TRACE_MIRROR": "prints the build-or-decline decisions, selects no code that computes",
    "NMN_RCCL_NARROW_LOCK": "needs several devices",
    "NMN_BENCH_CPU_SAMPLE": "read by bench.py, not by the library: how the CPU baseline of the benchmark is timed",
    "NMN_TT_DECOMPOSE_HOST_THREADS": "thread count of the host restatement, whose answers tests/test_tt_decompose_cpu.py holds to the oracle at the default",
    # knobs an existing test already sets
    "NMN_FB_TIMEOUT_TICKS": "tests/test_gpu_edge_cases.py::test_fallback_select_timeout_falls_back_to_one_workgroup",
    "NMN_WS_TEST_MAX_NQ": "tests/test_gpu_edge_cases.py (the shrunk query pass)",
    "NMN_NO_INGEST": "tests/test_gpu_write_paths.py",
    "NMN_NO_F32_MFMA": "tests/test_gpu_batched.py",
    "NMN_NO_SPLIT_SELECT": "tests/test_gpu_select_walk.py",
    "NMN_NO_FLAT_SELECT": "tests/test_gpu_select_walk.py (its worker process)",
    "NMN_NO_RING_EVEN": "tests/test_gpu_ring_even.py",
    "NMN_RING_MAIN": "tests/test_gpu_ring_even.py",
    "NMN_RING_TAIL": "tests/test_gpu_ring_even.py",
    "NMN_SHARDED_CREW": "tests/test_gpu_sharded_handle.py",
    "NMN_XMETRIC_SORT_FROM": "tests/test_gpu_xmetric.py",
    "NMN_HNSW_HOST_SEARCH": "tests/test_gpu_hnsw.py and the other HNSW modules",
    "NMN_HNSW_NO_COALESCE": "tests/test_gpu_hnsw_coalesce.py",
    "NMN_HNSW_BULK_BUILD": "tests/test_gpu_hnsw_bulk.py",
    "NMN_TT_DECOMPOSE_MIN": "tests/test_gpu_tt_decompose.py",
    "NMN_TT_DECOMPOSE_THREADS": "tests/test_gpu_tt_decompose.py",
    "NMN_TT_DECOMPOSE_GRID": "tests/test_gpu_tt_decompose.py",
    "NMN_TT_SIMILARITY_MIN": "tests/test_gpu_tt_similarity.py",
    "NMN_TT_SIMILARITY_HOST_THREADS": "tests/test_tt_similarity_cpu.py",
    "NMN_TT_SIMILARITY_GRID": "tests/test_gpu_tt_similarity.py",
}


def knobs_set_by_profiles():
    return {name for p in PROFILES for name in p.env}


# ---------------------------------------------------------------------------------------------- the oracle's answers
def oracle_answer(case):
    """-> list of (rows u64[c], score bits u32[c]) per query / program / thread, in the order of the worker's line; the tail value
    of the API (-inf for similarity searches, +inf for IVF distances) is the caller's business."""
    if case.api == "ivf":
        orc, _, Q = ivf_filled(case.corpus)
        out = []
        for i in range(case.nq):
            ids, dist = orc.search(Q[i], case.k, case.nprobe)
            out.append((np.asarray(ids, np.uint64), np.asarray(dist, F).view(np.uint32)))
        return out
    if case.api == "engine":
        A, Q = engine_setup(case.corpus)
        return [_flat(A, Q[i], case, None) for i in range(case.nq)]
    corpus = build_corpus(case)
    Q = build_queries(case, corpus)
    n = corpus.A.shape[0]
    if case.api == "pred":
        return [_flat(corpus.A, Q[j], case, oc.mask_from_bool(keep)) if keep.any() else (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
                for j, (_, keep) in enumerate(pred_programs(n, case.nq))]
    mask = build_mask(case, n)
    return [_flat(corpus.A, Q[i], case, mask) for i in range(case.nq)]


def _flat(A, q, case, mask):
    er, es = oc.search(A, q, case.k, case.metric, mask=mask, nthreads=8, partial=True, native=True)
    return er, es.view(np.uint32)
