"""Reader and writer of the HNSW index file, version 1 — TEST INFRASTRUCTURE ONLY.

Written from docs/hnsw.md §10 alone, independently of the product (neumann_amd/csrc/nmn_hnsw.hip).  The writer checks nothing:
it writes whatever the HnswFile object holds, which is how the refusal tests craft files that break one rule each.

  header   64 bytes: magic "NMNIDX\\0\\1", u32 version, kind, dim, flags, u64 rows, row_base, payload_bytes, aux, reserved
  graph    48 bytes of config | u64 rng | u64 entry_point | u32 max_layer | u32 n_upper | n x u8 levels (zero-padded to 4) |
           n x u32 layer-0 counts | the layer-0 ids | for every node of level >= 1, for layer 1 .. level: u32 count, ids
  rows     dense: a flat section (its own 64-byte header, rows x dim f32, rows f32 magnitudes); quantized: n x dim u8 codes,
           n x {scale, min_val, magnitude, x_sq} f32
"""
import struct
from dataclasses import dataclass, field

import numpy as np

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8

F = np.float32
U64 = (1 << 64) - 1
MAGIC = b"NMNIDX\x00\x01"
KIND_FLAT, KIND_HNSW = 1, 4
HEADER = struct.Struct("<8sIIIIQQQQQ")          # 64 bytes
CONFIG = struct.Struct("<IIIIdQfiiI")           # 48 bytes: the fields of nmn_hnsw_config in declaration order
CONFIG_FIELDS = ("m", "m0", "ef_construction", "ef_search", "ml", "max_nodes", "sparsity_threshold", "distance_metric", "storage",
                 "reserved")
FIXED = struct.Struct("<QQII")                  # rng, entry_point, max_layer, n_upper
STORAGE_DENSE, STORAGE_AUTO, STORAGE_QUANTIZED = 0, 1, 2
GRAPH_AT = HEADER.size
assert HEADER.size == 64 and CONFIG.size == 48


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & U64
    return h


def flat_checksum(payload):
    """the flat section's 64-bit payload checksum (docs/kernels-ingest-tiny-persist.md): four multiply-xor lanes over 32-byte
    blocks, the tail bytes dealt round-robin, folded with the byte count; 0 is never produced (0 = "none recorded")"""
    mul = 0x9E3779B97F4A7C15
    lane = [0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89]
    payload = bytes(payload)
    whole = len(payload) // 32 * 32
    words = np.frombuffer(payload[:whole], dtype="<u8").reshape(-1, 4).tolist()
    for w in words:
        for i in range(4):
            x = ((lane[i] ^ w[i]) * mul) & U64
            lane[i] = x ^ (x >> 29)
    for i, b in enumerate(payload[whole:]):
        x = ((lane[i & 3] ^ b) * mul) & U64
        lane[i & 3] = x ^ (x >> 29)
    h = (len(payload) * 0xD6E8FEB86659FD93) & U64
    for i in range(4):
        h = ((h ^ lane[i]) * mul) & U64
        h ^= h >> 32
    return h or 1


def rng_after(draws, seed=42):
    """state of the reference's xorshift level generator (hnsw.rs:1631-1651) after `draws` inserts"""
    o = ho.HNSWIndex()
    o.rng_seed = seed
    for _ in range(draws):
        o.next_random()
    return o.rng_seed


def chains_magnitude(rows):
    """simd::magnitude of every row, in the reference's order"""
    rows = np.asarray(rows, dtype=F)
    return np.sqrt(q8._chains(rows * rows)).astype(F)


@dataclass
class HnswFile:
    dim: int
    quantized: bool
    config: dict
    rng: int
    entry_point: object              # None = empty index (UINT64_MAX in the file)
    max_layer: int
    levels: list
    nbr: list                        # [node][layer] -> ascending ids
    rows: np.ndarray = None          # dense: [n][dim] f32
    mags: np.ndarray = None          # dense: [n] f32
    codes: np.ndarray = None         # quantized: [n][dim] u8
    rec: np.ndarray = None           # quantized: [n][4] f32 {scale, min_val, magnitude, x_sq}
    header: dict = field(default_factory=dict)   # filled by read(): the header as found, and n_upper
    section_tail: bytes = b""        # writer only: bytes appended to the graph section

    @property
    def n(self):
        return len(self.levels)

    def same_graph(self, other):
        return (self.dim == other.dim and self.quantized == other.quantized and self.config == other.config and
                self.rng == other.rng and self.entry_point == other.entry_point and self.max_layer == other.max_layer and
                list(self.levels) == list(other.levels) and self.nbr == other.nbr)

    def same_rows(self, other):
        def eq(a, b):
            return (a is None and b is None) or (a is not None and b is not None and a.tobytes() == b.tobytes())
        return eq(self.rows, other.rows) and eq(self.mags, other.mags) and eq(self.codes, other.codes) and eq(self.rec, other.rec)


def graph_section(f):
    cfg = CONFIG.pack(*[f.config[k] for k in CONFIG_FIELDS])
    n = f.n
    n_upper = sum(1 for lv in f.levels if lv >= 1)
    out = [cfg, FIXED.pack(f.rng, U64 if f.entry_point is None else f.entry_point, f.max_layer, n_upper)]
    lv = bytes(bytearray(int(x) for x in f.levels))
    out.append(lv + b"\0" * (-n % 4))

    def lst(node, layer):
        return f.nbr[node][layer] if layer < len(f.nbr[node]) else []
    out.append(np.asarray([len(lst(i, 0)) for i in range(n)], dtype="<u4").tobytes())
    for i in range(n):
        out.append(np.asarray(lst(i, 0), dtype="<u4").tobytes())
    for i in range(n):
        for layer in range(1, int(f.levels[i]) + 1):
            ids = lst(i, layer)
            out.append(struct.pack("<I", len(ids)) + np.asarray(ids, dtype="<u4").tobytes())
    out.append(f.section_tail)
    return b"".join(out)


def rows_section(f):
    if f.n == 0:
        return b""
    if f.quantized:
        return np.ascontiguousarray(f.codes, dtype=np.uint8).tobytes() + np.ascontiguousarray(f.rec, dtype="<f4").tobytes()
    payload = np.ascontiguousarray(f.rows, dtype="<f4").tobytes() + np.ascontiguousarray(f.mags, dtype="<f4").tobytes()
    head = HEADER.pack(MAGIC, 1, KIND_FLAT, f.dim, 0, f.n, 0, len(payload), 0, flat_checksum(payload))
    return head + payload


def write(f):
    """-> the file's bytes"""
    sec = graph_section(f)
    rows = rows_section(f)
    head = HEADER.pack(MAGIC, 1, KIND_HNSW, f.dim, 1 if f.quantized else 0, f.n, 0, len(sec) + len(rows), len(sec), fnv1a64(sec))
    return head + sec + rows


def read(data):
    """bytes -> HnswFile; asserts the framing only (sizes, checksums), not the graph rules"""
    data = bytes(data)
    magic, version, kind, dim, flags, n, row_base, payload, aux, reserved = HEADER.unpack_from(data, 0)
    assert magic == MAGIC and version == 1 and kind == KIND_HNSW, (magic, version, kind)
    assert payload == len(data) - HEADER.size and aux <= payload
    sec = data[GRAPH_AT:GRAPH_AT + aux]
    assert fnv1a64(sec) == reserved, "graph section checksum"
    config = dict(zip(CONFIG_FIELDS, CONFIG.unpack_from(sec, 0)))
    rng, entry, max_layer, n_upper = FIXED.unpack_from(sec, CONFIG.size)
    at = CONFIG.size + FIXED.size
    levels = list(sec[at:at + n])
    at += n + (-n % 4)
    l0cnt = np.frombuffer(sec, dtype="<u4", count=n, offset=at).tolist()
    at += 4 * n
    nbr = []
    for i in range(n):
        nbr.append([np.frombuffer(sec, dtype="<u4", count=l0cnt[i], offset=at).tolist()])
        at += 4 * l0cnt[i]
    for i in range(n):
        for _layer in range(1, levels[i] + 1):
            (c,) = struct.unpack_from("<I", sec, at)
            nbr[i].append(np.frombuffer(sec, dtype="<u4", count=c, offset=at + 4).tolist())
            at += 4 + 4 * c
    assert at == aux, (at, aux)
    quantized = bool(flags & 1)
    f = HnswFile(dim=dim, quantized=quantized, config=config, rng=rng, entry_point=None if entry == U64 else entry,
                 max_layer=max_layer, levels=levels, nbr=nbr)
    f.header = dict(version=version, kind=kind, dim=dim, flags=flags, rows=n, row_base=row_base, payload_bytes=payload, aux=aux,
                    reserved=reserved, n_upper=n_upper)
    at = GRAPH_AT + aux
    if n == 0:
        assert at == len(data)
    elif quantized:
        assert len(data) - at == n * dim + 16 * n
        f.codes = np.frombuffer(data, dtype=np.uint8, count=n * dim, offset=at).reshape(n, dim).copy()
        f.rec = np.frombuffer(data, dtype="<f4", count=4 * n, offset=at + n * dim).reshape(n, 4).copy()
    else:
        fm, fv, fk, fdim, fflags, frows, fbase, fpayload, _faux, fsum = HEADER.unpack_from(data, at)
        assert (fm, fv, fk, fdim, fflags, frows, fbase) == (MAGIC, 1, KIND_FLAT, dim, 0, n, 0)
        assert fpayload == 4 * n * dim + 4 * n == len(data) - at - HEADER.size
        body = data[at + HEADER.size:]
        assert fsum == flat_checksum(body), "flat section checksum"
        f.rows = np.frombuffer(body, dtype="<f4", count=n * dim).reshape(n, dim).copy()
        f.mags = np.frombuffer(body, dtype="<f4", count=n, offset=4 * n * dim).copy()
    return f


def patch(data, offset, new_bytes, restamp=True):
    """`data` with new_bytes at `offset` (same length); restamp: the graph section's checksum is recomputed into the header"""
    b = bytearray(data)
    b[offset:offset + len(new_bytes)] = new_bytes
    if restamp:
        aux = struct.unpack_from("<Q", b, 48)[0]
        struct.pack_into("<Q", b, 56, fnv1a64(bytes(b[GRAPH_AT:GRAPH_AT + aux])))
    return bytes(b)


def flip_bit(data, offset, bit=0, restamp=False):
    return patch(data, offset, bytes([data[offset] ^ (1 << bit)]), restamp)


# offsets inside a file, for patches
RNG_AT = GRAPH_AT + CONFIG.size
ENTRY_AT = RNG_AT + 8
MAX_LAYER_AT = RNG_AT + 16
LEVELS_AT = GRAPH_AT + CONFIG.size + FIXED.size


def golden_config(z, quantized):
    import math
    m, m0, efc, efs, metric = z["config"].tolist()
    return dict(m=m, m0=m0, ef_construction=efc, ef_search=efs, ml=1.0 / math.log(m), max_nodes=10_000_000,
                sparsity_threshold=0.5, distance_metric=metric, storage=STORAGE_QUANTIZED if quantized else STORAGE_DENSE,
                reserved=0)


def from_golden(z, quantized=False):
    """tests/golden/hnsw_small.npz / hnsw_q8_small.npz -> the HnswFile the library must save after inserting its rows"""
    n = len(z["levels"])
    levels = [int(x) for x in z["levels"]]
    nbr = [[z["l0"][i, :int(z["l0cnt"][i])].tolist()] for i in range(n)]
    at = 0
    for node, layer, c in z["up_head"].tolist():
        assert len(nbr[node]) == layer
        nbr[node].append(z["up_ids"][at:at + c].tolist())
        at += c
    f = HnswFile(dim=z["rows"].shape[1], quantized=quantized, config=golden_config(z, quantized), rng=rng_after(n),
                 entry_point=int(z["entry_point"]), max_layer=int(z["max_layer"]), levels=levels, nbr=nbr)
    if quantized:
        deq = np.asarray(z["dequantized"], dtype=F)
        x_sq = q8.squared_magnitude(z["codes"], z["scale"], z["min_val"])
        f.codes = np.asarray(z["codes"], dtype=np.uint8)
        f.rec = np.stack([z["scale"].astype(F), z["min_val"].astype(F), chains_magnitude(deq), x_sq.astype(F)], axis=1)
    else:
        f.rows = np.asarray(z["rows"], dtype=F)
        f.mags = chains_magnitude(f.rows)
    return f
