"""nmn_sparse_canonicalise_device / neumann_amd.hnsw.sparse_canonicalise_device against tests/_hnsw_sparse_query_oracle.py:
SparseVector::try_from_parts, magnitude and to_dense of CSR queries in device memory — the BITS of offsets, entries, magnitudes,
duplicate flags and dense rows (docs/hnsw.md §22).  A query with a status is the entry-less query.

One exception to "bits": where the oracle's magnitude is NaN the device's must be a NaN; the reference (Rust) leaves the payload
of a NaN an operation produces unspecified, so there are no bits to hold it to."""
import numpy as np
import pytest

from tests import _hnsw_sparse_query_oracle as so

pytestmark = pytest.mark.gpu
F = np.float32
GRID = 1024  # kCanonGridMax, nmn_sparse_canon.hip: the workgroups of one launch


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32)


def csr_of(queries):
    indptr = np.cumsum([0] + [len(p) for p, _ in queries]).astype(np.int64)
    pos = np.array([x for p, _ in queries for x in p], dtype=np.uint32)
    val = np.concatenate([np.asarray(v, dtype=F).reshape(-1) for _, v in queries] + [np.zeros(0, dtype=F)])
    return indptr, pos, val


def run(dim, indptr, pos, val, max_nnz=None, stream=None, sync=True):
    import torch
    from neumann_amd.hnsw import sparse_canonicalise_device
    dev = torch.device("cuda")
    ip = torch.from_numpy(np.asarray(indptr, dtype=np.int64)).to(dev)
    p = torch.from_numpy(np.asarray(pos, dtype=np.uint32).view(np.int32)).to(dev)
    v = torch.from_numpy(np.asarray(val, dtype=F)).to(dev)
    out = sparse_canonicalise_device(dim, ip, p, v, max_nnz=max_nnz, stream=stream)
    out["_keep"] = (ip, p, v)
    if sync:
        torch.cuda.synchronize()
    return out


def expected(dim, indptr, pos, val, max_nnz):
    """per query (status, SparseQuery): the first rule that fails, and what the oracle makes of a served query"""
    res, nnz_total = [], len(pos)
    for a, b in zip(indptr[:-1], indptr[1:]):
        a, b = int(a), int(b)
        if b < a or b > nnz_total or b - a > max_nnz:
            res.append((2, so.SparseQuery(dim, [], [])))
            continue
        try:
            res.append((0, so.SparseQuery.from_parts(dim, pos[a:b], val[a:b])))
        except so.IndexOutOfBounds:
            res.append((1, so.SparseQuery(dim, [], [])))
    return res


def check(dim, indptr, pos, val, max_nnz=None, out=None):
    out = out or run(dim, indptr, pos, val, max_nnz)
    want = expected(dim, indptr, pos, val, max_nnz or min(dim, 4096))
    off = out["off"].cpu().numpy()
    ent = out["entries"].cpu().numpy().view(np.uint32)
    mag, dup = out["mag"].cpu().numpy(), out["dup"].cpu().numpy()
    dense, status = out["dense"].cpu().numpy(), out["status"].cpu().numpy()
    assert status.tolist() == [s for s, _ in want]
    assert off.tolist() == np.cumsum([0] + [len(sq) for _, sq in want]).tolist()
    for q, (_, sq) in enumerate(want):
        e = ent[off[q]:off[q + 1]]
        assert e[:, 0].tolist() == sq.positions, q
        assert e[:, 1].tolist() == bits(sq.values).tolist(), q
        m = sq.magnitude()
        if np.isnan(m):
            assert np.isnan(mag[q]), q
        else:
            assert bits(mag[q]) == bits(m), (q, mag[q], m)
        assert int(dup[q]) == int(len(set(sq.positions)) != len(sq.positions)), q
        assert np.array_equal(bits(dense[q]), bits(sq.to_dense())), q
    return out


def random_query(rng, dim, n, zeros=0.1):
    """n raw entries: positions with repeats once n nears dim, a share of zeros of both signs among the values"""
    pos = rng.integers(0, dim, n)
    val = rng.standard_normal(n).astype(F)
    z = rng.random(n) < zeros
    val[z] = np.where(rng.random(int(z.sum())) < 0.5, F(0.0), F(-0.0))
    return pos.tolist(), val


def test_raw_counts_at_the_edges_of_the_sort():
    """the wave, workgroup and power-of-two edges of the network and the LDS limit in ONE call; 4097 raw entries: status 2"""
    rng = np.random.default_rng(22)
    dim = 771
    counts = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3]
    csr = csr_of([random_query(rng, dim, n) for n in counts])
    out = check(dim, *csr, max_nnz=4096)
    assert out["status"].cpu().tolist() == [0] * 11 + [2, 0]


def test_dropping_and_order():
    nan = F(np.nan)
    queries = [
        ([3, 1, 7], [0.0, -0.0, 0.0]),                                     # zeros only
        ([4, 2, 9, 0], [0.0, nan, -0.0, 1.5]),                             # both zeros dropped, NaN kept
        (list(range(11, -1, -1)), np.arange(1, 13, dtype=F)),              # strictly descending positions
        ([5, 5, 5], [3.0, 1.0, 2.0]),                                      # one position three times: the input's order
        ([7, 2, 9, 2, 0, 4, 2], [1.5, -3.0, 0.0, 4.0, -0.0, 0.25, -8.0]),  # all of it
    ]
    out = check(12, *csr_of(queries))
    assert out["dup"].cpu().tolist() == [0, 0, 0, 1, 1]
    assert out["dense"].cpu().numpy()[3, 5] == F(2.0)                      # the last of a duplicated position wins


@pytest.mark.parametrize("dim", [5, 8, 33, 771])
def test_every_position_once(dim):
    rng = np.random.default_rng(dim)
    perm = rng.permutation(dim)
    val = rng.standard_normal(dim).astype(F)
    val[val == 0] = F(1.0)
    out = check(dim, *csr_of([(perm.tolist(), val), (list(range(dim)), val)]))
    assert out["off"].cpu().tolist() == [0, dim, 2 * dim]


def test_magnitude_is_one_f64_chain_in_position_order():
    """(3e-30, 4e-30): the squares underflow in f32 and are ordinary numbers in f64, the magnitude is 5e-30.
    The six values whose squares are §13's (2^24, 1, 2^-30 four times): the chain runs by position whatever the input order.
    The tie case: squares 1, 2^-24, 2^-24 and eighty of 2^-54.  By ascending position (the 1 first) every 2^-54 is a quarter of an
    ulp of the running sum and is lost: S = 1 + 2^-23, sqrt = 1 + 2^-24 - 2^-49, below the f32 tie at 1 + 2^-24: 1.0.  By descending
    position the eighty add up first: S = 1 + 2^-23 + 1.25 * 2^-48, sqrt = 1 + 2^-24 + 2^-51, above the tie: 1 + 2^-23."""
    six = [2.0 ** 12, 1.0, 2.0 ** -15, 2.0 ** -15, 2.0 ** -15, 2.0 ** -15]
    perm = [3, 0, 5, 1, 4, 2]
    tie = [1.0, 2.0 ** -12, 2.0 ** -12] + [2.0 ** -27] * 80
    n = len(tie)
    shuffle = np.random.default_rng(83).permutation(n)
    queries = [
        ([0, 1], [3e-30, 4e-30]),
        (list(range(6)), six),
        (list(range(5, -1, -1)), six),
        ([perm[i] for i in range(6)], [six[perm[i]] for i in range(6)]),   # ascending pairs, shuffled input
        ([], []),                                                          # the entry-less query
        (list(range(n)), tie),
        (list(range(n - 1, -1, -1)), tie),
        ([int(i) for i in shuffle], [tie[int(i)] for i in shuffle]),       # = ascending
        ([n - 1 - int(i) for i in shuffle], [tie[int(i)] for i in shuffle]),  # = descending
    ]
    out = check(96, *csr_of(queries))
    mag = out["mag"].cpu().numpy()
    assert bits(mag[0]) == bits(F(5e-30))
    assert bits(mag[4]) == bits(so.SparseQuery(96, [], []).magnitude()) == 0x80000000   # sqrt(-0.0) = -0.0
    assert mag[5] == F(1.0) and mag[6] == F(1.0) + F(2.0 ** -23)
    assert bits(mag[7]) == bits(mag[5]) and bits(mag[8]) == bits(mag[6])
    assert bits(mag[3]) == bits(mag[1])


def test_statuses_beside_valid_queries():
    """status 1: a position == dim beside one == dim - 1, and one attached to a 0.0 value (checked before the value is looked at).
    status 2: a decreasing indptr, a range past nnz_total.  The valid queries around them are unaffected."""
    dim = 9
    pos = np.array([8, 1, 8, 9, 2, 9, 4, 0, 3, 3, 6], dtype=np.uint32)
    val = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 6.0, 7.0, 8.0, 9.0, -1.0], dtype=F)
    indptr = [0, 2, 4, 6, 8, 7, 9, 11, 14]
    # q0 [0,2) valid; q1 [2,4) has 9; q2 [4,6) has 9 with 0.0; q3 [6,8) valid; q4 [8,7) decreasing; q5 [7,9) valid (overlaps q3's
    # last entry); q6 [9,11) valid; q7 [11,14) past nnz_total = 11
    out = check(dim, indptr, pos, val)
    assert out["status"].cpu().tolist() == [0, 1, 1, 0, 2, 0, 0, 2]


def test_overlapping_ranges_never_write_past_the_entries():
    """behind a decreasing indptr two ranges may overlap, so that the kept entries outnumber nnz_total: the query that no longer
    fits the packed array is status 2, and nothing is written past it"""
    import torch
    dim = 16
    pos = np.arange(8, dtype=np.uint32)
    val = np.arange(1, 9, dtype=F)
    indptr = [0, 6, 2, 8]    # q0 [0,6): 6 entries; q1 decreasing; q2 [2,8): 6 more, 12 > 8
    out = run(dim, indptr, pos, val)
    torch.cuda.synchronize()
    assert out["status"].cpu().tolist() == [0, 2, 2]
    assert out["off"].cpu().tolist() == [0, 6, 6, 6]
    assert out["entries"].cpu().numpy()[:6, 0].tolist() == list(range(6))
    assert out["dense"].cpu().numpy()[2].tolist() == [0.0] * dim


@pytest.mark.parametrize("nq", [1, 2, GRID + 1])
def test_query_counts_and_the_stride_loop(nq):
    rng = np.random.default_rng(nq)
    dim = 20
    check(dim, *csr_of([random_query(rng, dim, int(rng.integers(0, 12))) for _ in range(nq)]))


def test_two_calls_on_a_stream_one_synchronise():
    import torch
    rng = np.random.default_rng(5)
    dim = 33
    a = csr_of([random_query(rng, dim, 20) for _ in range(7)])
    b = csr_of([random_query(rng, dim, 33) for _ in range(5)])
    s = torch.cuda.Stream()   # (the inputs go up with blocking copies before each call)
    oa = run(dim, *a, stream=s, sync=False)
    ob = run(dim, *b, stream=s, sync=False)
    s.synchronize()
    check(dim, *a, out=oa)
    check(dim, *b, out=ob)
