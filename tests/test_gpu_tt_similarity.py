"""nmn_tt_similarity, nmn_tt_self_dot and their device forms (neumann_amd.tt) on the GPU against tests/_tt_similarity_oracle.py, bit for
bit (a NaN compared as a NaN), at the smallest shapes that reach each path of docs/hnsw.md §23."""
import os
import threading

import numpy as np
import pytest

from tests import _tt_decompose_oracle as do
from tests import _tt_similarity_oracle as so
from tests.test_tt_similarity_cpu import GOLDEN, NAN_BITS, bits, lib_trains, same, special_pairs

pytestmark = pytest.mark.gpu
F = np.float32
OPS = (so.DOT, so.COSINE, so.EUCLIDEAN)


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def check(qs, ts, ops=OPS):
    """the host-buffer entries on the DEVICE (NMN_TT_SIMILARITY_MIN=0: a call of any size goes there) against the twin"""
    from neumann_amd import tt
    lq, lt = lib_trains(qs), lib_trains(ts)
    self_q = np.asarray([so.self_dot(q) for q in qs], dtype=F)
    self_t = np.asarray([so.self_dot(t) for t in ts], dtype=F)
    dots = so.similarity(so.DOT, qs, ts)
    with env(NMN_TT_SIMILARITY_MIN=0):
        for op in ops:
            want = dots if op == so.DOT else so.finish(op, dots, self_q[:, None], self_t[None, :])
            got = tt.tt_similarity(op, lq, lt)
            assert same(got, want), (op, np.argwhere(bits(got) != bits(want))[:5])
        assert same(tt.tt_self_dot(lt), self_t)


def trains(seed, shape, ranks, n):
    rng = np.random.default_rng(seed)
    return [so.random_tt(rng, shape, ranks) for _ in range(n)]


# r2a * r2b below, at and above one wave's 64 lanes, the largest the kernel takes, and r_a != r_b
@pytest.mark.parametrize("rq,rt", [(2, 2), (8, 8), (9, 9), (32, 32), (3, 5), (32, 1)])
def test_ranks_against_the_twin(rq, rt):
    qs = trains(rq * 100 + rt, [2, 2, 2], [1, rq, rq, 1], 2)
    ts = trains(rq * 100 + rt + 1, [2, 2, 2], [1, rt, rt, 1], 3)
    check(qs, ts)


@pytest.mark.parametrize("shape,ranks", [([7], [1, 1]), ([1, 5], [1, 3, 1]), ([3, 1, 5], [1, 2, 2, 1]), ([1, 1, 7], [1, 1, 1, 1]),
                                         ([2] * 8, [1, 2, 3, 2, 3, 2, 2, 2, 1])])
def test_one_two_three_and_eight_cores_and_modes_of_one(shape, ranks):
    qs = trains(len(shape) * 7 + 1, shape, ranks, 3)
    ts = trains(len(shape) * 7 + 2, shape, ranks, 4) + trains(len(shape) * 7 + 3, shape, [1] * (len(shape) + 1), 1)
    check(qs, ts)


def test_core_storage_at_exactly_the_limit():
    """16 32 + 32 7 32 + 32 16 = 8192 floats: the query fills the LDS the kernel has for it, and three waves share the rest"""
    from neumann_amd import tt
    assert tt.limits()[:3] == (8, 32, 8192)
    qs = trains(81, [16, 7, 16], [1, 32, 32, 1], 1)
    assert qs[0].flat().size == 8192
    ts = trains(82, [16, 7, 16], [1, 32, 32, 1], 2) + trains(83, [16, 7, 16], [1, 2, 3, 1], 3)
    check(qs, ts, ops=(so.DOT, so.EUCLIDEAN))


def test_a_train_beyond_the_limits_shares_a_call_with_trains_the_kernel_takes():
    """rank 33: the pairs it takes part in are the host restatement's, the others the kernel's, all of them the twin's bits"""
    shape = [2, 3, 2]
    qs = trains(91, shape, [1, 2, 2, 1], 2) + trains(92, shape, [1, 33, 33, 1], 1) + trains(93, shape, [1, 4, 3, 1], 1)
    ts = trains(94, shape, [1, 33, 2, 1], 1) + trains(95, shape, [1, 3, 3, 1], 3)
    check(qs, ts)
    check(qs[2:3], ts[1:])      # every query beyond the limits: no pair is left for the kernel
    check(qs[:2], ts[:1])       # every target beyond the limits


def mixed_ranks(seed, n):
    rng = np.random.default_rng(seed)
    choices = ([1, 2, 2, 1], [1, 2, 3, 1], [1, 1, 1, 1], [1, 4, 5, 1])
    return [so.random_tt(rng, [2, 2, 5], choices[int(rng.integers(0, 4))]) for _ in range(n)]


@pytest.mark.parametrize("nq,nt", [(1, 1), (3, 5), (1, 257), (65, 2)])
def test_batch_sizes_and_orientation(nq, nt):
    qs, ts = mixed_ranks(nq * 1000 + nt, nq), mixed_ranks(nq * 1000 + nt + 1, nt)
    check(qs, ts)
    with env(NMN_TT_SIMILARITY_GRID=4):     # four workgroups: the stride loop over work items and the waves' loop over a chunk
        check(qs, ts)


def test_golden_file_and_routing_by_size_never_changes_the_bits():
    from neumann_amd import tt
    z = np.load(GOLDEN)
    qs, ts = so.golden_sets()
    lq, lt = lib_trains(qs), lib_trains(ts)
    for min_pairs in (None, 0, 1 << 30):     # the default (384 pairs: the device), the device, the host
        with env(**({} if min_pairs is None else {"NMN_TT_SIMILARITY_MIN": min_pairs})):
            for name, op in (("dot", so.DOT), ("cosine", so.COSINE), ("euclidean", so.EUCLIDEAN)):
                assert same(tt.tt_similarity(op, lq, lt), z[name]), (name, min_pairs)
                assert same(tt.tt_similarity(op, lq[:2], lt[:3]), z[name][:2, :3]), (name, min_pairs)   # 6 pairs: the host by default
            assert same(tt.tt_self_dot(lq), z["self_q"]) and same(tt.tt_self_dot(lt), z["self_t"])


def test_special_trains_in_one_call():
    """the cosine threshold from both sides, the zero train, NaN cores and the pair whose squared distance is negative"""
    sp = special_pairs()
    check([p[1] for p in sp], [p[2] for p in sp])


def test_self_dot_is_the_square_of_tt_norm_in_bits():
    from neumann_amd import tt
    ts = mixed_ranks(55, 70) + [p[1] for p in special_pairs()]
    lt = lib_trains(ts)
    with env(NMN_TT_SIMILARITY_MIN=0):
        selfs, norms = tt.tt_self_dot(lt), tt.tt_norm(lt)
    with np.errstate(all="ignore"):
        assert same(np.sqrt(selfs), norms)
    assert same(selfs, [so.self_dot(t) for t in ts])


# ---- the device chain: decompose on the device, then self dots, then similarity --------------------------------------------------

def device_chain(vectors, shape, max_rank, tolerance, q_rows, with_core_off):
    """-> (status, {op: matrix [len(q_rows)][n]}, self dots [n]) from nmn_tt_decompose_device, nmn_tt_self_dot_device and
    nmn_tt_similarity_device on one stream, nothing read back in between"""
    import ctypes as C
    import torch
    from neumann_amd import TTConfig, _capi, tt
    lib = _capi.load()
    cfg = TTConfig(shape, max_rank, tolerance)
    n, d, slot = len(vectors), len(shape), cfg.max_storage
    sh = np.asarray(shape, dtype=np.uint32)
    vt = torch.from_numpy(np.ascontiguousarray(vectors)).cuda()
    status = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    ranks = torch.zeros((n, d + 1), dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    cores = torch.zeros(n * slot, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.nmn_tt_decompose_device(C.c_void_p(vt.data_ptr()), n, vectors.shape[1], C.c_void_p(sh.ctypes.data), d, max_rank,
                                            C.c_float(cfg.tolerance), C.c_void_p(status.data_ptr()), C.c_void_p(ranks.data_ptr()),
                                            C.c_void_p(off.data_ptr()), C.c_void_p(cores.data_ptr()), cores.numel(), C.c_void_p(stream)))
    targets = tt.TTDeviceSet(ranks, cores, slot, off if with_core_off else None, status)
    lo, hi = q_rows
    queries = tt.TTDeviceSet(ranks[lo:hi], cores[lo * slot:hi * slot], slot, None, status[lo:hi])   # the same slots, a view
    self_t = tt.tt_self_dot_device(shape, targets)
    self_q = tt.tt_self_dot_device(shape, queries)
    out = {op: tt.tt_similarity_device(op, shape, queries, targets, self_q, self_t) for op in OPS}
    torch.cuda.synchronize()
    assert same(self_q.cpu().numpy(), self_t.cpu().numpy()[lo:hi])
    return status.cpu().numpy(), {op: m.cpu().numpy() for op, m in out.items()}, self_t.cpu().numpy()


@pytest.mark.parametrize("with_core_off", [False, True])
def test_device_chain_equals_the_host_buffer_entry(with_core_off):
    from neumann_amd import TTConfig, tt
    shape, r, t, v = do.big_batch()
    v = v[:40]
    status, got, selfs = device_chain(v, shape, r, t, (5, 17), with_core_off)
    assert (status == 0).all()
    host = tt.tt_decompose(v, TTConfig(shape, r, t))
    assert len({tuple(x.ranks) for x in host}) >= 3
    for op in OPS:
        assert same(got[op], tt.tt_similarity(op, host[5:17], host)), op
    assert same(selfs, tt.tt_self_dot(host))


def test_device_chain_with_failed_decompositions_leaves_the_documented_nan():
    """tolerance 0.9: the first 8 of the 16 vectors are NMN_TT_EMPTY_MATRIX — their rows and columns are 0x7FC00000, the rest is the
    host-buffer entry's"""
    from neumann_amd import TTConfig, tt
    name, shape, r, t, v = [c for c in do.gpu_cases() if c[0] == "tolerance_0p9_444"][0]
    status, got, selfs = device_chain(v, list(shape), r, t, (4, 12), False)
    assert status.tolist() == [1] * 8 + [0] * 8
    host = tt.tt_decompose(v, TTConfig(shape, r, t), return_status=True)
    good = [x for x in host if isinstance(x, tt.TTVector)]
    assert len(good) == 8
    assert (bits(selfs[:8]) == NAN_BITS).all() and same(selfs[8:], tt.tt_self_dot(good))
    for op in OPS:
        m = got[op]
        assert (bits(m[:4]) == NAN_BITS).all() and (bits(m[:, :8]) == NAN_BITS).all(), op
        assert same(m[4:, 8:], tt.tt_similarity(op, good[:4], good)), op


# ---- ranks the host cannot check: the kernel's bounds check ------------------------------------------------------------------------

GUARD = 4096


def guarded(array, fill):
    """a device tensor with GUARD elements of `fill` on both sides of `array` -> (whole, view of the middle)"""
    import torch
    a = torch.from_numpy(np.ascontiguousarray(array))
    whole = torch.full((a.numel() + 2 * GUARD,), fill, dtype=a.dtype).cuda()
    whole[GUARD:GUARD + a.numel()] = a.reshape(-1).cuda()
    return whole, whole[GUARD:GUARD + a.numel()].view(a.shape)


def guards_intact(whole, fill):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == fill).all() and (w[-GUARD:] == fill).all())


BAD = {"rank_of_0": [1, 0, 2, 1], "rank_of_33": [1, 33, 2, 1], "cores_past_the_slot": [1, 2, 3, 1], "end_rank_of_2": [2, 2, 2, 1]}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_device_ranks_give_nan_and_touch_nothing_else(case):
    """6 queries and 9 targets in slots of 22 floats (shape [2,2,5], ranks [1,2,2,1]); query 2 and target 7 carry the bad rank
    vector.  Every array sits between guard regions; the bad trains' outputs are 0x7FC00000, every other output is the twin's, and
    no guard is written.  This is a bounds check that passes: nothing here faults."""
    import torch
    from neumann_amd import tt
    shape, good, slot = [2, 2, 5], [1, 2, 2, 1], 22
    qs, ts = trains(301, shape, good, 6), trains(302, shape, good, 9)
    held = []

    def device_set(tts, bad_at):
        ranks = np.asarray([t.ranks for t in tts], dtype=np.int32)
        ranks[bad_at] = BAD[case]
        cores = np.stack([t.flat() for t in tts]).astype(F)
        wr, r = guarded(ranks, 1 << 20)           # a guard read as a rank would be far above every limit
        wc, c = guarded(cores.reshape(-1), 3.0)
        held.extend([(wr, 1 << 20), (wc, 3.0)])
        return tt.TTDeviceSet(r, c, slot)

    dq, dt = device_set(qs, 2), device_set(ts, 7)
    wsq, sq = guarded(np.zeros(6, dtype=F), 5.0)
    wst, st = guarded(np.zeros(9, dtype=F), 5.0)
    held.extend([(wsq, 5.0), (wst, 5.0)])
    tt.tt_self_dot_device(shape, dq, out=sq)
    tt.tt_self_dot_device(shape, dt, out=st)
    outs = {}
    for op in OPS:
        wo, o = guarded(np.full((6, 9), 7.0, dtype=F), 5.0)
        held.append((wo, 5.0))
        outs[op] = tt.tt_similarity_device(op, shape, dq, dt, sq, st, out=o)
    torch.cuda.synchronize()
    for whole, fill in held:
        assert guards_intact(whole, fill)
    sq, st = sq.cpu().numpy(), st.cpu().numpy()
    assert bits(sq[2]) == NAN_BITS and bits(st[7]) == NAN_BITS
    keep_q, keep_t = [i for i in range(6) if i != 2], [j for j in range(9) if j != 7]
    assert same(sq[keep_q], [so.self_dot(qs[i]) for i in keep_q]) and same(st[keep_t], [so.self_dot(ts[j]) for j in keep_t])
    for op in OPS:
        m = outs[op].cpu().numpy()
        assert (bits(m[2]) == NAN_BITS).all() and (bits(m[:, 7]) == NAN_BITS).all(), op
        want = so.similarity(op, [qs[i] for i in keep_q], [ts[j] for j in keep_t])
        assert same(m[np.ix_(keep_q, keep_t)], want), op


def test_core_off_that_leaves_the_buffer_is_a_bad_train():
    """core_off given: a train whose range is longer than its cores need is fine, one that ends past n * stride floats or whose
    range is shorter than its cores is bad"""
    import torch
    from neumann_amd import tt
    shape, good, slot = [2, 2, 5], [1, 2, 2, 1], 22
    ts = trains(303, shape, good, 5)
    ranks = np.asarray([t.ranks for t in ts], dtype=np.int32)
    # train 1 in a range of 30 floats (fine), train 2 in one of 10 (short of its 22), train 3 at 62, train 4 at 100: it would end at
    # 122, past the 5 * 22 floats of the buffer
    off = np.asarray([0, 22, 52, 62, 100, 122], dtype=np.int64)
    cores = np.zeros(5 * slot, dtype=F)
    for i in (0, 1, 3):
        cores[off[i]:off[i] + slot] = ts[i].flat()
    wr, r = guarded(ranks, 1 << 20)
    wc, c = guarded(cores, 3.0)
    wo, o = guarded(off, 1 << 40)
    ws, s = guarded(np.zeros(5, dtype=F), 5.0)
    tt.tt_self_dot_device(shape, tt.TTDeviceSet(r, c, slot, o), out=s)
    torch.cuda.synchronize()
    assert all(guards_intact(w, f) for w, f in ((wr, 1 << 20), (wc, 3.0), (wo, 1 << 40), (ws, 5.0)))
    s = s.cpu().numpy()
    assert same(s[[0, 1, 3]], [so.self_dot(ts[i]) for i in (0, 1, 3)]) and (bits(s[[2, 4]]) == NAN_BITS).all()


def test_eight_threads_call_the_host_buffer_entry_at_once():
    from neumann_amd import tt
    qs, ts = so.golden_sets()
    z = np.load(GOLDEN)
    lq, lt = lib_trains(qs), lib_trains(ts)
    results, errors = [None] * 8, []

    def work(i):
        try:
            op = OPS[i % 3]
            results[i] = [tt.tt_similarity(op, lq, lt) for _ in range(4)]
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    pool = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in pool:
        t.start()
    for t in pool:
        t.join()
    assert not errors, errors
    for i in range(8):
        for m in results[i]:
            assert same(m, z[("dot", "cosine", "euclidean")[i % 3]]), i
