"""nmn_tt_decompose / nmn_tt_decompose_device (neumann_amd.tt.tt_decompose) on the GPU against tests/_tt_decompose_oracle.py: status,
ranks and core BITS, every branch of docs/hnsw.md §21 at the smallest shape that reaches it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import _tt_decompose_oracle as do

pytestmark = pytest.mark.gpu
F = np.float32
CASES = do.gpu_cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


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


def assert_same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(bits(got[3]), bits(want[3])), np.argwhere(bits(got[3]) != bits(want[3]))[:5]


@functools.lru_cache(maxsize=None)
def twin(i):
    _, shape, r, t, vectors = CASES[i]
    return do.decompose_batch(vectors, shape, r, t)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_device_equals_the_twin(i):
    from neumann_amd import TTConfig, tt
    name, shape, r, t, vectors = CASES[i]
    cfg = TTConfig(shape, r, t)
    want = twin(i)
    if tt.decompose_lds_floats(cfg) is None:
        assert_same(tt.tt_decompose_raw(vectors, cfg), want)       # the host path must still match
        pytest.skip(f"{shape} with rank {r} is above the published limits of the device path {tt.decompose_limits()}")
    with env(NMN_TT_DECOMPOSE_MIN=0):
        got = tt.tt_decompose_raw(vectors, cfg)
        assert_same(got, want)
        assert np.isfinite(got[3]).all()
        status_only = tt.tt_decompose_raw(vectors, cfg, want_cores=False)
        assert np.array_equal(status_only[0], want[0]) and np.array_equal(status_only[1], want[1])
        for threads in (128, 256):     # the layout is a choice of speed, never of bits
            with env(NMN_TT_DECOMPOSE_THREADS=threads):
                assert_same(tt.tt_decompose_raw(vectors, cfg), want)


def test_expected_branches_are_the_ones_reached():
    by = {c[0]: twin(i) for i, c in enumerate(CASES)}
    assert by["random_448"][1].tolist() == [[1, 4, 8, 1]] * 3
    assert by["rank_one_234"][1].tolist() == [[1, 1, 1, 1]] * 2
    assert by["zero_234"][1].tolist() == [[1, 2, 4, 1]] and by["zero_34"][1].tolist() == [[1, 3, 1]]
    assert by["tolerance_0p9_444"][0].tolist() == [1] * 8 + [0] * 8
    assert by["rank_zero_88"][0].tolist() == [0, 0] and by["rank_zero_88"][1].tolist() == [[1, 0, 1]] * 2
    assert by["randomized_33x34"][1][:, 1].max() <= 4 and do.takes_randomized_path(33, 34, 4)
    assert by["randomized_middle_8888"][1].tolist() == [[1, 8, 8, 8, 1]] * 2 and do.takes_randomized_path(64, 64, 8)


@functools.lru_cache(maxsize=None)
def big():
    shape, r, t, v = do.big_batch()
    return shape, r, t, v, do.decompose_batch(v, shape, r, t)


def test_batch_of_300_past_the_grid_rows_equal_one_vector_calls():
    from neumann_amd import TTConfig, tt
    shape, r, t, v, want = big()
    cfg = TTConfig(shape, r, t)
    assert len({tuple(x) for x in want[1].tolist()}) >= 3
    with env(NMN_TT_DECOMPOSE_MIN=0, NMN_TT_DECOMPOSE_GRID=64):      # 300 vectors on 64 workgroups: the stride loop
        got = tt.tt_decompose_raw(v, cfg)
    assert_same(got, want)
    with env(NMN_TT_DECOMPOSE_MIN=0):
        assert_same(tt.tt_decompose_raw(v, cfg), want)
        for q in (0, 1, 2, 51, 299):
            one = tt.tt_decompose_raw(v[q], cfg)
            assert np.array_equal(one[1][0], got[1][q])
            assert np.array_equal(bits(one[3]), bits(got[3][int(got[2][q]):int(got[2][q + 1])]))


def test_routing_by_batch_size_never_changes_the_bits():
    from neumann_amd import TTConfig, tt
    shape, r, t, v, want = big()
    cfg = TTConfig(shape, r, t)
    sub = (want[0][:41], want[1][:41], want[2][:42], want[3][:int(want[2][41])])
    with env(NMN_TT_DECOMPOSE_MIN=0):
        assert_same(tt.tt_decompose_raw(v[:41], cfg), sub)
    with env(NMN_TT_DECOMPOSE_MIN=1 << 30):
        assert_same(tt.tt_decompose_raw(v[:41], cfg), sub)
    assert_same(tt.tt_decompose_raw(v[:41], cfg), sub)               # the default


def test_device_entry_on_torch_tensors_equals_the_host_entry():
    import torch
    from neumann_amd import TTConfig, _capi, tt
    lib = _capi.load()
    shape, r, t, v, want = big()
    v = v[:70]
    cfg = TTConfig(shape, r, t)
    slot = cfg.max_storage
    assert slot == do.max_storage(shape, r)
    sh = np.asarray(shape, dtype=np.uint32)
    vt = torch.from_numpy(v).cuda()
    status = torch.full((70,), 9, dtype=torch.int32, device="cuda")
    ranks = torch.zeros((70, 4), dtype=torch.int32, device="cuda")
    off = torch.zeros(71, dtype=torch.int64, device="cuda")
    cores = torch.zeros(70 * slot, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.nmn_tt_decompose_device(C.c_void_p(vt.data_ptr()), 70, 128, C.c_void_p(sh.ctypes.data), 3, r, C.c_float(t),
                                            C.c_void_p(status.data_ptr()), C.c_void_p(ranks.data_ptr()), C.c_void_p(off.data_ptr()),
                                            C.c_void_p(cores.data_ptr()), cores.numel(), C.c_void_p(stream)))
    torch.cuda.synchronize()
    status, ranks, off, cores = status.cpu().numpy(), ranks.cpu().numpy().astype(np.uint32), off.cpu().numpy(), cores.cpu().numpy()
    assert (status == 0).all() and np.array_equal(ranks, want[1][:70]) and off.tolist() == [q * slot for q in range(71)]
    for q in range(70):
        a, b = int(want[2][q]), int(want[2][q + 1])
        assert np.array_equal(bits(cores[q * slot:q * slot + b - a]), bits(want[3][a:b])), q
    # the slots feed the preparation kernel unchanged: per-query ranks and core_off (nmn_tt_reconstruct takes packed trains)
    tts = tt.tt_decompose(v[:4], cfg)
    rec = tt.tt_reconstruct(tts)
    assert np.abs(rec[0].astype(np.float64) - v[0]).max() <= 1e-4 * np.abs(v[0]).max()       # a rank-one vector, ranks [1,1,1,1]
    # above the limits there is no host to fall back to
    big_shape = np.asarray([256, 256], dtype=np.uint32)
    code = lib.nmn_tt_decompose_device(C.c_void_p(vt.data_ptr()), 1, 65536, C.c_void_p(big_shape.ctypes.data), 2, 64, C.c_float(t),
                                       C.c_void_p(status.ctypes.data), C.c_void_p(ranks.ctypes.data), None, None, 0, C.c_void_p(stream))
    assert code == _capi.ERR_INVALID_ARGUMENT and "limits" in lib.nmn_last_error().decode()
