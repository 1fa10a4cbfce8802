"""The top-k search over a delta set on the device (docs/delta.md §8): deltaset_select_kernel and the large-k path forced with
min_device_rows = 0 and held to the twin tests/_deltaset_oracle.py bit for bit on the cases of tests/_deltaset_cases.py; the
stream-ordered form on a side stream against the host-buffer form; two threads on one set; every answer unchanged by the calls
before it."""
import numpy as np
import pytest

from tests import _delta_cases as dc
from tests import _deltaset_cases as sc

pytestmark = pytest.mark.gpu
F = np.float32
DEV = dc.ALWAYS


@pytest.mark.parametrize("n", sc.SIZES)
def test_search_sizes(n):
    sc.check_sizes(DEV, n)


@pytest.mark.parametrize("k", (4096, 4097))
def test_search_at_the_select_limit(k):
    sc.check_k_border(DEV, k)


def test_search_ties():
    sc.check_all_equal(DEV)
    sc.check_tie_runs(DEV)
    sc.check_zeros(DEV)


def test_search_special_scores():
    sc.check_specials(DEV)


@pytest.mark.parametrize("which", ("low", "mid", "top"))
def test_search_radix_patterns(which):
    sc.check_radix(DEV, which)


@pytest.mark.parametrize("nq", (1, 2, 5))
def test_search_of_scored_sets(nq):
    sc.check_scored_set(DEV, nq)


def test_search_of_encoded_and_unsorted_sets():
    sc.check_encoded_and_unsorted(DEV)


def test_search_empty_set_and_refusals():
    sc.check_empty_set_and_refusals(DEV)


def test_search_in_blocks_of_queries():
    sc.check_query_blocks(DEV)


def test_search_around_the_single_query_threshold():
    sc.check_single_query_threshold(DEV)


def test_search_two_threads():
    sc.check_two_threads(DEV)


def test_search_answer_does_not_depend_on_the_calls_before_it():
    sc.check_history(DEV)


def test_device_and_host_paths_agree_on_one_handle():
    s, _, _ = sc.planted(DEV, sc.mixed_values(5000, 200))
    q = np.stack([sc.E0, sc.NEGATIVE])
    got = [s.search(q, k, m) for k in (10, 4096, 4097) for m in sc.METRICS]
    s.registry.set_min_device_rows(dc.NEVER)
    want = [s.search(q, k, m) for k in (10, 4096, 4097) for m in sc.METRICS]
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and dc.same(g[1], w[1]) and np.array_equal(g[2], w[2])


def test_stream_ordered_search_equals_the_host_buffer_form_on_a_side_stream():
    import torch
    from neumann_amd import DeltaVectorError
    n = 5000
    s, twin, deltas = sc.planted(DEV, sc.mixed_values(n, 200))
    q = np.stack([sc.E0, sc.NEGATIVE])
    tq = torch.from_numpy(q).cuda()
    with pytest.raises(DeltaVectorError, match="not resident"):
        s.search_device(tq, 3)
    s.to_device()
    for text, call in (("k of at least 1", lambda: s.search_device(tq, 0)),
                       ("the search needs", lambda: s.search_device(tq, 3, scratch=torch.empty(16, dtype=torch.uint8, device="cuda")))):
        with pytest.raises(DeltaVectorError, match=text):
            call()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    answers = {}
    with torch.cuda.stream(side):
        for k in (1, 10, 4096, 4097, n + 1):
            for m in sc.METRICS:
                answers[k, m] = s.search_device(tq, k, m)
    side.synchronize()
    # a raw stream handle and a scratch of the caller's, reused across calls
    scratch = torch.empty(s.search_scratch_bytes(2, 4097), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    raw = [s.search_device(tq, 10, "dot", stream=side.cuda_stream, scratch=scratch),
           s.search_device(tq, 4097, "cosine", stream=side.cuda_stream, scratch=scratch),
           s.search_device(tq, 10, "dot", stream=side.cuda_stream)]
    side.synchronize()
    for (k, m), (rows, scores, counts) in answers.items():
        w = s.search(q, k, m)
        assert np.array_equal(rows.cpu().numpy(), w[0]), (k, m)
        assert dc.same(scores.cpu().numpy(), w[1]) and np.array_equal(counts.cpu().numpy().astype(np.uint32), w[2]), (k, m)
        sc.assert_answer(w, sc.expect(twin, deltas, q, m, ("border", n)), k, (k, m))
    for got, key in zip(raw, ((10, "dot"), (4097, "cosine"), (10, "dot"))):
        assert all(torch.equal(a, b) or (a.dtype == torch.float32 and dc.same(a.cpu().numpy(), b.cpu().numpy()))
                   for a, b in zip(got, answers[key])), key


# ---- sets made on the device --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threshold", dc.THRESHOLDS)
@pytest.mark.parametrize("dim", dc.ENCODE_DIMS)
def test_encode_device(dim, threshold):
    sc.check_encode_device(dim, threshold)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130, 300, 1100))
def test_encode_device_rows(n):
    sc.check_encode_device_rows(n)


def test_encode_device_slice_scan_and_empty_slices():
    sc.check_encode_device_slices()


def test_encode_device_at_the_largest_dimension():
    sc.check_encode_device_wide()


def test_host_arrays_come_on_first_need():
    sc.check_host_arrays_on_first_need()


def test_encode_device_on_a_side_stream_and_refusals():
    sc.check_encode_device_stream_and_refusals()


def test_encode_batch_joins_its_chunks():
    sc.check_encode_batch_joins_its_chunks()
