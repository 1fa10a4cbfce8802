"""tests/_hnsw_bulk_oracle.py against tests/_hnsw_oracle.py: the batched build (docs/hnsw.md §19) gives the sequential graph, list
for list, and the corpora can tell: with the validation switched off every one of them gives another graph."""
import pytest

from tests import _hnsw_bulk_oracle as bo


@pytest.mark.parametrize("name", sorted(bo.CASES))
def test_batched_build_is_the_sequential_graph(name):
    want = bo.case_sequential(name)
    got, st = bo.case_bulk(name)
    print(name, st)
    assert bo.same_graph(got, want)                                   # levels, entry, max_layer, generator state, every list
    n = bo.CASES[name][1]
    assert st["host_nodes"] == 1 and st["walks"] == n - 1             # min_nodes 1: only the first node of the empty index
    assert st["accepted"] + st["conflicts"] == st["walks"]
    # a condition on the INPUT: both outcomes of the validation are exercised, each by a twentieth of the walks at least
    assert 20 * st["accepted"] >= st["walks"] and 20 * st["conflicts"] >= st["walks"], st


@pytest.mark.parametrize("name", sorted(bo.CASES))
def test_without_validation_the_graph_differs(name):
    want = bo.case_sequential(name)
    got, st = bo.case_bulk(name, False)
    assert st["conflicts"] == 0 and st["accepted"] == st["walks"]
    assert got.levels == want.levels and got.rng_seed == want.rng_seed  # (levels are data-independent)
    assert not bo.same_graph(got, want)


def test_batch_cut_and_min_nodes():
    """a batch ends behind the first node above the top layer; below min_nodes every node takes the plain path"""
    name = "same-cos"
    rows, cfg = bo.case_rows(name), bo.case_config(name)
    want = bo.case_sequential(name)
    for batch, min_nodes in ((1, 1), (5, 40), (64, 1), (1000, 149), (8, 1000)):
        got, st = bo.bulk_build(rows, cfg, batch, min_nodes)
        assert bo.same_graph(got, want), (batch, min_nodes)
        assert st["host_nodes"] == min(max(min_nodes, 1), len(rows)) and st["walks"] == len(rows) - st["host_nodes"]
        assert st["batches"] >= -(-st["walks"] // batch)
        if batch == 1:
            assert st["conflicts"] == 0                               # a batch of one reads nothing dirty
