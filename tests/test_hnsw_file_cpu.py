"""tests/_hnsw_file.py, the Python reader / writer of the HNSW index file (docs/hnsw.md §10), held to known answers: the
GPU tests rely on it to judge the files the library writes and to craft the files the library must refuse."""
import os

import numpy as np
import pytest

from tests import _hnsw_file as hf
from tests import _hnsw_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = {False: os.path.join(ROOT, "tests", "golden", "hnsw_small.npz"), True: os.path.join(ROOT, "tests", "golden", "hnsw_q8_small.npz")}


def test_fnv1a64_known_answers():
    assert hf.fnv1a64(b"") == 0xcbf29ce484222325
    assert hf.fnv1a64(b"a") == 0xaf63dc4c8601ec8c


@pytest.mark.parametrize("quantized", [False, True])
def test_write_then_read_is_the_identity(quantized):
    z = np.load(GOLDEN[quantized])
    f = hf.from_golden(z, quantized)
    data = hf.write(f)
    g = hf.read(data)
    assert g.same_graph(f) and g.same_rows(f)
    assert hf.write(g) == data
    h = g.header
    n, dim = z["rows"].shape
    assert (h["version"], h["kind"], h["dim"], h["flags"], h["rows"], h["row_base"]) == (1, 4, dim, int(quantized), n, 0)
    assert h["payload_bytes"] == len(data) - 64 and h["n_upper"] == int((z["levels"] > 0).sum())
    rows_bytes = n * dim + 16 * n if quantized else 64 + 4 * n * dim + 4 * n
    assert h["aux"] == h["payload_bytes"] - rows_bytes
    # the graph the file holds is the golden's
    assert g.levels == z["levels"].tolist() and g.entry_point == int(z["entry_point"]) and g.max_layer == int(z["max_layer"])
    for node in range(n):
        assert g.nbr[node][0] == z["l0"][node, :int(z["l0cnt"][node])].tolist()
    at = 0
    for node, layer, c in z["up_head"].tolist():
        assert g.nbr[node][layer] == z["up_ids"][at:at + c].tolist()
        at += c


def test_empty_index_file():
    z = np.load(GOLDEN[False])
    f = hf.HnswFile(dim=20, quantized=False, config=hf.golden_config(z, False), rng=42, entry_point=None, max_layer=0, levels=[], nbr=[])
    data = hf.write(f)
    assert len(data) == 64 + 72
    g = hf.read(data)
    assert g.same_graph(f) and g.n == 0 and g.entry_point is None and g.header["payload_bytes"] == g.header["aux"] == 72


def test_rng_is_the_oracles_state_after_800_draws():
    o = ho.HNSWIndex()
    levels = [o.random_level() for _ in range(800)]
    z = np.load(GOLDEN[False])
    assert levels == z["levels"].tolist()          # the generator the golden graph was built with ...
    f = hf.from_golden(z)
    assert f.rng == o.rng_seed == hf.rng_after(800) != 42   # ... and its state is what the writer stamps
    assert hf.read(hf.write(f)).rng == o.rng_seed
    assert hf.rng_after(0) == 42


def test_patch_restamps_the_checksum():
    data = hf.write(hf.from_golden(np.load(GOLDEN[False])))
    p = hf.patch(data, hf.RNG_AT, (7).to_bytes(8, "little"))
    assert hf.read(p).rng == 7 and len(p) == len(data)
    with pytest.raises(AssertionError):
        hf.read(hf.flip_bit(data, hf.LEVELS_AT + 5))      # not restamped: the checksum no longer verifies
    with pytest.raises(AssertionError):
        hf.read(hf.flip_bit(data, len(data) - 100))       # a bit of a row: the flat section's checksum
