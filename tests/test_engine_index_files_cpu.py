"""What the three binary loaders of the engine refuse, and with which words: load_index_binary (a collection), load_ivf_index and
load_hnsw_index.  Every file here is crafted from the 64-byte PersistHeader of neumann_amd/csrc/nmn_persist.h plus a text
block, a few dozen bytes each, and every loader fails (or finishes) before it touches a device, so these run on the CPU box."""
import struct

import pytest

from neumann_amd.engine import VectorEngine, VectorEngineConfig, VectorError, _lib

MAGIC = b"NMNIDX\x00\x01"
HEADER = struct.Struct("<8sIIIIQQQQQ")  # magic, version, kind, dim, flags, rows, row_base, payload_bytes, aux, reserved
KIND_FLAT, KIND_ENGINE = 1, 3
assert HEADER.size == 64

CONFIG = '"config": {"dimension": null, "distance_metric": "Cosine", "auto_index": false, "auto_index_threshold": 1000}'
SER = "Serialization error: "


def index_file(text, rows=0, flags=0, kind=KIND_ENGINE, magic=MAGIC, aux=None, tail=b""):
    text = text.encode()
    return HEADER.pack(magic, 1, kind, 0, flags, rows, 0, 0, len(text) if aux is None else aux, 0) + text + tail


# loader -> (method, the flags its header carries, a text block it accepts with rows = 0, what it calls its file)
LOADERS = {
    "collection": ("load_index_binary", 0, '{"collection": "default", ' + CONFIG + ', "vectors": []}', "collection"),
    "ivf": ("load_ivf_index", 1, '{"nprobe": 3, "dim": 4, "trained": false, "keys": []}', "IVF index"),
    "hnsw": ("load_hnsw_index", 2, '{"dim": 4, "built": false, "keys": []}', "HNSW index"),
}


def refused(tmp_path, loader, data, config=None):
    path = tmp_path / "index.bin"
    path.write_bytes(data)
    engine = VectorEngine(config) if config else VectorEngine()
    with pytest.raises(VectorError) as err:
        getattr(engine, LOADERS[loader][0])(path)
    assert engine.count() == 0
    return err.value.kind, str(err.value)


@pytest.mark.parametrize("loader", LOADERS)
def test_the_smallest_valid_file_loads(tmp_path, loader):
    method, flags, text, _ = LOADERS[loader]
    path = tmp_path / "index.bin"
    path.write_bytes(index_file(text, flags=flags))
    got = getattr(VectorEngine(), method)(path)
    if loader == "collection":
        assert got == "default"
    else:
        assert list(got[1]) == [] and len(got[0]) == 0


@pytest.mark.parametrize("loader", LOADERS)
def test_wrong_magic_kind_or_flags(tmp_path, loader):
    _, flags, text, what = LOADERS[loader]
    want = ("SerializationError", SER + f"not a neumann_gpu {what} file")
    assert refused(tmp_path, loader, index_file(text, flags=flags, magic=b"NMNIDX\x00\x02")) == want
    assert refused(tmp_path, loader, index_file(text, flags=flags, kind=KIND_FLAT)) == want
    assert refused(tmp_path, loader, b"NMN") == want  # shorter than a header
    if loader != "collection":  # the collection loader does not look at the flags
        for other in {0, 1, 2, 3} - {flags}:
            assert refused(tmp_path, loader, index_file(text, flags=other)) == want


@pytest.mark.parametrize("loader", LOADERS)
def test_text_block_larger_than_the_file(tmp_path, loader):
    _, flags, text, _ = LOADERS[loader]
    want = ("SerializationError", SER + "file truncated (text block)")
    assert refused(tmp_path, loader, index_file(text, flags=flags, aux=len(text) + 1)) == want
    assert refused(tmp_path, loader, index_file(text, flags=flags, aux=(1 << 40) + 1)) == want


@pytest.mark.parametrize("loader", LOADERS)
def test_text_block_that_is_not_json_or_not_an_object(tmp_path, loader):
    _, flags, _, _ = LOADERS[loader]
    assert refused(tmp_path, loader, index_file("not json", flags=flags)) == ("SerializationError", SER + "invalid literal at byte 0")
    assert refused(tmp_path, loader, index_file('{"dim": 4,}', flags=flags)) == ("SerializationError", SER + "expected string at byte 10")
    assert refused(tmp_path, loader, index_file("[1, 2]", flags=flags)) == ("SerializationError", SER + "invalid text block")
    assert refused(tmp_path, loader, index_file("", flags=flags)) == ("SerializationError", SER + "unexpected end at byte 0")


def test_collection_text_block_lacks_a_field(tmp_path):
    for text in ('{"collection": "default", ' + CONFIG + '}', '{' + CONFIG + ', "vectors": []}', '{"collection": 1, "vectors": []}'):
        assert refused(tmp_path, "collection", index_file(text)) == ("SerializationError", SER + "missing field `collection` / `vectors`")
    assert refused(tmp_path, "collection", index_file('{"collection": "default", "vectors": []}')) == (
        "SerializationError", SER + "missing field `config`")
    assert refused(tmp_path, "collection", index_file('{"collection": "default", "config": {"dimension": null}, "vectors": []}')) == (
        "SerializationError", SER + "missing field in `config`")
    entry = '{"collection": "default", ' + CONFIG + ', "vectors": [{"key": "k", "metadata": null}]}'
    assert refused(tmp_path, "collection", index_file(entry, rows=1)) == ("SerializationError", SER + "invalid entry")


@pytest.mark.parametrize("loader,texts", [
    ("ivf", ('{"dim": 4, "trained": false, "keys": []}', '{"nprobe": 3, "trained": false, "keys": []}',
             '{"nprobe": 3, "dim": 4, "keys": []}', '{"nprobe": 3, "dim": 4, "trained": false}',
             '{"nprobe": 3.5, "dim": 4, "trained": false, "keys": []}', '{"nprobe": 3, "dim": 4, "trained": 0, "keys": []}',
             '{"nprobe": 3, "dim": 4, "trained": false, "keys": [1, 2]}')),
    ("hnsw", ('{"built": false, "keys": []}', '{"dim": 4, "keys": []}', '{"dim": 4, "built": false}',
              '{"dim": -1, "built": false, "keys": []}', '{"dim": 4, "built": "no", "keys": []}',
              '{"dim": 4, "built": false, "keys": [1, 2]}')),
])
def test_index_text_block_lacks_a_field(tmp_path, loader, texts):
    for text in texts:
        assert refused(tmp_path, loader, index_file(text, flags=LOADERS[loader][1])) == ("SerializationError", SER + "invalid text block"), text


def test_keys_that_differ_from_the_header(tmp_path):
    assert refused(tmp_path, "collection", index_file(LOADERS["collection"][2], rows=1)) == (
        "SerializationError", SER + "entry count differs from the header")
    for loader, text in (("ivf", '{"nprobe": 3, "dim": 4, "trained": false, "keys": ["a"]}'),
                         ("hnsw", '{"dim": 4, "built": false, "keys": ["a"]}')):
        flags = LOADERS[loader][1]
        for rows in (0, 2):
            assert refused(tmp_path, loader, index_file(text, rows=rows, flags=flags)) == (
                "SerializationError", SER + "key count differs from the header")
        mixed = text.replace('["a"]', '["a", 1]')
        assert refused(tmp_path, loader, index_file(mixed, rows=2, flags=flags)) == ("SerializationError", SER + "invalid key")


def test_an_untrained_ivf_index_keeps_its_keys(tmp_path):
    """build_ivf_index of an empty store has no keys, but the loader does not insist: only the HNSW one does"""
    path = tmp_path / "index.bin"
    path.write_bytes(index_file('{"nprobe": 3, "dim": 4, "trained": false, "keys": ["a", "b"]}', rows=2, flags=1))
    index, _ = VectorEngine().load_ivf_index(path)
    assert len(index) == 0
    assert [_lib().nmn_engine_ivf_key(index._h, i) for i in range(3)] == [b"a", b"b", None]


def test_an_hnsw_index_that_was_never_built_carries_nothing(tmp_path):
    want = ("SerializationError", SER + "an index that was never built carries keys or a section")
    assert refused(tmp_path, "hnsw", index_file('{"dim": 4, "built": false, "keys": ["a"]}', rows=1, flags=2)) == want
    assert refused(tmp_path, "hnsw", index_file(LOADERS["hnsw"][2], flags=2, tail=b"\0")) == want


@pytest.mark.parametrize("loader", LOADERS)
def test_file_size_limit_at_one_byte_over(tmp_path, loader):
    method, flags, text, _ = LOADERS[loader]
    data = index_file(text, flags=flags)
    size = len(data)
    assert refused(tmp_path, loader, data, VectorEngineConfig(max_index_file_bytes=size - 1)) == (
        "ConfigurationError", f"Configuration error: index file size {size} exceeds limit {size - 1}")
    getattr(VectorEngine(VectorEngineConfig(max_index_file_bytes=size)), method)(tmp_path / "index.bin")  # the file `refused` wrote


@pytest.mark.parametrize("loader,at_the_limit", [
    # one entry is within the limit, so each loader goes on to what it checks next
    ("collection", SER + "entry count differs from the header"),
    ("ivf", SER + "key count differs from the header"),
    ("hnsw", SER + "key count differs from the header"),
])
def test_entry_limit_at_one_entry_over(tmp_path, loader, at_the_limit):
    _, flags, text, _ = LOADERS[loader]
    few = VectorEngineConfig(max_index_entries=1)
    # the limit is applied to the header's count, before the text block is read: an empty block is not reached
    assert refused(tmp_path, loader, index_file("", rows=2, flags=flags), few) == (
        "ConfigurationError", "Configuration error: index entry count 2 exceeds limit 1")
    assert refused(tmp_path, loader, index_file(text, rows=2, flags=flags), few) == (
        "ConfigurationError", "Configuration error: index entry count 2 exceeds limit 1")
    assert refused(tmp_path, loader, index_file(text, rows=1, flags=flags), few) == ("SerializationError", at_the_limit)
    assert refused(tmp_path, loader, index_file(text, rows=2, flags=flags), VectorEngineConfig(max_index_entries=None)) == (
        "SerializationError", at_the_limit)
