"""The cached path of VectorEngine::search_similar (vector_engine/src/lib.rs:1976-2001) and search_in_collection (1622-1646) over
tests/_hnsw_oracle.py's index: walk, map node ids to keys, strip the prefix, stable sort by score descending, truncate.  What the
engine's hnsw_cache hook is held to (tests/test_gpu_engine_hnsw_cache.py); itself held to hand-made cases by
tests/test_hnsw_cache_oracle_cpu.py."""
import numpy as np

DEFAULT_ENTRY = "_default"   # the default collection's name in hnsw_cache (lib.rs:1332, 1979)


def embedding_prefix():                      # lib.rs:1337-1339
    return "emb:"


def collection_embedding_prefix(collection):  # lib.rs:1346-1348
    return f"coll:{collection}:emb:"


def cached_search(index, mapping, prefix, query, top_k):
    """-> [(key, score f32)], or None when the hook is not taken (no entry: mapping None; or an empty mapping) and the caller falls
    through to the exhaustive search.  `index` None stands for an empty HNSWIndex."""
    if mapping is None or len(mapping) == 0:          # `if let Some(..) = cache.get(..)`, `if !mapping.is_empty()`
        return None
    neighbors = index.search(np.asarray(query, dtype=np.float32), top_k) if index is not None else []
    results = []
    for node, score in neighbors:                     # filter_map over `mapping.get(idx)`
        if node < len(mapping):
            key = mapping[node]
            results.append((key[len(prefix):] if key.startswith(prefix) else key, np.float32(score)))  # strip_prefix().unwrap_or(key)
    results.sort(key=lambda r: r[1], reverse=True)    # sort_by(b.score.partial_cmp(a.score)): stable, equal scores keep their order
    return results[:top_k]
