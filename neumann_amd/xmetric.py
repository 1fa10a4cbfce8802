"""`tensor_store::DistanceMetric` (tensor_store/src/distance.rs:13-194), the ExtendedDistanceMetric of
VectorEngine::search_with_hnsw_and_metric (vector_engine/src/lib.rs:2560-2619) — host wrapper of `nmn_xmetric`
(include/neumann_gpu.h).  The arithmetic runs on the GPU (neumann_amd/csrc/nmn_xmetric.hip); `to_similarity` and
`higher_is_better` are the library's host functions."""
import ctypes as C

from . import _capi


class GeometricConfig:
    """GeometricConfig (distance.rs:115-166)."""

    def __init__(self, cosine_weight=0.5, structural_weight=0.3, magnitude_weight=0.2):
        self.cosine_weight = float(cosine_weight)
        self.structural_weight = float(structural_weight)
        self.magnitude_weight = float(magnitude_weight)

    @classmethod
    def _preset(cls, name):
        m = _capi.XMetric()
        getattr(_capi.load(), "nmn_xmetric_geometric_" + name)(C.byref(m))
        return cls(m.cosine_weight, m.structural_weight, m.magnitude_weight)

    @classmethod
    def default(cls):
        return cls._preset("default")

    @classmethod
    def angular_heavy(cls):
        return cls._preset("angular_heavy")

    @classmethod
    def structural_heavy(cls):
        return cls._preset("structural_heavy")

    @classmethod
    def conflict_detection(cls):
        return cls._preset("conflict_detection")

    def __eq__(self, other):
        return isinstance(other, GeometricConfig) and self._c_weights() == other._c_weights()

    def _c_weights(self):
        m = _capi.XMetric(0, self.cosine_weight, self.structural_weight, self.magnitude_weight)
        return (m.cosine_weight, m.structural_weight, m.magnitude_weight)

    def __repr__(self):
        return f"GeometricConfig({self.cosine_weight}, {self.structural_weight}, {self.magnitude_weight})"


class ExtendedDistanceMetric:
    """DistanceMetric (distance.rs:13-52): the class attributes Cosine .. Manhattan are the unit variants, `Composite(config)`
    builds the ninth."""
    _NAMES = ("Cosine", "Angular", "Geodesic", "Jaccard", "Overlap", "WeightedJaccard", "Euclidean", "Manhattan", "Composite")

    def __init__(self, kind, config=None):
        self.kind = int(kind)
        self.config = config

    @classmethod
    def Composite(cls, config=None):
        return cls(_capi.XMETRIC_COMPOSITE, config or GeometricConfig.default())

    @classmethod
    def from_name(cls, name):
        """"cosine", "weighted_jaccard", "WeightedJaccard", ... ("composite": GeometricConfig::default())"""
        key = name.replace("_", "").lower()
        for i, n in enumerate(cls._NAMES):
            if n.lower() == key:
                return cls.Composite() if i == _capi.XMETRIC_COMPOSITE else cls(i)
        raise _capi.NeumannGpuError(_capi.ERR_CONFIGURATION, f"unknown extended distance metric {name!r}")

    @property
    def name(self):
        return self._NAMES[self.kind] if 0 <= self.kind < len(self._NAMES) else f"Unknown({self.kind})"

    def _c(self):
        g = self.config or GeometricConfig(0.0, 0.0, 0.0)
        return _capi.XMetric(self.kind, g.cosine_weight, g.structural_weight, g.magnitude_weight)

    def to_similarity(self, raw):
        """DistanceMetric::to_similarity (distance.rs:92-106), f32 in and out"""
        m = self._c()
        return float(_capi.load().nmn_xmetric_to_similarity(C.byref(m), float(raw)))

    def higher_is_better(self):
        """DistanceMetric::higher_is_better (distance.rs:60-69)"""
        m = self._c()
        return bool(_capi.load().nmn_xmetric_higher_is_better(C.byref(m)))

    def __eq__(self, other):
        return isinstance(other, ExtendedDistanceMetric) and self.kind == other.kind and self.config == other.config

    def __hash__(self):
        return hash(self.kind)

    def __repr__(self):
        return f"ExtendedDistanceMetric.{self.name}" + (f"({self.config!r})" if self.config else "")


for _i, _n in enumerate(ExtendedDistanceMetric._NAMES[:-1]):
    setattr(ExtendedDistanceMetric, _n, ExtendedDistanceMetric(_i))


def score_host_rows(query, rows, metric, device=-1):
    """(compute(), to_similarity(compute())) of ONE query against rows in host memory, on the GPU (nmn_xmetric_score_host_rows):
    f32 [len(rows)] each.  Rows of any length; no index is involved."""
    import numpy as np
    q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.ndim == 1:
        r = r[None, :]
    if r.shape[1] != q.size:
        raise _capi.NeumannGpuError(_capi.ERR_DIMENSION_MISMATCH, f"expected {q.size}, got {r.shape[1]}")
    raw = np.empty(r.shape[0], dtype=np.float32)
    sim = np.empty(r.shape[0], dtype=np.float32)
    m = metric._c()
    _capi.check(_capi.load().nmn_xmetric_score_host_rows(int(device), C.c_void_p(r.ctypes.data), r.shape[0], r.shape[1],
                                                         C.c_void_p(q.ctypes.data), C.byref(m), C.c_void_p(raw.ctypes.data),
                                                         C.c_void_p(sim.ctypes.data)))
    return raw, sim
