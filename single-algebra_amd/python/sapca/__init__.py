"""sapca: MI355X-native sparse PCA (the src/dimred/pca hot path of SingleRust/single-algebra).

Python is the test/bench host here; the product is libsapca.so (C ABI in include/sapca.h).
"""
from ._lib import LIB_PATH, SapcaError, load  # noqa: F401
from .pca import (DeviceCsr, MaskedSparsePCA, MaskedSparsePCABuilder, PowerIterationNormalizer,  # noqa: F401
                  SparsePCA, SparsePCABuilder, SVDMethod, TSNE, KMeans, UMAP, Louvain, Harmony)
from .multi import MultiDevice  # noqa: F401
from .ops import Session  # noqa: F401  (Session.knn: the neighbour search behind a fit)
from ._lib import KNN_METRICS, KNN_MAX_NEIGHBORS, find_ab_params  # noqa: F401
