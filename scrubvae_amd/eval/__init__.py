from .cluster import GaussianMixture, dbscan, gmm  # noqa: F401
from .eval import generative_restrictiveness  # noqa: F401
from .hdbscan import HDBSCAN  # noqa: F401
from .metrics import cluster_entropy, linear_rand_cv, log_class_rand_cv, mlp_rand_cv, qda_rand_cv  # noqa: F401
