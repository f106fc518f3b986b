from .cluster import GaussianMixture, KMeans, dbscan, gmm, kmeans  # noqa: F401
from .hmm import GaussianHMM, dwell_times, hmm, state_runs  # noqa: F401
from .conditional_mi import (conditional_mutual_information, conditional_mutual_information_permutation_test,  # noqa: F401
                             conditional_permutations)
from .density import DensityGrid, DensityMap, density_map, density_regions  # noqa: F401
from .embed import TSNE, tsne, tsne_affinities  # noqa: F401
from .embed_transform import TSNEMap, tsne_transform  # noqa: F401
from .embed_quality import EmbeddingQuality, continuity, embedding_quality, neighbor_ranks, trustworthiness  # noqa: F401
from .eval import generative_restrictiveness  # noqa: F401
from .hdbscan import HDBSCAN  # noqa: F401
from .independence import HSICPermutationResult, hsic, hsic_bandwidth, hsic_permutation_test  # noqa: F401
from .metrics import (cluster_entropy, hungarian_match, knn_class_rand_cv, knn_reg_rand_cv, lda_rand_cv, linear_rand_cv,  # noqa: F401
                      log_class_rand_cv, mlp_rand_cv, mmd_bandwidth, mmd_estimate, mmd_permutation_test, mmd_permutations,
                      qda_rand_cv, shannon_entropy)
from .mutual_info import MIPermutationResult, latent_mi_scores, mutual_information, mutual_information_permutation_test  # noqa: F401
from .neighbors import kneighbors, kneighbors_cross, kneighbors_graph, knn_label_purity, knn_transfer_labels  # noqa: F401
from .silhouette import cluster_medoids, cluster_silhouette, silhouette_samples, silhouette_score  # noqa: F401
from .transport import SinkhornDivergence, SinkhornResult, sinkhorn, sinkhorn_divergence, transport_flow  # noqa: F401
