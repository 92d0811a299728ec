"""The part of ``scvae.analyses`` that ``scvae evaluate`` needs to report
on a model: label prediction from the latent representation
(``scvae/analyses/prediction.py``) with the clustering metrics it prints, and
the summary statistics of the evaluation set and of its reconstruction, the
metrics table of ``analyse_results`` (``scvae/analyses/metrics/summary.py``),
the PCA of its "Decompositions"
(``scvae/analyses/decomposition/decomposition.py``), and the t-SNE map of its
"latent space" (``scvae/analyses/subanalyses.py:595-673``), and the
histograms of its "Distributions" (``scvae/analyses/subanalyses.py:50-291``)
as tables, and the pairwise distance matrices of its "Distances"
(``scvae/analyses/subanalyses.py:294-468``) as arrays.  The ``analyse``
command, the metrics files, plots and the other decomposition methods are not
part of this build."""
from scvae_amd.analyses.prediction import (  # noqa: F401
    PREDICTION_METHODS, PredictionSpecifications, predict_labels,
    map_cluster_ids_to_label_ids)
from scvae_amd.analyses.silhouette import (  # noqa: F401
    silhouette_samples, silhouette_score)
from scvae_amd.analyses.count_silhouette import (  # noqa: F401
    count_silhouette_samples, count_silhouette_score)
from scvae_amd.analyses.summary import (  # noqa: F401
    comparison_statistics, format_summary_statistics, summary_statistics)
from scvae_amd.analyses.decomposition import (  # noqa: F401
    DevicePCA, decompose)
from scvae_amd.analyses.tsne import (  # noqa: F401
    DeviceTSNE, decompose_latent)
from scvae_amd.analyses.distributions import (  # noqa: F401
    distribution_histograms, histogram, order_statistics, percentile)
from scvae_amd.analyses.distances import (  # noqa: F401
    distance_matrices, evaluation_distances, hierarchical_order,
    pairwise_distances, write_distances)
