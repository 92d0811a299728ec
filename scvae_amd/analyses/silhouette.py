"""Silhouette values of a clustering of latent values on the device: the
"silhouette score" of a label prediction
(``scvae/analyses/metrics/clustering.py:120-142``) as the exact computation
over every pair of cells on the kernel of ``csrc/silhouette.hip``.

The definition is scikit-learn's ``silhouette_samples`` with the Euclidean
metric: for cell i of cluster A, a_i is the mean distance to the other cells
of A, b_i the lowest mean distance to the cells of another cluster, and
s_i = (b_i - a_i) / max(a_i, b_i), 0 in a cluster of one cell and when
max(a_i, b_i) = 0.  The score is the mean of s_i.

What differs from the reference on purpose: the reference hands the count
matrix (cells x genes) to scikit-learn and samples it down to 20 000 cells;
``scvae evaluate --silhouette-score`` scores the clustering in the latent
space it was made in, over every cell.  Distances are in the direct form
``sqrt(sum (x - y)^2)`` in fp32 and every sum has one fixed order, so the same
input gives the same bits on every run.
"""
import ctypes

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.kmeans import _as_matrix, _ptr

MINIMUM_ROWS = 3
MAXIMUM_LATENT_SIZE = 256


def limit_reason(number_of_rows, latent_size, number_of_clusters):
    """Why these sizes are outside what the kernel takes (``None``: they are
    inside)."""
    n, l, k = int(number_of_rows), int(latent_size), int(number_of_clusters)
    if not 1 <= l <= MAXIMUM_LATENT_SIZE:
        return "latent size {} (1 to {} supported)".format(
            l, MAXIMUM_LATENT_SIZE)
    if n < MINIMUM_ROWS:
        return "{} cells (at least {} supported)".format(n, MINIMUM_ROWS)
    if n >= 2 ** 31:
        return "{} cells (fewer than 2^31 supported)".format(n)
    if not 2 <= k <= n - 1:
        return "{} clusters for {} cells (2 to cells - 1 supported)".format(
            k, n)
    return None


def _cluster_ids(labels, number_of_rows):
    """Labels as 0 .. K - 1 through their sorted distinct values."""
    labels = numpy.asarray(labels).reshape(-1)
    if labels.shape[0] != number_of_rows:
        raise ValueError("{} labels for {} rows.".format(
            labels.shape[0], number_of_rows))
    distinct, ids = numpy.unique(labels, return_inverse=True)
    return len(distinct), ids.reshape(-1).astype(numpy.int64)


def _run(matrix, ids, number_of_clusters, device):
    """(s [N] fp32 in the caller's row order, on the device; the score)."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError(
            "No GPU visible: the device silhouette has no CPU path.")
    n, latent_size = matrix.shape
    reason = limit_reason(n, latent_size, number_of_clusters)
    if reason is not None:
        raise ValueError("Device silhouette: " + reason + ".")
    counts = numpy.bincount(ids, minlength=number_of_clusters)
    offsets = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(
        numpy.int64)
    if (offsets[0] != 0 or offsets[-1] != n
            or not (numpy.diff(offsets) > 0).all()):
        raise ValueError("Device silhouette: the cluster offsets must "
                         "increase strictly from 0 to the number of rows.")
    lib = _lib.load()
    device = torch.device(device if device is not None else "cuda:0")
    # a stable sort by cluster; the rows are gathered on the device
    order = torch.sort(torch.from_numpy(ids).to(device), stable=True)[1]
    x = torch.from_numpy(matrix).to(device)[order].contiguous()
    offsets = torch.from_numpy(offsets).to(device)
    nbytes = lib.scvae_silhouette_workspace_bytes(
        n, latent_size, number_of_clusters)
    if nbytes < 0:
        _lib.check(-1, "scvae_silhouette_workspace_bytes")
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    grouped = torch.empty(n, dtype=torch.float32, device=device)
    score = torch.zeros(1, dtype=torch.float64, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        _lib.check(lib.scvae_silhouette_samples(
            _ptr(x), x.stride(0), n, latent_size, _ptr(offsets),
            number_of_clusters, None, None, _ptr(grouped), _ptr(score),
            _ptr(workspace), workspace.numel(), stream),
            "scvae_silhouette_samples")
    values = torch.empty_like(grouped)
    values[order] = grouped
    return values, float(score.item())


def silhouette_samples(values, labels, device=None):
    """The silhouette value of every row of ``values`` ([cells, latent]) under
    ``labels`` (any values; equal labels make a cluster): fp32 ``[cells]`` in
    the caller's row order."""
    matrix = _as_matrix(values)
    number_of_clusters, ids = _cluster_ids(labels, matrix.shape[0])
    return _run(matrix, ids, number_of_clusters, device)[0].cpu().numpy()


def silhouette_score(values, labels, device=None):
    """The mean silhouette value, taken in fp64 on the device; ``nan`` for
    fewer than 2 or more than cells - 1 distinct labels (the reference's rule,
    ``clustering.py:125-127``), for which no GPU is opened."""
    labels = numpy.asarray(labels).reshape(-1)
    number_of_rows = (values.shape[0] if hasattr(values, "shape")
                      else len(values))
    number_of_clusters = numpy.unique(labels).shape[0]
    if number_of_clusters < 2 or number_of_clusters > number_of_rows - 1:
        return float("nan")
    matrix = _as_matrix(values)
    number_of_clusters, ids = _cluster_ids(labels, matrix.shape[0])
    return _run(matrix, ids, number_of_clusters, device)[1]
