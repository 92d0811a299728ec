"""Silhouette values of a clustering in count space on the device: the
"silhouette score" of a label prediction as the reference takes it
(``scvae/analyses/metrics/clustering.py:120-142``: cells x genes, sampled down
to 20 000 cells above 20 000), on the kernels of ``csrc/count_silhouette.hip``.

The definition is scikit-learn's ``silhouette_samples`` with the Euclidean
metric (see ``analyses/silhouette.py``, which scores the latent values).  The
counts are integers below 65 536, so the squared distance between two cells
is an integer and the device computes it exactly (int8 byte products on the
matrix cores, int32 accumulators, put together in int64); the distance is its
fp64 root rounded to fp32 once, exactly 0 for equal cells and for no others.
Sums of distances are taken in fp64 in one fixed order: the same input gives
the same bits on every run.

The rows are uploaded as CSR and densified to uint16 on the device
(``scvae_csr_densify_u16``) in the cluster-grouped order, a stable sort by
label; answers come back in the caller's row order.
"""
import ctypes

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.kmeans import _ptr
from scvae_amd.analyses.silhouette import _cluster_ids

MINIMUM_ROWS = 3
MAXIMUM_ROWS = 2 ** 20
MAXIMUM_FEATURES = 65536
MAXIMUM_VALUE = 65535
DENSIFY_ROWS = 4096     # rows per launch of the densify kernel


def _stored_values(values):
    """The values a matrix stores (a sparse matrix: its non-zeros)."""
    if hasattr(values, "tocsr"):
        return numpy.asarray(values.tocsr().data)
    return numpy.asarray(values)


def _value_reason(values):
    stored = _stored_values(values)
    if stored.size == 0:
        return None
    if stored.dtype.kind not in "iufb":
        return "values of type {} (integer counts supported)".format(
            stored.dtype)
    if stored.dtype.kind == "f":
        if not numpy.isfinite(stored).all():
            return "values that are not finite (integer counts supported)"
        if (stored != numpy.floor(stored)).any():
            return "values that are not integers (integer counts supported)"
    if stored.min() < 0 or stored.max() > MAXIMUM_VALUE:
        return "values outside 0 to {} (uint16 counts supported)".format(
            MAXIMUM_VALUE)
    return None


def row_pitch(number_of_features):
    """Elements between two uint16 rows: whole 128-byte lines."""
    return (int(number_of_features) + 63) // 64 * 64


def limit_reason(number_of_rows, number_of_features, number_of_clusters,
                 values=None, device=None):
    """Why a call is outside what the kernels take (``None``: it is inside):
    the sizes, then -- with ``values`` -- the stored values, which have to be
    integers in [0, 65 535], and, with a GPU in sight, the uint16 rows, which
    have to fit a quarter of the free device memory (the rule of the resident
    training set)."""
    n, f, k = (int(number_of_rows), int(number_of_features),
               int(number_of_clusters))
    if not 1 <= f <= MAXIMUM_FEATURES:
        return "{} features (1 to {} supported)".format(f, MAXIMUM_FEATURES)
    if n < MINIMUM_ROWS:
        return "{} cells (at least {} supported)".format(n, MINIMUM_ROWS)
    if n > MAXIMUM_ROWS:
        return "{} cells (at most 2^20 supported)".format(n)
    if not 2 <= k <= n - 1:
        return "{} clusters for {} cells (2 to cells - 1 supported)".format(
            k, n)
    if values is not None:
        reason = _value_reason(values)
        if reason is not None:
            return reason
        if torch.cuda.is_available():
            need = n * row_pitch(f) * 2
            free, _ = torch.cuda.mem_get_info(
                torch.device(device if device is not None else "cuda:0"))
            if need > free // 4:
                return ("{:.1f} GB of uint16 rows beyond a quarter of the "
                        "free device memory".format(need / 1e9))
    return None


def _as_csr(values):
    """``values`` as a canonical scipy CSR matrix of fp32 (what the densify
    kernel reads)."""
    import scipy.sparse
    if hasattr(values, "tocsr"):
        matrix = values.tocsr()
    else:
        dense = numpy.asarray(values)
        if dense.ndim != 2:
            raise ValueError("Expected a [cells, genes] matrix, got shape {}."
                             .format(dense.shape))
        matrix = scipy.sparse.csr_matrix(dense)
    if len(matrix.shape) != 2:
        raise ValueError("Expected a [cells, genes] matrix, got shape {}."
                         .format(matrix.shape))
    if not matrix.has_canonical_format:
        matrix = matrix.copy()
        matrix.sum_duplicates()
    matrix.sort_indices()
    return matrix


def _device_call(matrix, order, offsets, device):
    """(s fp32 [N] on the device in the grouped order, the score) of the rows
    ``matrix[order]`` (scipy CSR; ``order`` groups them by cluster)."""
    lib = _lib.load()
    n, f = matrix.shape
    k = len(offsets) - 1
    pitch = row_pitch(f)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        indptr = torch.from_numpy(matrix.indptr.astype(numpy.int64)).to(device)
        indices = torch.from_numpy(
            matrix.indices.astype(numpy.int32)).to(device)
        data = torch.from_numpy(matrix.data.astype(numpy.float32)).to(device)
        if data.numel() == 0:      # (the kernel takes no NULL arrays)
            indices = torch.zeros(1, dtype=torch.int32, device=device)
            data = torch.zeros(1, dtype=torch.float32, device=device)
        rows = torch.from_numpy(numpy.asarray(order, dtype=numpy.int64)).to(
            device)
        x = torch.empty((n, pitch), dtype=torch.uint16, device=device)
        for first in range(0, n, DENSIFY_ROWS):
            last = min(first + DENSIFY_ROWS, n)
            _lib.check(lib.scvae_csr_densify_u16(
                _ptr(indptr), _ptr(indices), _ptr(data),
                _ptr(rows[first:last]), last - first, f,
                _ptr(x[first:last]), pitch, stream), "scvae_csr_densify_u16")
        del indptr, indices, data
        nbytes = lib.scvae_count_silhouette_workspace_bytes(n, f, k)
        if nbytes < 0:
            _lib.check(-1, "scvae_count_silhouette_workspace_bytes")
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
        grouped = torch.empty(n, dtype=torch.float32, device=device)
        score = torch.zeros(1, dtype=torch.float64, device=device)
        _lib.check(lib.scvae_count_silhouette_samples_u16(
            _ptr(x), pitch, n, f,
            _ptr(torch.from_numpy(offsets).to(device)), k, None, None,
            _ptr(grouped), _ptr(score), _ptr(workspace), workspace.numel(),
            stream), "scvae_count_silhouette_samples_u16")
        return grouped, float(score.item())


def _run(values, labels, device):
    """(s [N] fp32 in the caller's row order, on the device; the score)."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError(
            "No GPU visible: the device count-space silhouette has no CPU "
            "path.")
    matrix = _as_csr(values)
    n, f = matrix.shape
    number_of_clusters, ids = _cluster_ids(labels, n)
    device = torch.device(device if device is not None else "cuda:0")
    reason = limit_reason(n, f, number_of_clusters, matrix, device)
    if reason is not None:
        raise ValueError("Device count-space silhouette: " + reason + ".")
    counts = numpy.bincount(ids, minlength=number_of_clusters)
    offsets = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(
        numpy.int64)
    order = numpy.argsort(ids, kind="stable")
    grouped, score = _device_call(matrix, order, offsets, device)
    result = torch.empty_like(grouped)
    result[torch.from_numpy(order).to(device)] = grouped
    return result, score


def _number_of_rows(values):
    return values.shape[0] if hasattr(values, "shape") else len(values)


def count_silhouette_samples(values, labels, device=None):
    """The silhouette value of every row of ``values`` ([cells, genes]: a
    scipy sparse matrix or a dense array of integers in [0, 65 535]) under
    ``labels`` (any values; equal labels make a cluster): fp32 ``[cells]`` in
    the caller's row order."""
    return _run(values, labels, device)[0].cpu().numpy()


def count_silhouette_score(values, labels, sample_size=None,
                           random_state=None, device=None):
    """The mean silhouette value, taken in fp64 on the device; ``nan`` for
    fewer than 2 or more than cells - 1 distinct labels (the reference's rule,
    ``clustering.py:125-127``), for which no GPU is opened.

    ``sample_size`` as in ``sklearn.metrics.silhouette_score``: the rows
    ``numpy.random.RandomState(random_state).permutation(cells)[:sample_size]``
    are scored; a sample with fewer than 2 or more than ``sample_size - 1``
    distinct labels raises ``ValueError``, as scikit-learn does."""
    labels = numpy.asarray(labels).reshape(-1)
    number_of_rows = _number_of_rows(values)
    number_of_clusters = numpy.unique(labels).shape[0]
    if number_of_clusters < 2 or number_of_clusters > number_of_rows - 1:
        return float("nan")
    if sample_size is not None:
        if len(labels) != number_of_rows:
            raise ValueError("{} labels for {} rows.".format(
                len(labels), number_of_rows))
        chosen = numpy.random.RandomState(random_state).permutation(
            number_of_rows)[:int(sample_size)]
        values = (values.tocsr()[chosen] if hasattr(values, "tocsr")
                  else numpy.asarray(values)[chosen])
        labels = labels[chosen]
        distinct = numpy.unique(labels).shape[0]
        if not 2 <= distinct <= len(labels) - 1:
            raise ValueError(
                "Number of labels is {}. Valid values are 2 to n_samples - 1 "
                "(inclusive)".format(distinct))
    return _run(values, labels, device)[1]
