"""Pairwise distances of data sets on the device: the matrices that
``analyse_matrices(..., plot_distances=True)`` plots
(``scvae/analyses/subanalyses.py:294-468``, called for the reconstructed set
and for ``z`` at ``scvae/analyses/analyses.py:1351-1362``).  For each set the
reference hands up to 10 000 sampled examples by all features to
``sklearn.metrics.pairwise_distances`` on the host four times
(``figures/matrices.py:124-130``): Euclidean and cosine, sorted by labels and
by hierarchical clustering (``matrices.py:181-222``).  Here the matrix comes
from ``scvae_pairwise_distances`` (``csrc/distances.hip``): an fp64 Gram
product on the matrix cores that reads the sampled rows in place through a row
index and applies the metric before anything is stored.

What differs from the reference on purpose:

*   the labels sort is ``numpy.argsort(labels, kind="stable")`` (the
    reference's default quicksort leaves the order inside a class to the
    implementation);
*   rows with identical values are at distance exactly 0, the diagonal is
    exactly 0 and the matrix is symmetric bit for bit (scikit-learn's
    expanded fp32 form leaves about 2e-7 between duplicates);
*   nothing is plotted: the matrices are returned and written as arrays.
"""
import ctypes
import os
from time import time

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.kmeans import _ptr
from scvae_amd.utilities import normalise_string

#: ``subanalyses.py:41-42``
MAXIMUM_NUMBER_OF_EXAMPLES_FOR_HEAT_MAPS = 10000
MAXIMUM_NUMBER_OF_EXAMPLES_FOR_DENDROGRAM = 1000
#: the limits of ``scvae_pairwise_distances``
MAXIMUM_ROWS_ON_DEVICE = 1 << 16
MAXIMUM_FEATURES_ON_DEVICE = 1 << 20

DISTANCE_METRICS = ("Euclidean", "cosine")
_METRIC_FLAGS = {"euclidean": 0, "cosine": 1}


class _HostFallback(Exception):
    """The device path does not cover this call: the reason."""


def _is_sparse(x):
    return hasattr(x, "tocsr") and not isinstance(x, numpy.ndarray)


def _device_of(device=None):
    device = torch.device(device if device is not None else "cuda:0")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _metric_flag(metric):
    flag = _METRIC_FLAGS.get(str(metric).lower())
    if flag is None:
        raise ValueError(
            "Distance metric `{}` not found: \"Euclidean\" or "
            "\"cosine\".".format(metric))
    return flag


def _row_index(rows, total_rows):
    """``rows`` as int64 positions, each inside the matrix."""
    rows = numpy.ascontiguousarray(numpy.asarray(rows).reshape(-1),
                                   dtype=numpy.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= total_rows):
        raise IndexError("Row index outside [0, {}).".format(total_rows))
    return rows


def _fits(number_of_bytes, device, what):
    free, _ = torch.cuda.mem_get_info(device)
    if number_of_bytes > free // 4:
        raise _HostFallback(
            "{:.1f} GB of {} against {:.1f} GB of free device memory (a "
            "quarter of it at most)".format(
                number_of_bytes / 1e9, what, free / 1e9))


def _resident(values, device):
    """``values`` as an fp32 ``[N, F]`` device tensor with unit column
    stride: a device tensor as it is, a NumPy array copied, a SciPy sparse
    matrix densified once."""
    if isinstance(values, torch.Tensor):
        if values.dtype != torch.float32:
            raise ValueError("Distances: float32 values expected, got "
                             "{}.".format(values.dtype))
        if values.dim() != 2:
            raise ValueError("Distances: a matrix expected.")
        if not values.is_cuda:
            values = values.to(_device_of(device))
        if (values.shape[1] > 1 and values.stride(1) != 1) or (
                values.shape[0] > 1 and values.stride(0) < values.shape[1]):
            values = values.contiguous()
        return values
    device = _device_of(device)
    _fits(4 * int(values.shape[0]) * int(values.shape[1]), device,
          "dense float32 values")
    if _is_sparse(values):
        from scvae_amd.analyses.decomposition import densify
        from scvae_amd.minibatch import DeviceCSR
        return densify(DeviceCSR.from_scipy(
            values.tocsr().astype(numpy.float32), device))
    values = numpy.asarray(values, dtype=numpy.float32)
    if values.ndim != 2:
        raise ValueError("Distances: a matrix expected.")
    return torch.from_numpy(numpy.ascontiguousarray(values)).to(device)


def _device_distances(values, metric, rows, device, maximum_rows):
    flag = _metric_flag(metric)
    total_rows, features = (int(s) for s in values.shape)
    if rows is not None:
        rows = _row_index(rows, total_rows)
    n = total_rows if rows is None else int(rows.size)
    if not 1 <= n <= maximum_rows:
        raise _HostFallback("{} rows (1 to {} supported)".format(
            n, maximum_rows))
    if not 1 <= features <= MAXIMUM_FEATURES_ON_DEVICE:
        raise _HostFallback("{} features (1 to {} supported)".format(
            features, MAXIMUM_FEATURES_ON_DEVICE))
    if not torch.is_tensor(values) or not values.is_cuda:
        device = _device_of(device)
    else:
        device = values.device
    _fits(4 * n * n, device, "distances")
    tensor = _resident(values, device)
    pitch = int(tensor.stride(0)) if total_rows > 1 else features
    lib = _lib.load()
    out = torch.empty(n, n, dtype=torch.float32, device=device)
    size = lib.scvae_pairwise_distances_workspace_bytes(n, features)
    _lib.check(min(size, 0), "scvae_pairwise_distances_workspace_bytes")
    workspace = torch.empty(size, dtype=torch.uint8, device=device)
    index = (torch.from_numpy(rows).to(device) if rows is not None else None)
    with torch.cuda.device(device):
        _lib.check(lib.scvae_pairwise_distances(
            _ptr(tensor), pitch, total_rows, features, _ptr(index), n, flag,
            _ptr(out), n, _ptr(workspace), size,
            ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
            "scvae_pairwise_distances")
    return out


def _host_values(values):
    if isinstance(values, torch.Tensor):
        values = values.cpu().numpy()
    if _is_sparse(values):
        return values.tocsr()
    return numpy.asarray(values)


def _host_distances(values, metric, rows):
    import sklearn.metrics
    _metric_flag(metric)
    values = _host_values(values)
    if rows is not None:
        values = values[_row_index(rows, values.shape[0])]
    return numpy.asarray(sklearn.metrics.pairwise_distances(
        values, metric=str(metric).lower()), dtype=numpy.float32)


def pairwise_distances(values, metric="euclidean", rows=None, on_device=None,
                       device=None, maximum_rows=MAXIMUM_ROWS_ON_DEVICE):
    """The fp32 ``[n, n]`` matrix of ``sklearn.metrics.pairwise_distances(
    values[rows], metric=metric)`` for ``metric`` "euclidean" or "cosine" (in
    any letter case).  ``values``: ``[N, F]`` as an fp32 device tensor (read
    in place, its row pitch honoured), a NumPy array or a SciPy sparse matrix
    (densified once to resident fp32, within a quarter of the free device
    memory).  ``rows``: positions into ``values`` in the wanted order,
    duplicates allowed (None: all rows); the device reads the rows through
    this index, no gathered copy is made.  A device tensor comes back for a
    device tensor, a NumPy array otherwise.

    On the device the squared norms and the products are one fp64
    accumulation per entry over exact products, the metric is applied in fp64
    and rounded once: rows with identical values are at exactly 0, the
    diagonal is 0 and the matrix is symmetric bit for bit.  Without a GPU or
    with ``on_device=False`` the call is scikit-learn's on the host; beyond
    ``maximum_rows`` rows (at most 2^16), 2^20 features or a quarter of the
    free device memory the call says so and does the same."""
    given_device_tensor = isinstance(values, torch.Tensor) and values.is_cuda
    if on_device is None:
        use_device = torch.cuda.is_available()
    elif on_device and not torch.cuda.is_available():
        raise _lib.HipLibraryError(
            "No GPU visible: distances on the device need one.")
    else:
        use_device = bool(on_device)
    distances = None
    if use_device:
        try:
            distances = _device_distances(
                values, metric, rows, device,
                min(int(maximum_rows), MAXIMUM_ROWS_ON_DEVICE))
        except _HostFallback as reason:
            print("distances on the device not used: {}.".format(reason))
    if distances is None:
        distances = _host_distances(values, metric, rows)
        if given_device_tensor:
            return torch.from_numpy(distances).to(values.device)
        return distances
    return distances if given_device_tensor else distances.cpu().numpy()


def hierarchical_order(distances):
    """The order of the examples along the reference's dendrogram
    (``figures/matrices.py:191-206``): the leaves of
    ``scipy.cluster.hierarchy.linkage(squareform(distances, checks=False))``.
    The reference passes ``metric="average"``, which SciPy ignores for a
    condensed matrix, and no ``method``: the linkage is **single** linkage,
    and that is what is built here.  ``leaves_list`` gives the order of
    seaborn's ``reordered_ind`` (the ``leaves`` of
    ``dendrogram(no_plot=True)``) without recursion.  Runs on the host; the
    reference takes at most 1 000 examples here."""
    import scipy.cluster.hierarchy
    import scipy.spatial.distance
    if isinstance(distances, torch.Tensor):
        distances = distances.cpu().numpy()
    distances = numpy.asarray(distances)
    if distances.shape[0] < 2:
        return numpy.arange(distances.shape[0], dtype=numpy.int64)
    condensed = scipy.spatial.distance.squareform(distances, checks=False)
    linkage = scipy.cluster.hierarchy.linkage(condensed, method="single")
    return numpy.asarray(scipy.cluster.hierarchy.leaves_list(linkage),
                         dtype=numpy.int64)


def figure_name(version, metric, sorting_method):
    """``build_figure_name(["distances", version, metric, sorting method])``
    (``figures/saving.py:44-63`` as called from ``subanalyses.py:422-426``
    and ``matrices.py:104``)."""
    return "-".join(normalise_string(str(part)) for part in (
        "distances", version, metric, sorting_method) if part is not None)


def distance_matrices(values, labels=None, version=None, on_device=None,
                      device=None):
    """The loop of ``analyse_matrices(..., plot_distances=True)``
    (``subanalyses.py:313-315, 374-427``) over one set.  ``values``:
    ``[N, F]`` as ``pairwise_distances`` takes them; ``labels``: ``[N]`` or
    None; ``version``: the set's version, for the names.

    The sample is the head of ``RandomState(57).permutation(N)``: 1 000
    examples for hierarchical clustering and 10 000 otherwise, all examples in
    their own order where there are no more than that.  The sorting methods
    are "labels" (only with labels) and then "hierarchical_clustering", each
    with both metrics.  For "labels" the sorted order goes into the row index,
    so the matrix leaves the kernel sorted; for hierarchical clustering it is
    computed in sample order and permuted by ``hierarchical_order``.

    Returns a list of dicts: ``name``, ``metric``, ``sorting_method``,
    ``indices`` (into the set, in plotted order), ``distances`` (fp32
    ``[n, n]`` in plotted order, on the host), ``sample_size`` (None where
    all examples are taken) and ``duration``."""
    number_of_examples = int(values.shape[0])
    if labels is not None:
        labels = numpy.asarray(labels)
        if labels.shape[0] != number_of_examples:
            raise ValueError("Distances: {} labels for {} examples.".format(
                labels.shape[0], number_of_examples))
    shuffled_indices = numpy.random.RandomState(57).permutation(
        number_of_examples)
    sorting_methods = ["hierarchical_clustering"]
    if labels is not None:
        sorting_methods.insert(0, "labels")
    if (on_device is not False and torch.cuda.is_available()
            and not isinstance(values, torch.Tensor)):
        # made resident once for all the matrices of the set
        try:
            values = _resident(values, device)
        except _HostFallback as reason:
            print("distances on the device not used: {}.".format(reason))
            on_device = False
    matrices = []
    for sorting_method in sorting_methods:
        for metric in DISTANCE_METRICS:
            time_start = time()
            if (sorting_method == "hierarchical_clustering"
                    and number_of_examples
                    > MAXIMUM_NUMBER_OF_EXAMPLES_FOR_DENDROGRAM):
                sample_size = MAXIMUM_NUMBER_OF_EXAMPLES_FOR_DENDROGRAM
            elif (number_of_examples
                    > MAXIMUM_NUMBER_OF_EXAMPLES_FOR_HEAT_MAPS):
                sample_size = MAXIMUM_NUMBER_OF_EXAMPLES_FOR_HEAT_MAPS
            else:
                sample_size = None
            indices = numpy.arange(number_of_examples)
            if sample_size:
                indices = shuffled_indices[:sample_size]
            if sorting_method == "labels":
                indices = indices[numpy.argsort(labels[indices],
                                                kind="stable")]
            distances = pairwise_distances(
                values, metric=metric, rows=indices, on_device=on_device,
                device=device)
            if isinstance(distances, torch.Tensor):
                distances = distances.cpu().numpy()
            if sorting_method == "hierarchical_clustering":
                order = hierarchical_order(distances)
                distances = distances[order][:, order]
                indices = indices[order]
            matrices.append({
                "name": figure_name(version, metric, sorting_method),
                "version": version,
                "metric": metric,
                "sorting_method": sorting_method,
                "indices": numpy.asarray(indices, dtype=numpy.int64),
                "distances": distances,
                "sample_size": sample_size,
                "duration": time() - time_start,
            })
    return matrices


def evaluation_distances(reconstructed, latent_z=None, labels=None,
                         example_names=None, on_device=None):
    """What ``ModelBase.evaluate`` attaches (``analyses.py:1351-1362``): the
    distance matrices of the reconstructed set from ``reconstructed``
    (``[N, F]`` fp32 on the device, read in place) and, where ``latent_z`` is
    given, those of the ``z`` latent values.  Returns ``{"reconstructed":
    [...], "z": [...]}``; every matrix also carries the names and labels of
    its examples in plotted order (``example_names``, ``labels``; None where
    the set has none)."""
    result = {}
    for version, values in (("reconstructed", reconstructed),
                            ("z", latent_z)):
        if values is None:
            continue
        matrices = distance_matrices(values, labels=labels, version=version,
                                     on_device=on_device)
        for matrix in matrices:
            matrix["example_names"] = (
                numpy.asarray(example_names)[matrix["indices"]]
                if example_names is not None else None)
            matrix["labels"] = (
                numpy.asarray(labels)[matrix["indices"]]
                if labels is not None else None)
        result[version] = matrices
    return result


def write_distances(directory, result):
    """One matrix of ``distance_matrices`` as two files under ``directory``:
    ``<name>.npy``, the fp32 matrix in plotted order, and ``<name>.tsv`` with
    a row per position: ``position``, ``index`` (in the evaluation set),
    ``example`` and, where the set has labels, ``label``.  Returns the two
    paths."""
    os.makedirs(directory, exist_ok=True)
    matrix_path = os.path.join(directory, result["name"] + ".npy")
    table_path = os.path.join(directory, result["name"] + ".tsv")
    numpy.save(matrix_path, numpy.asarray(result["distances"],
                                          dtype=numpy.float32))
    names = result.get("example_names")
    labels = result.get("labels")
    with open(table_path, "w") as file:
        file.write("position\tindex\texample" + (
            "\tlabel" if labels is not None else "") + "\n")
        for position, index in enumerate(result["indices"]):
            fields = [str(position), str(int(index)),
                      str(names[position]) if names is not None else ""]
            if labels is not None:
                fields.append(str(labels[position]))
            file.write("\t".join(fields) + "\n")
    return matrix_path, table_path
