"""Value preprocessing of a data set (``scvae/data/processing.py:305-333,
496-522``): the encoder input x may be a transformed copy of the counts, the
likelihood always sees the counts themselves (or, for the Bernoulli likelihood,
their binarisation).  Element-wise NumPy / SciPy work on the host, once per
data set; sparse matrices stay sparse (every method maps 0 to 0).

Feature selection and example filters (``scvae/data/processing.py:95-302``):
``select_features`` and ``filter_examples`` with the reference's signatures,
printed lines and errors.  For a sparse matrix of integer counts the per-gene
moments come from one pass of ``csrc/selection.hip`` over the CSR on the
device and the selected sub-matrix from its two sub-matrix kernels; the same
functions have a host path that returns the same bits.

What differs from the reference on purpose: the reference takes the variances
as fp32 ``E[x^2] - E[x]^2`` and orders them with an unstable sort; here
``N sum x^2 - (sum x)^2`` is an exact integer and ties go to the higher gene
index (``numpy.argsort(kind="stable")[-k:]``).  And the example filter ``keep``
returns the kept rows in ascending order, where the reference iterates a
Python ``set``."""
import ctypes
from functools import reduce
from time import time

import numpy
import scipy.sparse

from scvae_amd.data.sparse import SparseRowMatrix
from scvae_amd.utilities import format_duration, normalise_string

PREPROCESSERS = {}


def _register(name):
    def decorator(function):
        PREPROCESSERS[name] = function
        return function
    return decorator


def _on_values(values, function):
    if scipy.sparse.issparse(values):
        result = values.copy().astype(numpy.float32)
        result.data = function(result.data).astype(numpy.float32)
        result.eliminate_zeros()
        return result
    return function(numpy.asarray(values, dtype=numpy.float32)).astype(
        numpy.float32)


@_register("log")
def _log(values):
    return _on_values(values, numpy.log1p)


@_register("exp")
def _exp(values):
    return _on_values(values, numpy.expm1)


@_register("normalise")
def _normalise(values):
    """Every feature (column) scaled to unit l2 norm
    (``sklearn.preprocessing.normalize(values, norm="l2", axis=0)``)."""
    if scipy.sparse.issparse(values):
        values = scipy.sparse.csr_matrix(values, dtype=numpy.float32)
        norms = numpy.sqrt(numpy.asarray(
            values.multiply(values).sum(axis=0))).reshape(-1)
    else:
        values = numpy.asarray(values, dtype=numpy.float32)
        norms = numpy.sqrt((values * values).sum(axis=0))
    scale = numpy.where(norms > 0, 1.0 / numpy.maximum(norms, 1e-30), 1.0)
    if scipy.sparse.issparse(values):
        return scipy.sparse.csr_matrix(
            values.multiply(scale.reshape(1, -1)), dtype=numpy.float32)
    return (values * scale).astype(numpy.float32)


@_register("binarise")
def _binarise(values):
    """``sklearn.preprocessing.binarize(values, threshold=0.5)``."""
    return _on_values(values, lambda v: (v > 0.5).astype(numpy.float32))


@_register("bernoulli_sample")
def _bernoulli_sample(values):
    """A Bernoulli draw per value, the value its probability
    (``scvae/data/processing.py:516-522``: what "binarise" means when the
    preprocessing is noisy -- a new sample of the data set every epoch).
    NumPy's global generator, as in the reference: the draws of a run follow
    ``numpy.random.seed``."""
    def draw(probabilities):
        probabilities = numpy.asarray(probabilities, dtype=numpy.float64)
        if probabilities.size and (probabilities.min() < 0
                                   or probabilities.max() > 1):
            raise ValueError(
                "Bernoulli sampling needs values in [0, 1]; found [{:g}, {:g}]."
                .format(probabilities.min(), probabilities.max()))
        return numpy.random.binomial(1, probabilities)
    return _on_values(values, draw)


def build_preprocessor(preprocessing_methods, noisy=False):
    preprocessers = []
    for method in preprocessing_methods or []:
        if noisy and method == "binarise":
            method = "bernoulli_sample"
        if method not in PREPROCESSERS:
            raise ValueError(
                "Preprocessing method `{}` not found.".format(method))
        preprocessers.append(PREPROCESSERS[method])

    def preprocess(values):
        return reduce(lambda v, p: p(v), preprocessers, values)
    return preprocess


# -- feature selection and example filters (processing.py:95-302) -------------

#: limits of ``scvae_csr_feature_moments`` (``include/scvae_hip.h``): with them
#: ``sum x^2 <= 2^31 * 2^32`` of a gene stays inside 64 bits
MAXIMUM_NUMBER_OF_EXAMPLES = 2 ** 31 - 1
MAXIMUM_NUMBER_OF_FEATURES = 2 ** 20
MAXIMUM_COUNT = 65535
#: rows of a block of the host moments: 2^20 values below 2^32 add up to less
#: than 2^53, so the fp64 sums ``numpy.bincount`` takes are exact integers
_HOST_ROW_BLOCK = 2 ** 20
#: (processing.py:199, 206)
MACOSKO_NUMBER_OF_NON_ZERO_ELEMENTS = 900
#: whether ``on_device=None`` takes the device where it can (DESIGN.md 6i:
#: the whole device call against the host path at 68 579 x 32 738)
DEVICE_BY_DEFAULT = True

FEATURE_SELECTIONS = ("remove_zeros", "keep_variances_above",
                      "keep_highest_variances")
EXAMPLE_FILTERS = ("macosko", "inverse_macosko", "keep", "remove",
                   "excluded_classes", "remove_count_sum_above", "random")


def _canonical(values):
    """A sparse matrix as fp32 CSR with the duplicates summed and the indices
    sorted (what ``DeviceCSR.from_scipy`` uploads); a dense one as it is."""
    if not scipy.sparse.issparse(values):
        return numpy.asarray(values)
    matrix = values.tocsr()
    if matrix.dtype != numpy.float32:
        matrix = matrix.astype(numpy.float32)
    if not matrix.has_canonical_format:
        matrix = matrix.copy()
        matrix.sum_duplicates()
    return matrix


def _is_integer_counts(data):
    data = numpy.asarray(data)
    if data.size == 0:
        return True
    if data.dtype.kind not in "iuf":
        return False
    with numpy.errstate(invalid="ignore"):
        return bool(((data >= 0) & (data <= MAXIMUM_COUNT)
                     & (data == numpy.trunc(data))).all())


def _within_limits(shape):
    return (1 <= shape[0] <= MAXIMUM_NUMBER_OF_EXAMPLES
            and 1 <= shape[1] <= MAXIMUM_NUMBER_OF_FEATURES)


def _host_integer_moments(matrix):
    """``sum x``, ``sum x^2`` (uint64) and the number of values != 0 (int64)
    of every column of a canonical CSR matrix of integer counts."""
    n_examples, n_features = matrix.shape
    sums = numpy.zeros(n_features, dtype=numpy.uint64)
    squares = numpy.zeros(n_features, dtype=numpy.uint64)
    nonzeros = numpy.zeros(n_features, dtype=numpy.int64)
    for first in range(0, n_examples, _HOST_ROW_BLOCK):
        last = min(first + _HOST_ROW_BLOCK, n_examples)
        begin, end = int(matrix.indptr[first]), int(matrix.indptr[last])
        columns = matrix.indices[begin:end]
        data = matrix.data[begin:end].astype(numpy.float64)
        sums += numpy.bincount(
            columns, weights=data, minlength=n_features).astype(numpy.uint64)
        squares += numpy.bincount(
            columns, weights=data * data,
            minlength=n_features).astype(numpy.uint64)
        nonzeros += numpy.bincount(
            columns[data != 0], minlength=n_features).astype(numpy.int64)
    return sums, squares, nonzeros


def _float_column_moments(values):
    """Column sums and population variances in fp64, the variances from a
    second pass over the deviations from the mean (a dense array, or a
    canonical CSR matrix whose absent entries count as zeros)."""
    n_examples, n_features = values.shape
    if not scipy.sparse.issparse(values):
        values = numpy.asarray(values, dtype=numpy.float64)
        sums = values.sum(axis=0)
        deviations = values - sums / n_examples
        return sums, (deviations * deviations).sum(axis=0) / n_examples
    data = values.data.astype(numpy.float64)
    sums = numpy.bincount(values.indices, weights=data, minlength=n_features)
    means = sums / n_examples
    deviations = data - means[values.indices]
    stored = numpy.bincount(values.indices, minlength=n_features)
    m2 = numpy.bincount(values.indices, weights=deviations * deviations,
                        minlength=n_features)
    m2 += (n_examples - stored) * means * means
    return sums, m2 / n_examples


def _gpu_present():
    try:
        import torch
    except ImportError:
        return False
    return bool(torch.cuda.is_available())


def _pointer(tensor):
    return ctypes.c_void_p(tensor.data_ptr() if tensor is not None else None)


class _DeviceMatrix:
    """A canonical CSR matrix uploaded once: int64 ``indptr``, int32
    ``indices``, fp32 ``values``."""

    def __init__(self, matrix, device):
        import torch
        self.shape = matrix.shape
        self.device = device
        self.indptr = torch.from_numpy(
            matrix.indptr.astype(numpy.int64, copy=False)).to(device)
        self.indices = torch.from_numpy(
            matrix.indices.astype(numpy.int32, copy=False)).to(device)
        self.values = torch.from_numpy(
            matrix.data.astype(numpy.float32, copy=False)).to(device)


class _Placement:
    """Where one call does its work: decides once between the device and the
    host, says why the device is not used when a GPU is present, and keeps
    what it uploaded."""

    def __init__(self, what, on_device):
        self.what = what
        self.on_device = on_device
        self.decided = None
        self.uploaded = {}
        self.library = None
        self.device = None

    def _reason(self, matrices):
        if not _gpu_present():
            return "no GPU is visible"
        try:
            from scvae_amd import _lib
            self.library = _lib.load()
        except (OSError, AttributeError, RuntimeError) as error:
            return "the library of kernels does not load ({})".format(error)
        import torch
        self.device = torch.device("cuda", torch.cuda.current_device())
        needed = 0
        for matrix in matrices:
            if matrix is None:
                continue
            if not scipy.sparse.issparse(matrix):
                return "the values are a dense array"
            if not _within_limits(matrix.shape):
                return ("the matrix is outside 1 to 2^31 - 1 examples and "
                        "1 to 2^20 features")
            # the three arrays of the input and as much again for the result
            needed += 2 * (8 * matrix.nnz + 8 * (matrix.shape[0] + 1))
            needed += 32 * matrix.shape[1]
        free = torch.cuda.mem_get_info(self.device)[0]
        if needed > free // 4:
            return ("input and output take {} bytes, more than a quarter of "
                    "the {} free bytes of device memory".format(needed, free))
        return None

    def _not_used(self, reason):
        if self.on_device:
            from scvae_amd import _lib
            raise _lib.HipLibraryError(
                "{} on the device not possible: {}.".format(
                    self.what.capitalize(), reason))
        if _gpu_present():
            print("{} on the device not used: {}.".format(self.what, reason))
        self.decided = False
        return False

    def use_device(self, matrices):
        if self.decided is None:
            if self.on_device is False or (
                    self.on_device is None and not DEVICE_BY_DEFAULT):
                self.decided = False
            else:
                reason = self._reason(matrices)
                self.decided = (True if reason is None
                                else self._not_used(reason))
        return self.decided

    def fall_back(self, reason):
        return self._not_used(reason)

    def upload(self, matrix):
        key = id(matrix)
        if key not in self.uploaded:
            self.uploaded[key] = (matrix, _DeviceMatrix(matrix, self.device))
        return self.uploaded[key][1]

    def stream(self):
        import torch
        return ctypes.c_void_p(
            torch.cuda.current_stream(self.device).cuda_stream)


def _device_moments(placement, matrix):
    """The moments of a canonical CSR matrix from the kernel, and its ``bad``
    word."""
    import torch
    from scvae_amd import _lib
    uploaded = placement.upload(matrix)
    n_examples, n_features = matrix.shape
    # uint64 as the bits of int64 tensors: every value is below 2^63
    results = torch.empty(3, n_features, dtype=torch.int64,
                          device=placement.device)
    bad = torch.zeros(1, dtype=torch.int32, device=placement.device)
    with torch.cuda.device(placement.device):
        _lib.check(placement.library.scvae_csr_feature_moments(
            _pointer(uploaded.indptr), _pointer(uploaded.indices),
            _pointer(uploaded.values), n_examples, n_features,
            _pointer(results[0]), _pointer(results[1]), _pointer(results[2]),
            _pointer(bad), placement.stream()), "scvae_csr_feature_moments")
    results = results.cpu().numpy()
    return (results[0].view(numpy.uint64), results[1].view(numpy.uint64),
            results[2].copy(), int(bad.item()))


def _device_submatrix(placement, matrix, rows, columns):
    import torch
    from scvae_amd import _lib
    uploaded = placement.upload(matrix)
    device = placement.device
    n_examples, n_features = matrix.shape
    n_out, n_columns = n_examples, n_features
    row_list = column_map = None
    if rows is not None:
        n_out = len(rows)
        row_list = torch.from_numpy(
            numpy.ascontiguousarray(rows, dtype=numpy.int64)).to(device)
    if columns is not None:
        n_columns = len(columns)
        host_map = numpy.full(n_features, -1, dtype=numpy.int32)
        host_map[columns] = numpy.arange(n_columns, dtype=numpy.int32)
        column_map = torch.from_numpy(host_map).to(device)
    counts = torch.empty(n_out, dtype=torch.int64, device=device)
    out_indptr = torch.zeros(n_out + 1, dtype=torch.int64, device=device)
    bad = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(placement.library.scvae_csr_submatrix_count(
            _pointer(uploaded.indptr), _pointer(uploaded.indices), n_examples,
            n_features, _pointer(row_list), n_out, _pointer(column_map),
            _pointer(counts), _pointer(bad), placement.stream()),
            "scvae_csr_submatrix_count")
        torch.cumsum(counts, dim=0, out=out_indptr[1:])
        kept = int(out_indptr[-1].item())
        out_indices = torch.empty(kept, dtype=torch.int32, device=device)
        out_values = torch.empty(kept, dtype=torch.float32, device=device)
        _lib.check(placement.library.scvae_csr_submatrix_fill(
            _pointer(uploaded.indptr), _pointer(uploaded.indices),
            _pointer(uploaded.values), n_examples, n_features,
            _pointer(row_list), n_out, _pointer(column_map),
            _pointer(out_indptr), _pointer(out_indices), _pointer(out_values),
            _pointer(bad), placement.stream()), "scvae_csr_submatrix_fill")
    if int(bad.item()):
        raise _lib.HipLibraryError(
            "Sub-matrix on the device: the CSR arrays are not consistent "
            "(flags {}).".format(int(bad.item())))
    return _as_result(out_values.cpu().numpy(), out_indices.cpu().numpy(),
                      out_indptr.cpu().numpy(), (n_out, n_columns))


def _as_result(data, indices, indptr, shape):
    """A ``SparseRowMatrix`` from the three arrays, with the index type SciPy
    gives a matrix of this size: both paths end here."""
    largest = max(len(data), shape[0], shape[1])
    index_type = (numpy.int32 if largest <= numpy.iinfo(numpy.int32).max
                  else numpy.int64)
    return SparseRowMatrix(
        (numpy.asarray(data, dtype=numpy.float32),
         numpy.asarray(indices, dtype=index_type),
         numpy.asarray(indptr, dtype=index_type)), shape=shape)


def _row_indices(rows, n_examples):
    rows = numpy.asarray(rows)
    if rows.dtype == bool:
        if rows.shape != (n_examples,):
            raise IndexError("A row mask of {} examples expected.".format(
                n_examples))
        return numpy.flatnonzero(rows).astype(numpy.int64)
    rows = rows.reshape(-1).astype(numpy.int64)
    rows = numpy.where(rows < 0, rows + n_examples, rows)
    if rows.size and (rows.min() < 0 or rows.max() >= n_examples):
        raise IndexError("Row index outside the {} examples.".format(
            n_examples))
    return rows


def _column_indices(columns, n_features):
    columns = numpy.asarray(columns)
    if columns.dtype == bool:
        if columns.shape != (n_features,):
            raise IndexError("A column mask of {} features expected.".format(
                n_features))
        return numpy.flatnonzero(columns).astype(numpy.int64)
    columns = columns.reshape(-1).astype(numpy.int64)
    if columns.size and (columns.min() < 0 or columns.max() >= n_features):
        raise IndexError("Column index outside the {} features.".format(
            n_features))
    if columns.size > 1 and not (numpy.diff(columns) > 0).all():
        raise ValueError("Column indices in ascending order expected.")
    return columns


def _submatrix(placement, values, rows, columns):
    if values is None:
        return None
    if rows is not None:
        rows = _row_indices(rows, values.shape[0])
    if columns is not None:
        columns = _column_indices(columns, values.shape[1])
    matrix = _canonical(values)
    if not scipy.sparse.issparse(matrix):
        placement.use_device([matrix])
        if rows is not None:
            matrix = matrix[rows]
        if columns is not None:
            matrix = matrix[:, columns]
        return matrix
    if placement.use_device([matrix]):
        return _device_submatrix(placement, matrix, rows, columns)
    if rows is not None:
        matrix = matrix[rows]
    if columns is not None:
        matrix = matrix[:, columns]
    return _as_result(matrix.data, matrix.indices, matrix.indptr,
                      matrix.shape)


def submatrix(values, rows=None, columns=None, on_device=None):
    """``values[rows][:, columns]`` as a CSR matrix: ``rows`` a list of row
    indices in any order (or a mask), ``columns`` ascending column indices (or
    a mask); ``None`` keeps all.  The matrix is put in canonical form first
    (duplicates summed, indices sorted); the entries of a row keep their
    order and explicitly stored zeros stay.  On the device
    (``scvae_csr_submatrix_count`` / ``_fill``) or on the host with SciPy,
    with the same arrays as the result.  A dense array is indexed on the
    host."""
    return _submatrix(_Placement("sub-matrix", on_device), values, rows,
                      columns)


def _integer_moments(placement, matrix):
    """The exact moments of a canonical CSR matrix, or ``None`` where it is
    not one of integer counts within the limits."""
    if not scipy.sparse.issparse(matrix) or not _within_limits(matrix.shape):
        placement.use_device([matrix])
        return None
    if placement.use_device([matrix]):
        if matrix.nnz == 0:
            zeros = numpy.zeros(matrix.shape[1], dtype=numpy.uint64)
            return zeros, zeros.copy(), zeros.astype(numpy.int64)
        sums, squares, nonzeros, bad = _device_moments(placement, matrix)
        if bad & ~1:
            from scvae_amd import _lib
            raise _lib.HipLibraryError(
                "Feature moments on the device: the CSR arrays are not "
                "consistent (flags {}).".format(bad))
        if not bad:
            return sums, squares, nonzeros
        placement.fall_back(
            "the values are not integer counts in [0, {}]".format(
                MAXIMUM_COUNT))
        return None
    if not _is_integer_counts(matrix.data):
        return None
    return _host_integer_moments(matrix)


def feature_moments(values, on_device=None):
    """``sum x``, ``sum x^2`` (uint64) and the number of values != 0 (int64)
    of every feature of a matrix of integer counts in [0, 65 535], as exact
    integers: ``N sum x^2 - (sum x)^2`` is ``N^2`` times the population
    variance.  From ``scvae_csr_feature_moments`` on the device or from
    ``numpy.bincount`` over row blocks on the host; the same numbers."""
    placement = _Placement("feature moments", on_device)
    matrix = _canonical(values)
    if not scipy.sparse.issparse(matrix):
        if not _is_integer_counts(matrix):
            raise ValueError("Feature moments: integer counts in [0, {}] "
                             "expected.".format(MAXIMUM_COUNT))
        placement.use_device([matrix])
        matrix = _canonical(scipy.sparse.csr_matrix(
            matrix, dtype=numpy.float32))
        return _host_integer_moments(matrix)
    moments = _integer_moments(placement, matrix)
    if moments is None:
        raise ValueError(
            "Feature moments: integer counts in [0, {}] in a matrix of 1 to "
            "2^31 - 1 examples and 1 to 2^20 features expected.".format(
                MAXIMUM_COUNT))
    return moments


def variance_numerators(sums, squares, n_examples):
    """``N sum x^2 - (sum x)^2`` of every feature as Python integers."""
    n_examples = int(n_examples)
    return [n_examples * int(q) - int(s) * int(s)
            for s, q in zip(sums.tolist(), squares.tolist())]


def _highest(keys, number_to_keep):
    """The last ``number_to_keep`` of the ascending order by (key, index), in
    ascending index order: ``numpy.argsort(kind="stable")[-k:]``, sorted."""
    order = sorted(range(len(keys)), key=lambda j: (keys[j], j))
    return numpy.sort(numpy.asarray(order, dtype=numpy.int64)[
        -number_to_keep:])


def select_features(values_dictionary, feature_names, method=None,
                    parameters=None, on_device=None):
    """``processing.py:95-166``.  ``on_device``: ``None`` takes the device
    where it can, ``True`` raises where it cannot, ``False`` stays on the
    host."""
    method = normalise_string(method)

    print("Selecting features.")
    start_time = time()

    if not isinstance(values_dictionary, dict):
        values_dictionary = {"original": values_dictionary}
    values = values_dictionary["original"]
    n_examples, n_features = values.shape

    if method not in FEATURE_SELECTIONS:
        raise ValueError(
            "Feature selection `{}` not found.".format(method))

    placement = _Placement("feature selection", on_device)
    versions = {version: (_canonical(v) if v is not None else None)
                for version, v in values_dictionary.items()}
    original = versions["original"]
    placement.use_device(list(versions.values()))
    moments = _integer_moments(placement, original)
    if moments is not None:
        sums, squares, _ = moments
        if method != "remove_zeros":
            variances = variance_numerators(sums, squares, n_examples)
            denominator = n_examples * n_examples
    else:
        sums, variances = _float_column_moments(original)
        variances = variances.tolist()
        denominator = 1

    if method == "remove_zeros":
        indices = numpy.asarray(sums != 0)
    elif method == "keep_variances_above":
        threshold = float(parameters[0]) if parameters else 0.5
        indices = numpy.asarray(
            [v / denominator > threshold for v in variances], dtype=bool)
    else:
        number_to_keep = (int(parameters[0]) if parameters
                          else int(n_examples / 2))
        indices = _highest(variances, number_to_keep)

    error = Exception(
        "No features excluded using feature selection {}.".format(method))
    if indices.dtype == "bool" and all(indices):
        raise error
    elif indices.dtype != "bool" and len(indices) == n_features:
        raise error

    feature_selected_values = {
        version: _submatrix(placement, v, None, indices)
        for version, v in versions.items()}
    feature_selected_feature_names = (
        feature_names[indices] if feature_names is not None else None)
    n_features_changed = (int(indices.sum()) if indices.dtype == "bool"
                          else len(indices))

    duration = time() - start_time
    print("{} features selected, {} excluded ({}).".format(
        n_features_changed, n_features - n_features_changed,
        format_duration(duration)))

    return feature_selected_values, feature_selected_feature_names


def filter_examples(values_dictionary, example_names, method=None,
                    parameters=None, labels=None, excluded_classes=None,
                    superset_labels=None, excluded_superset_classes=None,
                    batch_indices=None, count_sum=None, on_device=None):
    """``processing.py:169-302``; ``keep`` returns its rows in ascending
    order.  ``on_device`` as for ``select_features``."""
    print("Filtering examples.")
    start_time = time()

    method = normalise_string(method)

    if superset_labels is not None:
        filter_labels = numpy.asarray(superset_labels).copy()
        filter_excluded_classes = excluded_superset_classes
    elif labels is not None:
        filter_labels = numpy.asarray(labels).copy()
        filter_excluded_classes = excluded_classes
    else:
        filter_labels = None
        filter_excluded_classes = None

    if not isinstance(values_dictionary, dict):
        values_dictionary = {"original": values_dictionary}
    values = values_dictionary["original"]
    n_examples, n_features = values.shape

    filter_indices = numpy.arange(n_examples)

    if method in ("macosko", "inverse_macosko"):
        number_of_non_zero_elements = numpy.asarray(
            (values != 0).sum(axis=1)).reshape(-1)
        if method == "macosko":
            filter_indices = numpy.nonzero(
                number_of_non_zero_elements
                > MACOSKO_NUMBER_OF_NON_ZERO_ELEMENTS)[0]
        else:
            filter_indices = numpy.nonzero(
                number_of_non_zero_elements
                <= MACOSKO_NUMBER_OF_NON_ZERO_ELEMENTS)[0]

    elif method in ("keep", "remove", "excluded_classes"):
        if filter_labels is None:
            raise ValueError(
                "Cannot filter examples based on labels, "
                "since data set is unlabelled.")
        if method == "excluded_classes":
            method = "remove"
            parameters = filter_excluded_classes
        filter_class_names = numpy.unique(filter_labels)
        named = numpy.zeros(n_examples, dtype=bool)
        for parameter in parameters or []:
            normalised_parameter = normalise_string(str(parameter))
            for class_name in filter_class_names:
                if normalise_string(str(class_name)) == normalised_parameter:
                    named |= filter_labels == class_name
        filter_indices = filter_indices[named if method == "keep"
                                        else ~named]

    elif method == "remove_count_sum_above":
        threshold = int(parameters[0])
        filter_indices = filter_indices[
            numpy.asarray(count_sum).reshape(-1) <= threshold]

    elif method == "random":
        n_samples = min(int(parameters[0]), n_examples)
        random_state = numpy.random.RandomState(90)
        filter_indices = random_state.permutation(n_examples)[:n_samples]

    else:
        raise ValueError(
            "Example filter `{}` not found.".format(method))

    if method and len(filter_indices) == n_examples:
        raise Exception(
            "No examples filtered out using example filter `{}`."
            .format(method))

    placement = _Placement("example filter", on_device)
    versions = {version: (_canonical(v) if v is not None else None)
                for version, v in values_dictionary.items()}
    placement.use_device(list(versions.values()))
    example_filtered_values = {
        version: _submatrix(placement, v, filter_indices, None)
        for version, v in versions.items()}

    example_filtered_example_names = (
        example_names[filter_indices] if example_names is not None else None)
    example_filtered_labels = (
        labels[filter_indices] if labels is not None else None)
    example_filtered_batch_indices = (
        batch_indices[filter_indices] if batch_indices is not None else None)

    n_examples_changed = len(filter_indices)

    duration = time() - start_time
    print("{} examples filtered out, {} remaining ({}).".format(
        n_examples - n_examples_changed, n_examples_changed,
        format_duration(duration)))

    return (example_filtered_values, example_filtered_example_names,
            example_filtered_labels, example_filtered_batch_indices)
