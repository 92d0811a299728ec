"""Decompositions of data sets: the two-component PCA behind the scatter
plots of ``analyse_results`` (``scvae/analyses/analyses.py:1237-1280``,
``subanalyses.py:471-709``, ``decomposition/decomposition.py:44-167``).

Where the reference leaves exact PCA -- more than 2000 features, or a sparse
matrix -- it fits ``IncrementalPCA(batch_size=100)`` on the host
(``decomposition.py:66-73``).  Here that case runs on the device: block
subspace iteration with Rayleigh-Ritz extraction over the kernels of
``csrc/pca.hip``, which read the fp32 matrix where it lies, subtract the
column means per element in fp64 and accumulate in fp64 on the matrix cores.

What differs from the reference on purpose: the device path returns the
converged exact PCA of the matrix, not IncrementalPCA's approximation, which
depends on the order of the batches.

The loop (``subspace_iteration``) is written against an operator with
``shape``, ``moments()``, ``project(q)`` and ``back_project(y)``;
``NumpyOperator`` is the fp64 host model of ``DeviceOperator``.  The small
algebra -- the QR factorisation of the ``F x b`` block and the ``b x b``
symmetric eigenproblem -- is NumPy's LAPACK in fp64 on the host: the kernels
sum in one fixed order, so a seeded fit gives the same bits on every run.
"""
import ctypes
from time import time

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.kmeans import _ptr
from scvae_amd.defaults import defaults
from scvae_amd.utilities import normalise_string

DECOMPOSITION_METHOD_NAMES = {
    "PCA": ["pca"],
    "SVD": ["svd"],
    "ICA": ["ica"],
    "t-SNE": ["t_sne", "tsne"]
}
DECOMPOSITION_METHOD_LABEL = {
    "PCA": "PC",
    "SVD": "SVD",
    "ICA": "IC",
    "t-SNE": "tSNE"
}

MAXIMUM_FEATURE_SIZE_FOR_NORMAL_PCA = 2000

MAXIMUM_BLOCK_SIZE = 32
MAXIMUM_NUMBER_OF_FEATURES = 2 ** 20
MAXIMUM_NUMBER_OF_ROWS = 2 ** 31 - 1
#: rows of a block in which a sparse matrix is densified
_DENSIFY_ROWS = 2048


def _is_sparse(x):
    return hasattr(x, "tocsr") and not isinstance(x, numpy.ndarray)


def method_name(method):
    """The key of ``DECOMPOSITION_METHOD_NAMES`` that ``method`` spells (the
    string itself where there is none)."""
    normalised = normalise_string(str(method))
    for name, spellings in DECOMPOSITION_METHOD_NAMES.items():
        if normalised == normalise_string(name) or normalised in spellings:
            return name
    return method


def limit_reason(number_of_rows, number_of_features, number_of_components=2,
                 block_size=16):
    """Why these sizes are outside what the kernels take (``None``: they are
    inside)."""
    n, f = int(number_of_rows), int(number_of_features)
    c, b = int(number_of_components), int(block_size)
    if not 1 <= f <= MAXIMUM_NUMBER_OF_FEATURES:
        return "{} features (1 to {} supported)".format(
            f, MAXIMUM_NUMBER_OF_FEATURES)
    if not 2 <= n <= MAXIMUM_NUMBER_OF_ROWS:
        return "{} examples (2 to 2^31 - 1 supported)".format(n)
    if not 1 <= c <= MAXIMUM_BLOCK_SIZE:
        return "{} components (1 to {} supported)".format(
            c, MAXIMUM_BLOCK_SIZE)
    if not c <= b <= MAXIMUM_BLOCK_SIZE:
        return "a block of {} vectors ({} to {} supported)".format(
            b, c, MAXIMUM_BLOCK_SIZE)
    if min(b, n - 1, f) < c:
        return "{} components from {} examples with {} features".format(
            c, n, f)
    return None


def flip_signs(components):
    """For each component (a row) the loading of largest magnitude positive,
    the lowest index on ties: scikit-learn's
    ``svd_flip(u_based_decision=False)``.  Returns the signs."""
    components = numpy.asarray(components)
    index = numpy.argmax(numpy.abs(components), axis=1)
    signs = numpy.sign(components[numpy.arange(components.shape[0]), index])
    signs[signs == 0] = 1.0
    return signs


class NumpyOperator:
    """The fp64 host model of ``DeviceOperator``."""

    def __init__(self, values):
        if _is_sparse(values):
            values = values.toarray()
        self.values = numpy.asarray(values, dtype=numpy.float64)
        if self.values.ndim != 2:
            raise ValueError("Expected a matrix, got shape {}.".format(
                self.values.shape))
        self.shape = self.values.shape
        self.mean = None

    def moments(self):
        self.mean = self.values.mean(axis=0)
        self.centred = self.values - self.mean
        return self.mean, float((self.centred ** 2).sum())

    def project(self, q, values=None):
        if values is None:
            return self.centred @ q
        if _is_sparse(values):
            values = values.toarray()
        return (numpy.asarray(values, dtype=numpy.float64) - self.mean) @ q

    def back_project(self, y):
        return self.centred.T @ y

    def to_host(self, y):
        return y

    def release(self):
        pass


class DeviceOperator:
    """An fp32 matrix on the device and the three passes over it.  ``values``:
    an fp32 device tensor (read where it lies, a row pitch is honoured), a
    NumPy array, or a SciPy sparse matrix, densified once to resident fp32."""

    def __init__(self, values, device=None):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(
                "No GPU visible: the device decomposition has no CPU path.")
        self.lib = _lib.load()
        if device is None and isinstance(values, torch.Tensor) and (
                values.is_cuda):
            device = values.device
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.values = self._resident(values)
        self.shape = tuple(int(s) for s in self.values.shape)
        reason = limit_reason(*self.shape, 1, 1)
        if reason:
            raise ValueError("Decomposition on the device: {}.".format(reason))
        self.mean = None
        self.workspace = None

    def _resident(self, values):
        if isinstance(values, torch.Tensor):
            if values.dtype != torch.float32 or values.dim() != 2:
                raise ValueError(
                    "Decomposition: a float32 matrix expected, got {} of "
                    "shape {}.".format(values.dtype, tuple(values.shape)))
            values = values.to(self.device)
            if values.shape[1] > 1 and values.stride(1) != 1:
                values = values.contiguous()
            return values
        shape = tuple(values.shape)
        if len(shape) != 2:
            raise ValueError("Decomposition: a matrix expected, got shape "
                             "{}.".format(shape))
        reason = memory_limit_reason(shape, self.device)
        if reason:
            raise ValueError("Decomposition on the device: {}.".format(reason))
        if _is_sparse(values):
            from scvae_amd.minibatch import DeviceCSR
            return densify(DeviceCSR.from_scipy(values, self.device))
        values = numpy.ascontiguousarray(values, dtype=numpy.float32)
        if not values.flags.writeable:
            values = values.copy()
        return torch.from_numpy(values).to(self.device)

    def _stream(self):
        return ctypes.c_void_p(
            torch.cuda.current_stream(self.device).cuda_stream)

    def _pitch(self, values):
        return values.stride(0) if values.shape[0] > 1 else values.shape[1]

    def _workspace(self, rows, block):
        size = self.lib.scvae_pca_workspace_bytes(rows, self.shape[1], block)
        if size < 0:
            _lib.check(-1, "scvae_pca_workspace_bytes")
        if self.workspace is None or self.workspace.numel() < size:
            self.workspace = torch.empty(max(size, 8), dtype=torch.uint8,
                                         device=self.device)
        return self.workspace

    def moments(self):
        rows, features = self.shape
        self.mean = torch.empty(features, dtype=torch.float64,
                                device=self.device)
        total = torch.empty(1, dtype=torch.float64, device=self.device)
        workspace = self._workspace(rows, 1)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_pca_moments(
                _ptr(self.values), self._pitch(self.values), rows, features,
                _ptr(self.mean), _ptr(total), _ptr(workspace),
                workspace.numel(), self._stream()), "scvae_pca_moments")
        return self.mean.cpu().numpy(), float(total.item())

    def _block(self, q, rows):
        q = numpy.ascontiguousarray(q, dtype=numpy.float64)
        if q.ndim != 2 or q.shape[0] != rows or not (
                1 <= q.shape[1] <= MAXIMUM_BLOCK_SIZE):
            raise ValueError(
                "A [{}, b] block with b <= {} expected, got shape {}.".format(
                    rows, MAXIMUM_BLOCK_SIZE, q.shape))
        return torch.from_numpy(q).to(self.device)

    def project(self, q, values=None):
        """``(values - 1 mean^T) q`` as a device tensor (``values``: the
        matrix itself when None, else another set with the same features)."""
        if self.mean is None:
            raise RuntimeError("moments() comes first.")
        if values is None:
            values = self.values
        else:
            values = DeviceOperator._resident(self, values)
            if values.shape[1] != self.shape[1]:
                raise ValueError(
                    "{} features expected, got {}.".format(
                        self.shape[1], values.shape[1]))
        q = self._block(q, self.shape[1])
        rows = int(values.shape[0])
        y = torch.empty(rows, q.shape[1], dtype=torch.float64,
                        device=self.device)
        if rows == 0:
            return y
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_pca_project(
                _ptr(values), self._pitch(values), rows, self.shape[1],
                _ptr(self.mean), _ptr(q), q.shape[1], _ptr(y),
                self._stream()), "scvae_pca_project")
        return y

    def back_project(self, y):
        if self.mean is None:
            raise RuntimeError("moments() comes first.")
        rows, features = self.shape
        if not isinstance(y, torch.Tensor):
            y = self._block(y, rows)
        block = int(y.shape[1])
        z = torch.empty(features, block, dtype=torch.float64,
                        device=self.device)
        workspace = self._workspace(rows, block)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_pca_back_project(
                _ptr(self.values), self._pitch(self.values), rows, features,
                _ptr(self.mean), _ptr(y), block, _ptr(z), _ptr(workspace),
                workspace.numel(), self._stream()), "scvae_pca_back_project")
        return z.cpu().numpy()

    def to_host(self, y):
        return y.cpu().numpy()

    def release(self):
        """Let go of the matrix (``project`` of other sets still works)."""
        self.values = None
        self.workspace = None


def memory_limit_reason(shape, device):
    """A matrix that is made resident must fit within a quarter of the free
    device memory."""
    needed = 4 * int(shape[0]) * int(shape[1])
    free, _ = torch.cuda.mem_get_info(device)
    if needed > free // 4:
        return ("{:.1f} GB of dense float32 values against {:.1f} GB of free "
                "device memory (a quarter of it at most)".format(
                    needed / 1e9, free / 1e9))
    return None


def densify(csr):
    """The rows of a ``DeviceCSR`` as one resident fp32 matrix."""
    rows, features = csr.shape
    out = torch.empty(rows, features, dtype=torch.float32, device=csr.device)
    for first in range(0, rows, _DENSIFY_ROWS):
        last = min(first + _DENSIFY_ROWS, rows)
        index = torch.arange(first, last, dtype=torch.int64,
                             device=csr.device)
        csr.gather_dense(index, out=out[first:last])
    return out


def subspace_iteration(operator, number_of_components=2, block_size=16,
                       tolerance=1e-7, maximum_iterations=100, seed=42):
    """The leading eigenpairs of ``Xc^T Xc`` (``Xc``: the operator's matrix
    less its column means) by block subspace iteration.  Each iteration forms
    ``Y = Xc Q`` and ``Z = Xc^T Y``; the Ritz pairs ``(lambda_k, v_k = Q s_k)``
    come from the eigenvectors ``s_k`` of ``H = Q^T Z``, their residuals are
    ``|Z s_k - lambda_k v_k| / lambda_1``; the iteration stops when the first
    ``number_of_components`` residuals are at most ``tolerance``, else
    ``Q = qr(Z)``.  Returns a dict."""
    rows, features = operator.shape
    components = int(number_of_components)
    block = min(int(block_size), rows - 1, features)
    if block < components:
        raise ValueError(
            "{} components need a block of at least as many vectors: got "
            "min(block size {}, examples - 1 = {}, features {}).".format(
                components, block_size, rows - 1, features))
    mean, total = operator.moments()
    if not numpy.isfinite(total):
        raise ValueError("The values to decompose must be finite.")
    if not total > 0:
        raise ValueError(
            "The values have no variance: nothing to decompose.")
    rng = numpy.random.default_rng(seed)
    q, _ = numpy.linalg.qr(rng.standard_normal((features, block)))
    converged = False
    residual_history = []
    for iteration in range(1, int(maximum_iterations) + 1):
        z = operator.back_project(operator.project(q))
        h = q.T @ z
        eigenvalues, s = numpy.linalg.eigh((h + h.T) / 2)
        order = numpy.argsort(-eigenvalues, kind="stable")
        eigenvalues, s = eigenvalues[order], s[:, order]
        vectors = q @ s
        residuals = numpy.linalg.norm(
            z @ s - vectors * eigenvalues, axis=0) / eigenvalues[0]
        residual_history.append(residuals[:components].copy())
        if bool(numpy.all(residuals[:components] <= tolerance)):
            converged = True
            break
        q, _ = numpy.linalg.qr(z)
    vectors = vectors[:, :components].T
    vectors = vectors * flip_signs(vectors)[:, None]
    return {
        "mean": mean, "total": total, "components": vectors,
        "eigenvalues": eigenvalues[:components].copy(),
        "residuals": residuals[:components].copy(),
        "residual_history": residual_history,
        "iterations": iteration, "converged": converged, "block": block,
    }


class DevicePCA:
    """PCA with scikit-learn's attributes from ``subspace_iteration`` on the
    device.  ``operator`` (for the CPU suite): the class of the operator."""

    def __init__(self, n_components=2, block_size=16, tolerance=1e-7,
                 maximum_iterations=100, seed=42, device=None,
                 operator=DeviceOperator):
        self.n_components = int(n_components)
        self.block_size = int(block_size)
        self.tolerance = float(tolerance)
        self.maximum_iterations = int(maximum_iterations)
        self.seed = seed
        self.device = device
        self._operator_class = operator
        if self.n_components < 1:
            raise ValueError("At least one component expected.")
        if not self.n_components <= self.block_size <= MAXIMUM_BLOCK_SIZE:
            raise ValueError(
                "A block of {} to {} vectors expected, got {}.".format(
                    self.n_components, MAXIMUM_BLOCK_SIZE, self.block_size))
        if not self.tolerance >= 0:
            raise ValueError("A tolerance of at least zero expected.")
        if self.maximum_iterations < 1:
            raise ValueError("At least one iteration expected.")

    def _fit(self, values):
        if self._operator_class is DeviceOperator:
            operator = DeviceOperator(values, device=self.device)
        else:
            operator = self._operator_class(values)
        result = subspace_iteration(
            operator, self.n_components, self.block_size, self.tolerance,
            self.maximum_iterations, self.seed)
        rows = operator.shape[0]
        self.operator_ = operator
        self.mean_ = result["mean"]
        self.components_ = result["components"]
        eigenvalues = result["eigenvalues"]
        self.explained_variance_ = eigenvalues / (rows - 1)
        self.explained_variance_ratio_ = eigenvalues / result["total"]
        self.singular_values_ = numpy.sqrt(numpy.maximum(eigenvalues, 0))
        self.n_iterations_ = result["iterations"]
        self.residuals_ = result["residuals"]
        self.converged_ = result["converged"]
        self.total_variance_ = result["total"]
        if not self.converged_:
            print("Decomposition not converged after {} iterations "
                  "(largest residual {:.3g}, tolerance {:.3g}): these are the "
                  "last Ritz pairs.".format(
                      self.n_iterations_, float(self.residuals_.max()),
                      self.tolerance))
        return operator

    def fit(self, values):
        self._fit(values).release()
        return self

    def fit_transform(self, values):
        operator = self._fit(values)
        coordinates = operator.to_host(operator.project(self.components_.T))
        operator.release()
        return coordinates

    def transform(self, values):
        if not hasattr(self, "operator_"):
            raise RuntimeError("This DevicePCA has not been fitted.")
        operator = self.operator_
        return operator.to_host(
            operator.project(self.components_.T, values=values))


def _device_reason(values, number_of_components):
    """Why ``decompose`` cannot take the device path for these values."""
    reason = limit_reason(values.shape[0], values.shape[1],
                          number_of_components, max(16, number_of_components))
    if reason is None and not isinstance(values, torch.Tensor):
        reason = memory_limit_reason(values.shape, torch.device(
            "cuda", torch.cuda.current_device()))
    return reason


def decompose(values, other_value_sets={}, centroids={}, method=None,
              number_of_components=None, random=False):
    """The reference's ``decompose`` (``decomposition.py:44-167``): same
    arguments, same list returned.  Only PCA is built.  Up to 2000 dense
    features it is scikit-learn's ``PCA`` on the host as in the reference;
    above, or for a sparse matrix, ``DevicePCA`` (the converged exact PCA
    where the reference fits ``IncrementalPCA``)."""
    if method is None:
        method = defaults["analyses"]["decomposition_method"]
    method = method_name(method)
    if method not in DECOMPOSITION_METHOD_NAMES:
        raise ValueError("Method `{}` not found.".format(method))
    if method != "PCA":
        raise NotImplementedError(
            "Decomposition method `{}` is not part of this build "
            "(scvae/analyses/decomposition/decomposition.py:74-87): only PCA "
            "is.".format(method))
    if number_of_components is None:
        number_of_components = defaults["analyses"][
            "decomposition_dimensionality"]

    other_values_provided_as_dictionary = True
    if other_value_sets is not None and not isinstance(other_value_sets, dict):
        other_value_sets = {"unknown": other_value_sets}
        other_values_provided_as_dictionary = False

    if (values.shape[1] <= MAXIMUM_FEATURE_SIZE_FOR_NORMAL_PCA
            and not _is_sparse(values)):
        from sklearn.decomposition import PCA
        model = PCA(n_components=number_of_components)
    else:
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(
                "No GPU visible: the device decomposition has no CPU path.")
        reason = _device_reason(values, number_of_components)
        if reason is None:
            model = DevicePCA(
                n_components=number_of_components,
                block_size=max(16, number_of_components),
                seed=None if random else 42)
        else:
            print("decomposition on the device not used: {}.".format(reason))
            from sklearn.decomposition import IncrementalPCA
            model = IncrementalPCA(n_components=number_of_components,
                                   batch_size=100)
    if isinstance(values, torch.Tensor) and not isinstance(model, DevicePCA):
        values = values.cpu().numpy()
    values_decomposed = model.fit_transform(values)

    if other_value_sets:
        other_value_sets_decomposed = {}
        for other_set_name, other_values in other_value_sets.items():
            other_value_sets_decomposed[other_set_name] = (
                model.transform(other_values) if other_values is not None
                else None)
    else:
        other_value_sets_decomposed = None
    if other_value_sets_decomposed and not other_values_provided_as_dictionary:
        other_value_sets_decomposed = other_value_sets_decomposed["unknown"]

    # (decomposition.py:109-157: centroids without data sets as top levels)
    if centroids is not None:
        if "means" in centroids:
            centroids = {"unknown": centroids}
        components = numpy.asarray(model.components_, dtype=numpy.float64)
        mean = numpy.asarray(model.mean_, dtype=numpy.float64)
        centroids_decomposed = {}
        for distribution, distribution_centroids in centroids.items():
            if not distribution_centroids:
                centroids_decomposed[distribution] = None
                continue
            decomposed = {}
            for parameter, parameter_values in distribution_centroids.items():
                if parameter == "means":
                    shape = list(parameter_values.shape)
                    flat = numpy.asarray(parameter_values).reshape(
                        -1, shape[-1])
                    shape[-1] = number_of_components
                    decomposed[parameter] = (
                        (flat - mean) @ components.T).reshape(shape)
                elif parameter == "covariance_matrices":
                    shape = list(parameter_values.shape)
                    flat = numpy.asarray(parameter_values).reshape(
                        -1, shape[-1], shape[-1])
                    shape[-2:] = [number_of_components] * 2
                    decomposed[parameter] = numpy.stack([
                        components @ matrix @ components.T
                        for matrix in flat]).reshape(shape)
                else:
                    decomposed[parameter] = parameter_values
            centroids_decomposed[distribution] = decomposed
        if "unknown" in centroids_decomposed:
            centroids_decomposed = centroids_decomposed["unknown"]
    else:
        centroids_decomposed = None

    output = [values_decomposed]
    if other_value_sets != {}:
        output.append(other_value_sets_decomposed)
    if centroids != {}:
        output.append(centroids_decomposed)
    return output


def evaluation_decomposition(values, projected=None, number_of_components=2):
    """What ``ModelBase.evaluate`` attaches: the PCA of ``values`` (an fp32
    device matrix, read in place) as a dict; with ``projected`` (another
    device matrix with the same features) the coordinates are those of
    ``projected`` in the space of ``values`` (``analyses.py:1267-1280``)."""
    time_start = time()
    model = DevicePCA(n_components=number_of_components)
    coordinates = model.fit_transform(values)
    result = {}
    if projected is not None:
        result["fitted_coordinates"] = coordinates
        coordinates = model.transform(projected)
    result.update({
        "coordinates": coordinates,
        "components": model.components_,
        "mean": model.mean_,
        "explained_variance_ratio": model.explained_variance_ratio_,
        "iterations": model.n_iterations_,
        "converged": model.converged_,
        "model": model,
        "duration": time() - time_start,
    })
    return result
