"""k-means over latent values on the device: the clustering behind
``scvae evaluate -P k-means`` (``scvae/analyses/prediction.py:33-131``) as
exact Lloyd iterations on the kernels of ``csrc/kmeans.hip``.

The reference calls scikit-learn (``KMeans`` up to 10 000 cells,
``MiniBatchKMeans`` above); this runs full Lloyd for every size.  What differs
from scikit-learn's ``KMeans`` on purpose: distances in the direct form
``sum (x - c)^2`` in fp32, the lowest cluster index on equal distances, plain
k-means++ (one candidate per centre), and a cluster that loses all its cells
keeps its centre instead of being relocated.  Every kernel sums in one fixed
order, so a seeded fit gives the same bits on every run.
"""
import ctypes

import numpy
import torch

from scvae_amd import _lib

MAXIMUM_CLUSTERS = 256
MAXIMUM_LATENT_SIZE = 256
MAXIMUM_CENTRE_VALUES = 8192
_VARIANCE_CHUNK = 1 << 16


def limit_reason(number_of_rows, latent_size, number_of_clusters):
    """Why these sizes are outside what the kernels take (``None``: they are
    inside)."""
    n, l, k = int(number_of_rows), int(latent_size), int(number_of_clusters)
    if not 1 <= k <= MAXIMUM_CLUSTERS:
        return "{} clusters (1 to {} supported)".format(k, MAXIMUM_CLUSTERS)
    if not 1 <= l <= MAXIMUM_LATENT_SIZE:
        return "latent size {} (1 to {} supported)".format(
            l, MAXIMUM_LATENT_SIZE)
    if k * l > MAXIMUM_CENTRE_VALUES:
        return "{} clusters x {} latent values (at most {} supported)".format(
            k, l, MAXIMUM_CENTRE_VALUES)
    if k > n:
        return "{} clusters for {} cells".format(k, n)
    if n >= 2 ** 31:
        return "{} cells (fewer than 2^31 supported)".format(n)
    return None


def _as_matrix(values):
    if hasattr(values, "toarray"):
        values = values.toarray()
    values = numpy.ascontiguousarray(values, dtype=numpy.float32)
    if values.ndim != 2:
        raise ValueError("Expected a [cells, latent] matrix, got shape {}."
                         .format(values.shape))
    if not numpy.isfinite(values).all():
        raise ValueError("The values to cluster must be finite.")
    return values if values.flags.writeable else values.copy()


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr()) if tensor is not None else None


class DeviceKMeans:
    """Lloyd's k-means on one GPU with scikit-learn's stopping rule: stop when
    no label changed, when the squared centre shift is at most
    ``tol * mean(var(X, axis=0))``, or after ``max_iter`` iterations."""

    def __init__(self, n_clusters, n_init=10, max_iter=300, tol=1e-4,
                 seed=None, device=None):
        self.n_clusters = int(n_clusters)
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.seed = seed
        self.device = device
        self.cluster_centers_ = None
        self.labels_ = None
        self.inertia_ = None
        self.n_iter_ = None
        #: rows of the training set that seeded each k-means++ run
        self.seed_rows_ = []

    # ---- plumbing -------------------------------------------------------
    def _open(self):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(
                "No GPU visible: the device k-means has no CPU path.")
        self._lib = _lib.load()
        self._device = torch.device(
            self.device if self.device is not None else "cuda:0")

    def _stream(self):
        return ctypes.c_void_p(
            torch.cuda.current_stream(self._device).cuda_stream)

    def _upload(self, values):
        matrix = _as_matrix(values)
        reason = limit_reason(matrix.shape[0], matrix.shape[1],
                              self.n_clusters)
        if reason is not None:
            raise ValueError("Device k-means: " + reason + ".")
        return torch.from_numpy(matrix).to(self._device)

    def _workspace(self, rows, latent_size):
        nbytes = self._lib.scvae_kmeans_workspace_bytes(
            rows, latent_size, self.n_clusters)
        if nbytes < 0:
            _lib.check(-1, "scvae_kmeans_workspace_bytes")
        return torch.empty(nbytes, dtype=torch.uint8, device=self._device)

    def _assign(self, x, centres, labels, inertia, workspace, min_d2=None):
        _lib.check(self._lib.scvae_kmeans_assign(
            _ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(centres),
            centres.shape[0], _ptr(labels), _ptr(min_d2), _ptr(inertia),
            _ptr(workspace), workspace.numel(), self._stream()),
            "scvae_kmeans_assign")

    def _update(self, x, labels, centres, new_centres, counts, shift,
                workspace):
        _lib.check(self._lib.scvae_kmeans_update(
            _ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(labels),
            _ptr(centres), centres.shape[0], _ptr(new_centres), _ptr(counts),
            _ptr(shift), _ptr(workspace), workspace.numel(), self._stream()),
            "scvae_kmeans_update")

    def _min_d2_update(self, x, row, min_d2):
        _lib.check(self._lib.scvae_kmeans_min_d2_update(
            _ptr(x), x.stride(0), x.shape[0], x.shape[1], int(row),
            _ptr(min_d2), self._stream()), "scvae_kmeans_min_d2_update")

    @staticmethod
    def _mean_variance(x):
        """mean(var(X, axis=0)) in fp64, in row chunks (two passes)."""
        n = x.shape[0]
        total = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
        for start in range(0, n, _VARIANCE_CHUNK):
            total += x[start:start + _VARIANCE_CHUNK].double().sum(dim=0)
        mean = total / n
        squares = torch.zeros_like(total)
        for start in range(0, n, _VARIANCE_CHUNK):
            d = x[start:start + _VARIANCE_CHUNK].double() - mean
            squares += (d * d).sum(dim=0)
        return float((squares / n).mean())

    # ---- seeding and Lloyd ----------------------------------------------
    def _kmeanspp_rows(self, x, rng):
        """Plain k-means++: a uniform first row, every further row with
        probability proportional to its squared distance to the nearest
        chosen one (uniform when all of them are 0)."""
        n = x.shape[0]
        rows = [int(rng.integers(n))]
        min_d2 = torch.full((n,), float("inf"), dtype=torch.float32,
                            device=x.device)
        self._min_d2_update(x, rows[0], min_d2)
        for _ in range(1, self.n_clusters):
            u = float(rng.random())
            cumulative = torch.cumsum(min_d2.double(), dim=0)
            total = cumulative[-1]
            target = (total * u).reshape(1)
            row = torch.searchsorted(cumulative, target, right=True)
            row, total = torch.stack(
                [row[0].double().clamp(max=n - 1), total]).tolist()
            rows.append(int(row) if total > 0 else min(int(u * n), n - 1))
            self._min_d2_update(x, rows[-1], min_d2)
        return rows

    def _lloyd(self, x, initial_centres, tolerance, workspace):
        k = self.n_clusters
        device = x.device
        centres = initial_centres.clone()
        new_centres = torch.empty_like(centres)
        labels = torch.empty(x.shape[0], dtype=torch.int32, device=device)
        previous = torch.full_like(labels, -1)
        counts = torch.empty(k, dtype=torch.int32, device=device)
        scalars = torch.zeros(2, dtype=torch.float64, device=device)
        inertia, shift = scalars[0:1], scalars[1:2]
        iterations = 0
        for iteration in range(self.max_iter):
            self._assign(x, centres, labels, inertia, workspace)
            self._update(x, labels, centres, new_centres, counts, shift,
                         workspace)
            centres, new_centres = new_centres, centres
            iterations = iteration + 1
            changed, moved = torch.stack(
                [(labels != previous).any().double(), shift[0]]).tolist()
            if not changed or moved <= tolerance:
                break
            labels, previous = previous, labels
        self._assign(x, centres, labels, inertia, workspace)
        return centres, labels, float(inertia.item()), iterations

    # ---- public -----------------------------------------------------------
    def fit(self, values, initial_centres=None):
        self._open()
        x = self._upload(values)
        workspace = self._workspace(x.shape[0], x.shape[1])
        tolerance = self.tol * self._mean_variance(x)
        self.seed_rows_ = []
        if initial_centres is not None:
            start = numpy.ascontiguousarray(initial_centres,
                                            dtype=numpy.float32)
            if start.shape != (self.n_clusters, x.shape[1]):
                raise ValueError(
                    "Initial centres of shape {}, expected {}.".format(
                        start.shape, (self.n_clusters, x.shape[1])))
            if not numpy.isfinite(start).all():
                raise ValueError("The initial centres must be finite.")
            best = self._lloyd(x, torch.from_numpy(start).to(self._device),
                               tolerance, workspace)
        else:
            rng = numpy.random.default_rng(self.seed)
            best = None
            for _ in range(max(self.n_init, 1)):
                rows = self._kmeanspp_rows(x, rng)
                self.seed_rows_.append(rows)
                index = torch.tensor(rows, dtype=torch.int64,
                                     device=self._device)
                run = self._lloyd(x, x[index].contiguous(), tolerance,
                                  workspace)
                if best is None or run[2] < best[2]:
                    best = run
        centres, labels, inertia, iterations = best
        self.cluster_centers_ = centres.cpu().numpy()
        self.labels_ = labels.cpu().numpy()
        self.inertia_ = inertia
        self.n_iter_ = iterations
        return self

    def predict(self, values):
        if self.cluster_centers_ is None:
            raise ValueError("predict() before fit().")
        self._open()
        matrix = _as_matrix(values)
        rows = matrix.shape[0]
        if rows == 0:
            return numpy.zeros(0, dtype=numpy.int32)
        if rows < self.n_clusters:   # the kernels ask for K <= N
            matrix = numpy.concatenate(
                [matrix, numpy.repeat(matrix[:1], self.n_clusters - rows, 0)])
        x = self._upload(matrix)
        centres = torch.from_numpy(self.cluster_centers_).to(self._device)
        if centres.shape[1] != x.shape[1]:
            raise ValueError("Fitted on {} latent values, asked about {}."
                             .format(centres.shape[1], x.shape[1]))
        labels = torch.empty(x.shape[0], dtype=torch.int32,
                             device=self._device)
        inertia = torch.zeros(1, dtype=torch.float64, device=self._device)
        self._assign(x, centres, labels, inertia,
                     self._workspace(x.shape[0], x.shape[1]))
        return labels[:rows].cpu().numpy()
