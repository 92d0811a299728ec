"""The two-dimensional map of the latent space: exact t-SNE of the latent
values on the device (``scvae/analyses/analyses.py:1405-1416``,
``subanalyses.py:595-673``, ``decomposition/decomposition.py:78-91``).

The reference fits scikit-learn's Barnes-Hut approximation on the host.  Here
the objective and the optimiser are scikit-learn's ``TSNE(method="exact")``
-- two components, Euclidean metric, one degree of freedom -- over every pair
of cells, with the kernels of ``csrc/tsne.hip``.  The joint probabilities are
never stored: every pass over the pairs forms them again from the latent
rows, the precision ``beta_i`` and the normaliser ``S_i`` of each row.

What differs from scikit-learn on purpose: the initialisation is the exact
two-component PCA of the values (no random numbers; scikit-learn's
``init="pca"`` uses a randomised solver), the embedding is held in fp32 on
the device, and ``kl_divergence_`` is the divergence of the embedding that is
returned (scikit-learn reports the one before the last update).  The kernels
sum in one fixed order, so a fit gives the same bits on every run.
"""
import ctypes
from time import time

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.decomposition import (
    _is_sparse, decompose, flip_signs, method_name)
from scvae_amd.analyses.kmeans import _ptr
from scvae_amd.utilities import capitalise_string, format_duration

# scvae/analyses/subanalyses.py:45-47
MAXIMUM_NUMBER_OF_FEATURES_FOR_TSNE = 100
MAXIMUM_NUMBER_OF_EXAMPLES_FOR_TSNE = 200000
MAXIMUM_NUMBER_OF_PCA_COMPONENTS_BEFORE_TSNE = 50
MINIMUM_NUMBER_OF_EXAMPLES = 4

#: scikit-learn's ``_gradient_descent``: iterations between two checks of the
#: KL divergence and the gradient norm, the floor of the gains
ITERATIONS_BETWEEN_CHECKS = 50
MINIMUM_GAIN = 0.01
#: standard deviation of the first coordinate of the initial embedding
INITIAL_SCALE = 1e-4


def limit_reason(number_of_rows, number_of_features, perplexity=30.0,
                 number_of_components=2):
    """Why these sizes are outside what ``DeviceTSNE`` takes (``None``: they
    are inside)."""
    n, f = int(number_of_rows), int(number_of_features)
    if int(number_of_components) != 2:
        return "{} components (2 supported)".format(number_of_components)
    if not MINIMUM_NUMBER_OF_EXAMPLES <= n <= (
            MAXIMUM_NUMBER_OF_EXAMPLES_FOR_TSNE):
        return "{} examples ({} to {} supported)".format(
            n, MINIMUM_NUMBER_OF_EXAMPLES,
            MAXIMUM_NUMBER_OF_EXAMPLES_FOR_TSNE)
    if not 1 <= f <= MAXIMUM_NUMBER_OF_FEATURES_FOR_TSNE:
        return "{} features (1 to {} supported)".format(
            f, MAXIMUM_NUMBER_OF_FEATURES_FOR_TSNE)
    if not 0 < float(perplexity) < n:
        return "a perplexity of {:g} for {} examples (it must be below " \
            "their number)".format(float(perplexity), n)
    return None


def centre(values):
    """``values`` less its column means, subtracted in fp64 and rounded to
    fp32 once: the rows that go to the device.  Distances do not change."""
    if _is_sparse(values):
        values = values.toarray()
    values = numpy.asarray(values, dtype=numpy.float64)
    if values.ndim != 2:
        raise ValueError("t-SNE: a matrix expected, got shape {}.".format(
            values.shape))
    return numpy.ascontiguousarray(
        values - values.mean(axis=0), dtype=numpy.float32)


def initial_embedding(values):
    """scikit-learn's ``init="pca"`` without random numbers: the exact
    two-component PCA of ``values`` in fp64 from the ``L x L`` covariance,
    signs as ``flip_signs`` sets them, scaled so that the first coordinate
    has the standard deviation 1e-4.  ``[N, 2]`` fp64.  (A single feature
    leaves the second coordinate zero.)"""
    values = numpy.asarray(values, dtype=numpy.float64)
    centred = values - values.mean(axis=0)
    _, vectors = numpy.linalg.eigh(centred.T @ centred)
    components = vectors[:, ::-1][:, :2].T
    components = components * flip_signs(components)[:, None]
    coordinates = numpy.zeros((values.shape[0], 2))
    coordinates[:, :components.shape[0]] = centred @ components.T
    deviation = coordinates[:, 0].std()
    if not deviation > 0 or not numpy.isfinite(deviation):
        raise ValueError(
            "The values have no finite variance: nothing to embed.")
    return coordinates / deviation * INITIAL_SCALE


class TSNEPasses:
    """An fp32 matrix on the device and the passes of ``csrc/tsne.hip`` over
    it.  ``values``: an fp32 device tensor (read where it lies, a row pitch
    is honoured) or a NumPy array of fp32 rows."""

    def __init__(self, values, device=None):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(
                "No GPU visible: the device t-SNE has no CPU path.")
        self.lib = _lib.load()
        if isinstance(values, torch.Tensor):
            if values.dtype != torch.float32 or values.dim() != 2:
                raise ValueError(
                    "t-SNE: a float32 matrix expected, got {} of shape "
                    "{}.".format(values.dtype, tuple(values.shape)))
            if device is None and values.is_cuda:
                device = values.device
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(values, torch.Tensor):
            values = values.to(self.device)
            if values.shape[1] > 1 and values.stride(1) != 1:
                values = values.contiguous()
        else:
            values = torch.from_numpy(numpy.array(
                values, dtype=numpy.float32, order="C")).to(self.device)
        self.values = values
        self.rows, self.features = (int(s) for s in values.shape)
        self.pitch = (values.stride(0) if self.rows > 1 else self.features)
        size = self.lib.scvae_tsne_workspace_bytes(self.rows, self.features)
        if size < 0:
            _lib.check(-1, "scvae_tsne_workspace_bytes")
        self.workspace = torch.empty(size, dtype=torch.uint8,
                                     device=self.device)
        self.beta = self.row_sum = self.steps = self.sum_p = None

    def _stream(self):
        return ctypes.c_void_p(
            torch.cuda.current_stream(self.device).cuda_stream)

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def search(self, perplexity):
        """The perplexity search: sets ``beta``, ``row_sum``, ``steps``
        (device tensors) and ``sum_p``, the sum of the symmetrised
        conditionals, joined in fp64 on the host."""
        self.beta, self.row_sum = self._new(self.rows), self._new(self.rows)
        self.steps = self._new(self.rows, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_tsne_perplexity(
                _ptr(self.values), self.pitch, self.rows, self.features,
                float(perplexity), _ptr(self.beta), _ptr(self.row_sum),
                _ptr(self.steps), _ptr(self.workspace),
                self.workspace.numel(), self._stream()),
                "scvae_tsne_perplexity")
        ratios = self.workspace[:8 * self.rows].view(torch.float64)
        self.sum_p = 2.0 * float(numpy.sum(ratios.cpu().numpy()))
        return self

    def gradient(self, y, exaggeration, grad, kl=None, grad_norm=None):
        """One pass over all pairs at ``y``: fills ``grad`` and, where given,
        the one-element fp64 device tensors ``kl`` and ``grad_norm``."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_tsne_gradient(
                _ptr(self.values), self.pitch, self.rows, self.features,
                _ptr(self.beta), _ptr(self.row_sum), self.sum_p, _ptr(y),
                float(exaggeration), _ptr(grad), _ptr(kl), _ptr(grad_norm),
                _ptr(self.workspace), self.workspace.numel(),
                self._stream()), "scvae_tsne_gradient")

    def normaliser(self):
        """``Z`` of the last pass."""
        return float(self.workspace[:8].view(torch.float64).item())

    def update(self, y, update, gains, grad, momentum, learning_rate,
               min_gain=MINIMUM_GAIN):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_tsne_update(
                _ptr(y), _ptr(update), _ptr(gains), _ptr(grad), self.rows,
                float(momentum), float(learning_rate), float(min_gain),
                self._stream()), "scvae_tsne_update")


class DeviceTSNE:
    """Exact t-SNE with scikit-learn's schedule and attributes
    (``embedding_``, ``kl_divergence_``, ``n_iter_``, ``learning_rate_``) on
    one GPU."""

    def __init__(self, perplexity=30.0, early_exaggeration=12.0,
                 learning_rate="auto", max_iter=1000,
                 exploration_iterations=250, n_iter_without_progress=300,
                 min_grad_norm=1e-7, device=None):
        self.perplexity = float(perplexity)
        self.early_exaggeration = float(early_exaggeration)
        self.learning_rate = learning_rate
        self.max_iter = int(max_iter)
        self.exploration_iterations = int(exploration_iterations)
        self.n_iter_without_progress = int(n_iter_without_progress)
        self.min_grad_norm = float(min_grad_norm)
        self.device = device
        if not self.perplexity > 0:
            raise ValueError("A positive perplexity expected.")
        if not self.early_exaggeration >= 1:
            raise ValueError("An early exaggeration of at least 1 expected.")
        if learning_rate != "auto" and not float(learning_rate) > 0:
            raise ValueError(
                "A positive learning rate or \"auto\" expected.")
        if self.exploration_iterations < 0 or (
                self.max_iter < self.exploration_iterations):
            raise ValueError(
                "At least as many iterations as exploration iterations "
                "expected.")

    def _descend(self, passes, state, first, last, momentum, exaggeration,
                 patience):
        """scikit-learn's ``_gradient_descent`` from iteration ``first`` to
        ``last - 1``, from a zero update and unit gains as every call of it;
        the host waits for the device only at the checks.  Returns the last
        iteration."""
        y, update, gains, grad, kl, grad_norm = state
        if first < last:
            update.zero_()
            gains.fill_(1.0)
        best_error, best_iteration = numpy.finfo(float).max, first
        iteration = first
        for iteration in range(first, last):
            check = (iteration + 1) % ITERATIONS_BETWEEN_CHECKS == 0
            passes.gradient(y, exaggeration, grad, kl if check else None,
                            grad_norm if check else None)
            passes.update(y, update, gains, grad, momentum,
                          self.learning_rate_)
            if check:
                error = float(kl.item())
                if error < best_error:
                    best_error, best_iteration = error, iteration
                elif iteration - best_iteration > patience:
                    break
                if float(grad_norm.item()) <= self.min_grad_norm:
                    break
        return iteration

    def fit_transform(self, values):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(
                "No GPU visible: the device t-SNE has no CPU path.")
        reason = limit_reason(values.shape[0], values.shape[1],
                              self.perplexity)
        if reason:
            raise ValueError("t-SNE on the device: {}.".format(reason))
        if isinstance(values, torch.Tensor):
            host = values.detach().double().cpu().numpy()
        else:
            values = host = centre(values)
        y0 = initial_embedding(host)
        passes = TSNEPasses(values, device=self.device)
        rows = passes.rows
        if self.learning_rate == "auto":
            self.learning_rate_ = max(
                rows / self.early_exaggeration / 4.0, 50.0)
        else:
            self.learning_rate_ = float(self.learning_rate)
        passes.search(self.perplexity)
        y = torch.from_numpy(y0.astype(numpy.float32)).to(passes.device)
        state = (y, torch.zeros_like(y), torch.ones_like(y),
                 torch.empty_like(y),
                 passes._new(1, dtype=torch.float64),
                 passes._new(1, dtype=torch.float64))
        exploration = self.exploration_iterations
        iteration = self._descend(
            passes, state, 0, exploration, 0.5, self.early_exaggeration,
            exploration)
        if iteration < exploration or self.max_iter - exploration > 0:
            iteration = self._descend(
                passes, state, iteration + 1, self.max_iter, 0.8, 1.0,
                self.n_iter_without_progress)
        passes.gradient(y, 1.0, state[3], state[4], None)
        self.kl_divergence_ = float(state[4].item())
        self.n_iter_ = iteration
        self.embedding_ = y.double().cpu().numpy()
        self.update_ = state[1].cpu().numpy()
        self.gains_ = state[2].cpu().numpy()
        self.beta_ = passes.beta.cpu().numpy()
        self.row_sum_ = passes.row_sum.cpu().numpy()
        self.sum_p_ = passes.sum_p
        self.search_steps_ = passes.steps.cpu().numpy()
        return self.embedding_


def decompose_latent(values, method, title="latent space"):
    """One method of ``analyse_decompositions`` for a latent set, with the
    lines it prints (``subanalyses.py:595-673``): a dict with the two
    ``coordinates`` of every example, the fitted ``model`` (``None`` for
    PCA) and the ``duration``, or ``None`` where the reference skips."""
    method = method_name(method)
    if _is_sparse(values):
        values = values.toarray()
    if method != "t-SNE":
        print("Decomposing {} using {}.".format(title, method))
        time_start = time()
        fit = {"coordinates": decompose(values, method=method)[0],
               "model": None}
        return _decomposed(fit, title, time_start)
    if values.shape[0] > MAXIMUM_NUMBER_OF_EXAMPLES_FOR_TSNE:
        print("The number of examples for {}".format(title),
              "is too large to decompose it",
              "using {}. Skipping.".format(method))
        print()
        return None
    if values.shape[1] > MAXIMUM_NUMBER_OF_FEATURES_FOR_TSNE:
        number_of_components = min(
            MAXIMUM_NUMBER_OF_PCA_COMPONENTS_BEFORE_TSNE,
            values.shape[0] - 1)
        print("The number of features for {}".format(title),
              "is too large to decompose it",
              "using {} in due time.".format(method))
        print("Decomposing {} to {} components using PCA beforehand.".format(
            title, number_of_components))
        time_start = time()
        values = decompose(values, method="pca",
                           number_of_components=number_of_components)[0]
        print("{} pre-decomposed ({}).".format(
            capitalise_string(title), format_duration(time() - time_start)))
    print("Decomposing {} using {}.".format(title, method))
    time_start = time()
    reason = limit_reason(values.shape[0], values.shape[1])
    if reason is None:
        model = DeviceTSNE()
    else:
        print("t-SNE on the device not used: {}.".format(reason))
        from sklearn.manifold import TSNE
        model = TSNE(n_components=2, random_state=42)
        if isinstance(values, torch.Tensor):
            values = values.cpu().numpy()
    fit = {"coordinates": model.fit_transform(values), "model": model}
    return _decomposed(fit, title, time_start)


def _decomposed(fit, title, time_start):
    fit["duration"] = time() - time_start
    print("{} decomposed ({}).".format(
        capitalise_string(title), format_duration(fit["duration"])))
    return fit
