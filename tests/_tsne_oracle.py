"""fp64 NumPy statement of exact t-SNE as scikit-learn documents it
(``TSNE(method="exact")``, two components, Euclidean metric, one degree of
freedom): the perplexity search, the joint probabilities, the KL divergence
and its gradient with both clamps, the gradient-descent step with gains and
the two-stage loop.  Everything is dense ``N x N``: for small inputs only."""
import numpy

EPS = float(numpy.finfo(numpy.float64).eps)
SEARCH_STEPS = 100
SEARCH_TOLERANCE = 1e-5
EMPTY_ROW_SUM = 1e-8
ITERATIONS_BETWEEN_CHECKS = 50
MINIMUM_GAIN = 0.01


def squared_distances(x):
    """``sum_l (x_il - x_jl)^2`` in fp64."""
    x = numpy.asarray(x, dtype=numpy.float64)
    difference = x[:, None, :] - x[None, :, :]
    return (difference ** 2).sum(axis=2)


def row_entropy(d2_row, i, beta):
    """``(H, S, raw)`` of row ``i`` at ``beta``: the conditional
    ``p_j = exp(-beta d2_j) / S`` over ``j != i``, ``S`` their sum ``raw``,
    1e-8 where that is 0, ``H = log S + beta sum_j d2_j p_j``."""
    d2 = numpy.delete(numpy.asarray(d2_row, dtype=numpy.float64), i)
    p = numpy.exp(-d2 * beta)
    raw = float(p.sum())
    S = raw if raw > 0 else EMPTY_ROW_SUM
    return float(numpy.log(S) + beta * (d2 * p).sum() / S), S, raw


def perplexity_search(d2, perplexity):
    """The binary search of every row: ``beta`` from 1, doubled or halved
    until bracketed, then bisected, until ``|H - log(perplexity)| <= 1e-5`` or
    100 steps.  Returns ``beta``, ``S`` and ``steps`` (100: not reached)."""
    n = d2.shape[0]
    target = numpy.log(perplexity)
    betas, sums = numpy.empty(n), numpy.empty(n)
    steps = numpy.empty(n, dtype=numpy.int64)
    for i in range(n):
        beta, beta_min, beta_max = 1.0, -numpy.inf, numpy.inf
        for step in range(SEARCH_STEPS):
            H, S, _ = row_entropy(d2[i], i, beta)
            betas[i], sums[i] = beta, S
            difference = H - target
            if abs(difference) <= SEARCH_TOLERANCE:
                steps[i] = step
                break
            if difference > 0:
                beta_min = beta
                beta = beta * 2 if beta_max == numpy.inf else (
                    beta + beta_max) / 2
            else:
                beta_max = beta
                beta = beta / 2 if beta_min == -numpy.inf else (
                    beta + beta_min) / 2
        else:
            steps[i] = SEARCH_STEPS
    return betas, sums, steps


def conditionals(d2, beta, sums):
    """``p(j | i) = exp(-beta_i d2_ij) / S_i``, 0 on the diagonal."""
    p = numpy.exp(-d2 * numpy.asarray(beta, dtype=numpy.float64)[:, None])
    p = p / numpy.asarray(sums, dtype=numpy.float64)[:, None]
    numpy.fill_diagonal(p, 0.0)
    return p


def joint_probabilities(d2, beta, sums, sum_p=None):
    """``P_ij = max((p(j | i) + p(i | j)) / sumP, eps)``, 0 on the diagonal;
    ``sumP`` the sum of the symmetrised conditionals unless given."""
    p = conditionals(d2, beta, sums)
    p = p + p.T
    if sum_p is None:
        sum_p = max(float(p.sum()), EPS)
    p = numpy.maximum(p / sum_p, EPS)
    numpy.fill_diagonal(p, 0.0)
    return p


def kl_divergence_and_gradient(P, y, exaggeration=1.0):
    """``(KL, grad, Z)`` at the embedding ``y``:
    ``w = 1 / (1 + |y_i - y_j|^2)``, ``Q = max(w / Z, eps)``, ``KL = sum P log(max(P, eps) / Q)``,
    ``grad_i = 4 sum_j (P - Q)_ij w_ij (y_i - y_j)``, ``P`` times the
    exaggeration throughout."""
    y = numpy.asarray(y, dtype=numpy.float64)
    P = P * exaggeration
    difference = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (difference ** 2).sum(axis=2))
    numpy.fill_diagonal(w, 0.0)
    Z = float(w.sum())
    Q = numpy.maximum(w / Z, EPS)
    off = ~numpy.eye(len(y), dtype=bool)
    kl = float((P[off] * numpy.log(numpy.maximum(P[off], EPS) / Q[off])).sum())
    grad = 4.0 * (((P - Q) * w)[:, :, None] * difference).sum(axis=1)
    return kl, grad, Z


def update_step(y, update, gains, grad, momentum, learning_rate,
                min_gain=MINIMUM_GAIN):
    """One step of scikit-learn's ``_gradient_descent``; returns the new
    ``(y, update, gains)``."""
    increase = update * grad < 0.0
    gains = numpy.where(increase, gains + 0.2, gains * 0.8)
    gains = numpy.maximum(gains, min_gain)
    update = momentum * update - learning_rate * gains * grad
    return y + update, update, gains


def _descend(P, y, first, last, momentum, exaggeration, patience,
             learning_rate, min_grad_norm, trace):
    """scikit-learn's ``_gradient_descent``: every call starts from a zero
    update and unit gains."""
    update, gains = numpy.zeros_like(y), numpy.ones_like(y)
    best_error, best_iteration = numpy.finfo(float).max, first
    iteration = first
    for iteration in range(first, last):
        error, grad, _ = kl_divergence_and_gradient(P, y, exaggeration)
        if trace is not None:
            trace.append({"y": y, "update": update, "gains": gains,
                          "grad": grad, "momentum": momentum,
                          "exaggeration": exaggeration})
        check = (iteration + 1) % ITERATIONS_BETWEEN_CHECKS == 0
        y, update, gains = update_step(y, update, gains, grad, momentum,
                                       learning_rate)
        if check:
            if error < best_error:
                best_error, best_iteration = error, iteration
            elif iteration - best_iteration > patience:
                break
            if numpy.linalg.norm(grad) <= min_grad_norm:
                break
    return y, gains, iteration


def fit(x, y0, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto",
        max_iter=1000, exploration_iterations=250,
        n_iter_without_progress=300, min_grad_norm=1e-7, trace=None):
    """The whole fit from the rows ``x`` and the initial embedding ``y0``.
    ``trace`` (a list): gets the state and the gradient before every update.
    Returns a dict: ``embedding``, ``kl_divergence`` (of that embedding),
    ``n_iter``, ``gains``, ``P``."""
    x = numpy.asarray(x, dtype=numpy.float64)
    n = x.shape[0]
    d2 = squared_distances(x)
    beta, sums, _ = perplexity_search(d2, perplexity)
    P = joint_probabilities(d2, beta, sums)
    if learning_rate == "auto":
        learning_rate = max(n / early_exaggeration / 4.0, 50.0)
    y = numpy.array(y0, dtype=numpy.float64)
    y, gains, iteration = _descend(
        P, y, 0, exploration_iterations, 0.5, early_exaggeration,
        exploration_iterations, learning_rate, min_grad_norm, trace)
    if iteration < exploration_iterations or (
            max_iter - exploration_iterations > 0):
        y, gains, iteration = _descend(
            P, y, iteration + 1, max_iter, 0.8, 1.0,
            n_iter_without_progress, learning_rate, min_grad_norm, trace)
    return {"embedding": y, "gains": gains, "n_iter": iteration,
            "kl_divergence": kl_divergence_and_gradient(P, y)[0],
            "P": P, "learning_rate": learning_rate}
