"""Oracle of the feature selection: the per-gene moments of a count matrix as
Python integers and the selection rule on them, written without
``scvae_amd/data/processing.py`` (plain loops over the stored entries, no
NumPy reductions).

    num_j = N * sum_i x_ij^2 - (sum_i x_ij)^2         (an exact integer)
    population variance of gene j = num_j / N^2

``remove_zeros`` keeps sum_j != 0, ``keep_variances_above t`` keeps
num_j / N^2 > t (the quotient by Python's true division of integers, which
rounds once), ``keep_highest_variances k`` keeps the last k genes of the
ascending order by (num_j, j), in ascending gene order.
"""
import numpy
import scipy.sparse


def moments(matrix):
    """``(sum, sum of squares, number of values != 0)`` per column as lists of
    Python integers; duplicate entries of a sparse matrix are summed first."""
    matrix = scipy.sparse.coo_matrix(matrix)
    n_features = matrix.shape[1]
    cells = {}
    for i, j, v in zip(matrix.row.tolist(), matrix.col.tolist(),
                       matrix.data.tolist()):
        cells[(i, j)] = cells.get((i, j), 0) + v
    sums = [0] * n_features
    squares = [0] * n_features
    nonzeros = [0] * n_features
    for (_, j), v in cells.items():
        x = int(v)
        assert x == v and 0 <= x <= 65535, v
        sums[j] += x
        squares[j] += x * x
        nonzeros[j] += 1 if x else 0
    return sums, squares, nonzeros


def numerators(matrix):
    n_examples = matrix.shape[0]
    sums, squares, _ = moments(matrix)
    return [n_examples * q - s * s for s, q in zip(sums, squares)]


def select(matrix, method, parameter=None):
    """The selected genes in ascending order."""
    n_examples, n_features = matrix.shape
    if method == "remove_zeros":
        sums = moments(matrix)[0]
        return [j for j in range(n_features) if sums[j] != 0]
    num = numerators(matrix)
    if method == "keep_variances_above":
        threshold = 0.5 if parameter is None else float(parameter)
        return [j for j in range(n_features)
                if num[j] / (n_examples * n_examples) > threshold]
    if method == "keep_highest_variances":
        k = n_examples // 2 if parameter is None else int(parameter)
        order = sorted(range(n_features), key=lambda j: (num[j], j))
        return sorted(order[-k:])
    raise KeyError(method)


def count_matrix(n_examples, n_features, density, seed, empty_rows=(),
                 empty_columns=(), maxima=0):
    """A seeded CSR count matrix: gamma-Poisson counts at about ``density``
    stored entries, some rows and columns emptied, ``maxima`` entries set to
    65 535."""
    random_state = numpy.random.RandomState(seed)
    mask = random_state.random_sample((n_examples, n_features)) < density
    rates = random_state.gamma(0.6, 4.0, size=(n_examples, n_features))
    dense = (random_state.poisson(rates) + 1) * mask
    dense[list(empty_rows), :] = 0
    dense[:, list(empty_columns)] = 0
    stored = numpy.argwhere(dense > 0)
    if maxima and len(stored):
        for i, j in stored[random_state.choice(len(stored), maxima,
                                               replace=False)]:
            dense[i, j] = 65535
    return scipy.sparse.csr_matrix(dense.astype(numpy.float32))
