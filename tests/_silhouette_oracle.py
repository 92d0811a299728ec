"""fp64 NumPy restatement of the device silhouette
(``scvae_amd/csrc/silhouette.hip``, ``scvae_amd/analyses/silhouette.py``):
scikit-learn's ``silhouette_samples`` with the Euclidean metric, distances in
the direct form, s = 0 in a cluster of one row and when max(a, b) = 0."""
import functools

import numpy

import _kmeans_oracle as ko


def silhouette(x, labels):
    """(a, b, s), fp64 [N] each.  a = 0 in a cluster of one row."""
    x = numpy.asarray(x, dtype=numpy.float64)
    chunk = max(1, (1 << 22) // x.size)     # 32 MB of differences at a time
    distinct, ids = numpy.unique(numpy.asarray(labels).reshape(-1),
                                 return_inverse=True)
    ids = ids.reshape(-1)
    n, k = x.shape[0], len(distinct)
    assert len(ids) == n and k >= 2
    counts = numpy.bincount(ids, minlength=k).astype(numpy.float64)
    one_hot = numpy.zeros((n, k))
    one_hot[numpy.arange(n), ids] = 1.0
    sums = numpy.empty((n, k))
    for start in range(0, n, chunk):
        d = x[start:start + chunk, None, :] - x[None, :, :]
        sums[start:start + chunk] = numpy.sqrt((d * d).sum(axis=2)) @ one_hot
    rows = numpy.arange(n)
    own = counts[ids]
    a = numpy.where(own > 1, sums[rows, ids] / numpy.maximum(own - 1, 1), 0.0)
    means = sums / counts[None, :]
    means[rows, ids] = numpy.inf
    b = means.min(axis=1)
    largest = numpy.maximum(a, b)
    s = numpy.where((own > 1) & (largest > 0),
                    (b - a) / numpy.where(largest > 0, largest, 1.0), 0.0)
    return a, b, s


#: (N, L, K, ldx) of the blob cases
SHAPES = [
    (1000, 25, 20, 25), (2051, 100, 20, 100), (777, 2, 5, 2),
    (500, 25, 20, 40), (130, 256, 3, 256), (65, 7, 64, 7), (3, 1, 2, 1)]


def _freeze(*arrays):
    for array in arrays:
        array.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def blob_case(shape):
    """(x fp32 [N, L], labels int64 [N] with exactly K distinct values): blobs
    with 20 % of the planted labels reshuffled, so that s takes both signs.
    The first K rows carry the labels 0 .. K - 1 (every cluster has a row);
    K = N - 1 gives N - 2 clusters of one row, and the two rows of the last
    cluster but one are the same point."""
    n, latent_size, k, _ = shape
    x, planted, _ = ko.blobs(n, latent_size, k, seed=n + 31 * k)
    rng = numpy.random.default_rng(n + k)
    labels = planted.astype(numpy.int64)
    moved = rng.random(n) < 0.2
    labels[moved] = rng.integers(k, size=int(moved.sum()))
    labels[:k] = numpy.arange(k)
    if k == n - 1:
        labels[k:] = k - 2
        x[k] = x[k - 2]
    assert len(numpy.unique(labels)) == k
    return _freeze(x, labels)


@functools.lru_cache(maxsize=None)
def edge_case():
    """322 rows at L = 10 in clusters of exactly 1, 63, 64, 65 and 129 rows:
    in the grouped order the clusters end at rows 1, 64, 128, 193 and 322, on
    and around the edges of the 64-column tiles."""
    sizes = [1, 63, 64, 65, 129]
    x, _, _ = ko.blobs(sum(sizes), 10, 5, seed=322)
    labels = numpy.repeat(numpy.arange(5), sizes).astype(numpy.int64)
    return _freeze(x, labels)


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """Rows 0-69: one point 70 times (cluster 0); rows 70-99: another point
    30 times (cluster 1): a = 0 < b, s = 1 for all of them.  Rows 100-103: a
    third point four times, split over clusters 2 = {100, 102} and
    3 = {101, 103}: identical rows in two clusters, a = b = 0 and s = 0."""
    rng = numpy.random.default_rng(5)
    points = (4.0 * rng.standard_normal((3, 6))).astype(numpy.float32)
    x = numpy.concatenate([numpy.repeat(points[0:1], 70, 0),
                           numpy.repeat(points[1:2], 30, 0),
                           numpy.repeat(points[2:3], 4, 0)])
    labels = numpy.array([0] * 70 + [1] * 30 + [2, 3, 2, 3], dtype=numpy.int64)
    return _freeze(x, labels)


def all_cases():
    """name -> (x, labels, ldx)"""
    cases = {}
    for shape in SHAPES:
        x, labels = blob_case(shape)
        cases["x".join(str(v) for v in shape)] = (x, labels, shape[3])
    x, labels = edge_case()
    cases["edges"] = (x, labels, x.shape[1])
    x, labels = duplicate_case()
    cases["duplicates"] = (x, labels, x.shape[1])
    return cases


@functools.lru_cache(maxsize=None)
def expected(name):
    x, labels, _ = all_cases()[name]
    return _freeze(*silhouette(x, labels))
