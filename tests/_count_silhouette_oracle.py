"""NumPy oracle of the count-space silhouette
(``scvae_amd/csrc/count_silhouette.hip``,
``scvae_amd/analyses/count_silhouette.py``): squared distances between count
rows from int64 arithmetic (exact), d = sqrt in fp64, then a, b and s in fp64:
a = 0 in a cluster of one row, s = 0 there and when max(a, b) = 0."""
import functools

import numpy


def squared_distances(x):
    """d2 [N, N] int64, exact: n_i + n_j - 2 g_ij with g = X X^T in int64."""
    x = numpy.asarray(x).astype(numpy.int64)
    gram = x @ x.T
    norms = numpy.diagonal(gram)
    return norms[:, None] + norms[None, :] - 2 * gram


def silhouette_from_distances(d, labels):
    """(a, b, s), fp64 [N] each, from the distances d [N, N] fp64."""
    distinct, ids = numpy.unique(numpy.asarray(labels).reshape(-1),
                                 return_inverse=True)
    ids = ids.reshape(-1)
    n, k = d.shape[0], len(distinct)
    assert len(ids) == n and k >= 2
    counts = numpy.bincount(ids, minlength=k).astype(numpy.float64)
    one_hot = numpy.zeros((n, k))
    one_hot[numpy.arange(n), ids] = 1.0
    sums = d @ one_hot
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


def silhouette(x, labels):
    d = numpy.sqrt(squared_distances(x).astype(numpy.float64))
    return silhouette_from_distances(d, labels)


def _freeze(*arrays):
    for array in arrays:
        array.setflags(write=False)
    return arrays


def pitch_of(features, extra=0):
    """A row pitch of the uint16 layout: a multiple of 8, at least the
    features rounded up to 64."""
    return (features + 63) // 64 * 64 + extra


#: name -> (N, F, K, ldx) of the planted cases
SHAPES = {
    "130x300x5": (130, 300, 5, pitch_of(300, 8)),
    "65x515x64": (65, 515, 64, pitch_of(515)),
    "257x256x2": (257, 256, 2, pitch_of(256)),
    "257x257x2": (257, 257, 2, pitch_of(257)),
    "200x32738x20": (200, 32738, 20, pitch_of(32738)),
    "1000x2000x999": (1000, 2000, 999, pitch_of(2000, 64)),
}


def planted_counts(n, features, k, seed, large=0, planted=None):
    """Poisson counts around K gene profiles (uint16 [N, F]) and the planted
    cluster of every row (drawn here unless given); ``large`` entries are
    raised into the thousands."""
    rng = numpy.random.default_rng(seed)
    profiles = rng.gamma(0.3, 2.0, size=(k, features))
    if planted is None:
        planted = rng.integers(k, size=n)
        planted[:k] = numpy.arange(k)
    depth = rng.uniform(0.5, 2.0, size=(n, 1))
    x = rng.poisson(profiles[planted] * depth).astype(numpy.int64)
    if large:
        at = (rng.integers(n, size=large), rng.integers(features, size=large))
        x[at] = rng.integers(1000, 60000, size=large)
    assert x.min() >= 0 and x.max() <= 65535
    return x.astype(numpy.uint16), planted.astype(numpy.int64)


@functools.lru_cache(maxsize=None)
def planted_case(name):
    """(x uint16 [N, F], labels int64 [N] with exactly K distinct values):
    20 % of the planted labels are reshuffled, so that s takes both signs.
    K = N - 1 gives N - 2 clusters of one row and one of two rows that are
    the same cell."""
    n, features, k, _ = SHAPES[name]
    x, labels = planted_counts(n, features, k, seed=n + 31 * k + features,
                               large=40 if features > 30000 else 0)
    rng = numpy.random.default_rng(n + k)
    moved = rng.random(n) < 0.2
    labels[moved] = rng.integers(k, size=int(moved.sum()))
    labels[:k] = numpy.arange(k)
    if k == n - 1:
        labels[k:] = k - 2
        x[k] = x[k - 2]
    assert len(numpy.unique(labels)) == k
    return _freeze(x, labels)


@functools.lru_cache(maxsize=None)
def saturated_case():
    """12 x 520 at the ends of the range.  Rows 0-3 are all 65 535, split
    over clusters 0 = {0, 2} and 1 = {1, 3}: identical rows in different
    clusters, a = b = 0 and s = 0.  Rows 4-5 all 0 (cluster 2), rows 6-7 all
    255 (cluster 3), rows 8-9 all 256 (cluster 4): a = 0 < b, s = 1.  Rows
    10-11, all 0 and all 65 535, are cluster 5: d2 = 520 x 65 535^2, the
    largest a distance gets per gene, and their twins in clusters 2 and 0 / 1
    give b = 0 < a, s = -1.  All-0 rows drive the int8 products to
    their largest magnitude (-128 x -128 in every gene), all-65 535 rows to
    127 x 127, 255 and 256 put everything in one byte."""
    fill = [65535] * 4 + [0, 0, 255, 255, 256, 256, 0, 65535]
    x = numpy.repeat(numpy.array(fill, dtype=numpy.uint16)[:, None], 520, 1)
    labels = numpy.array([0, 1, 0, 1, 2, 2, 3, 3, 4, 4, 5, 5],
                         dtype=numpy.int64)
    return _freeze(numpy.ascontiguousarray(x), labels)


@functools.lru_cache(maxsize=None)
def edge_case():
    """322 rows at F = 70 in clusters of exactly 1, 63, 64, 65 and 129 rows:
    in the grouped order the clusters end at rows 1, 64, 128, 193 and 322, on
    and around the edges of the 64-lane walk and the 128-row tiles.  Every
    fifth row is drawn from the profile of the next cluster."""
    sizes = [1, 63, 64, 65, 129]
    labels = numpy.repeat(numpy.arange(5), sizes).astype(numpy.int64)
    planted = numpy.where(numpy.arange(len(labels)) % 5 == 4,
                          (labels + 1) % 5, labels)
    x, _ = planted_counts(len(labels), 70, 5, seed=322, planted=planted)
    return _freeze(x, labels)


def all_cases():
    """name -> (x, labels, ldx)"""
    cases = {}
    for name, shape in SHAPES.items():
        x, labels = planted_case(name)
        cases[name] = (x, labels, shape[3])
    x, labels = saturated_case()
    cases["saturated"] = (x, labels, pitch_of(x.shape[1]))
    x, labels = edge_case()
    cases["edges"] = (x, labels, pitch_of(x.shape[1]))
    return cases


@functools.lru_cache(maxsize=None)
def expected_squared_distances(name):
    return _freeze(squared_distances(all_cases()[name][0]))[0]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(a, b, s) fp64 in the case's own row order."""
    d = numpy.sqrt(expected_squared_distances(name).astype(numpy.float64))
    return _freeze(*silhouette_from_distances(d, all_cases()[name][1]))
