"""fp64 NumPy restatement of the device k-means (``scvae_amd/csrc/kmeans.hip``,
``scvae_amd/analyses/kmeans.py``): distances in the direct form, the lowest
cluster index on equal distances, means as sum / count, an empty cluster keeps
its centre, scikit-learn's Lloyd stopping rule."""
import numpy


def squared_distances(x, centres, chunk=2048):
    """[N, K] of sum_l (x_il - c_kl)^2 in fp64."""
    x = numpy.asarray(x, dtype=numpy.float64)
    centres = numpy.asarray(centres, dtype=numpy.float64)
    out = numpy.empty((x.shape[0], centres.shape[0]))
    for start in range(0, x.shape[0], chunk):
        d = x[start:start + chunk, None, :] - centres[None, :, :]
        out[start:start + chunk] = (d * d).sum(axis=2)
    return out


def assign(x, centres):
    """labels (lowest index on ties: ``argmin``), their distances, inertia."""
    d2 = squared_distances(x, centres)
    labels = d2.argmin(axis=1)
    minimum = d2[numpy.arange(len(labels)), labels]
    return labels.astype(numpy.int32), minimum, float(minimum.sum())


def update(x, labels, centres):
    """new centres, counts, squared shift; empty clusters keep their centre."""
    x = numpy.asarray(x, dtype=numpy.float64)
    centres = numpy.asarray(centres, dtype=numpy.float64)
    k = centres.shape[0]
    counts = numpy.bincount(labels, minlength=k)
    sums = numpy.zeros_like(centres)
    numpy.add.at(sums, labels, x)
    new = centres.copy()
    filled = counts > 0
    new[filled] = sums[filled] / counts[filled, None]
    return new, counts, float(((new - centres) ** 2).sum())


def tolerance(x, tol):
    return tol * float(numpy.var(numpy.asarray(x, dtype=numpy.float64),
                                 axis=0).mean())


def lloyd(x, initial_centres, max_iter=300, tol=1e-4):
    """centres, labels, inertia, n_iter, labels of every iteration.  Stops when
    the labels did not change, when the shift <= tol * mean(var(x, axis=0)),
    or at max_iter; labels and inertia from a final assign."""
    limit = tolerance(x, tol)
    centres = numpy.asarray(initial_centres, dtype=numpy.float64).copy()
    previous = None
    history = []
    n_iter = 0
    for iteration in range(max_iter):
        labels, _, _ = assign(x, centres)
        centres, _, shift = update(x, labels, centres)
        history.append(labels)
        n_iter = iteration + 1
        if previous is not None and numpy.array_equal(labels, previous):
            break
        if shift <= limit:
            break
        previous = labels
    labels, _, inertia = assign(x, centres)
    return centres, labels, inertia, n_iter, history


def blobs(n, latent_size, k, seed, spread=3.0):
    """C ~ N(0, spread^2) [k, L]; rows C[label] + N(0, 1); both fp32."""
    rng = numpy.random.default_rng(seed)
    centres = (spread * rng.standard_normal((k, latent_size))).astype(
        numpy.float32)
    planted = rng.integers(k, size=n)
    x = (centres[planted] + rng.standard_normal((n, latent_size))).astype(
        numpy.float32)
    return x, planted, centres


def distinct_rows(x, k, seed):
    """k pairwise distinct rows of x as start centres."""
    rng = numpy.random.default_rng(seed)
    order = rng.permutation(x.shape[0])
    chosen, seen = [], set()
    for row in order:
        key = x[row].tobytes()
        if key not in seen:
            seen.add(key)
            chosen.append(row)
            if len(chosen) == k:
                break
    assert len(chosen) == k
    return x[numpy.array(chosen)].copy()


def adjusted_rand_index(a, b):
    a = numpy.asarray(a)
    b = numpy.asarray(b)
    _, ai = numpy.unique(a, return_inverse=True)
    _, bi = numpy.unique(b, return_inverse=True)
    table = numpy.zeros((ai.max() + 1, bi.max() + 1), dtype=numpy.int64)
    numpy.add.at(table, (ai, bi), 1)

    def pairs(v):
        return (v * (v - 1) // 2).sum()
    together = pairs(table)
    rows, cols = pairs(table.sum(axis=1)), pairs(table.sum(axis=0))
    total = len(a) * (len(a) - 1) // 2
    expected = rows * cols / total
    maximum = (rows + cols) / 2
    if maximum == expected:
        return 1.0
    return float((together - expected) / (maximum - expected))
