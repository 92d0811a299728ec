"""fp64 direct-form oracle for ``csrc/distances.hip`` and the error bounds
of the kernel's expanded form against it.

The oracle never subtracts large numbers: the Euclidean distance is the root
of ``sum_k (x_ik - x_jk)^2`` (the differences of fp32 values are formed in
fp64, where they are exact unless the two magnitudes are more than 2^29
apart), and the cosine distance is ``0.5 sum_k (a_ik - a_jk)^2`` over the rows
``a_i = x_i / |x_i|`` (equal to ``1 - cos`` for unit rows).  The Euclidean
oracle carries a relative error of about ``(F + 4) 2^-53`` of itself, charged
to its bound as ``gamma(F + 4) d``.  The cosine oracle carries that and the
error of the two norms, which scales ``a_i`` and ``a_j`` by ``1 + e``,
``|e| <= gamma(F + 4)``, and so moves ``d`` by at most
``|a_i - a_j| (|e_i| + |e_j|) = 2 sqrt(2 d) gamma(F + 4)``; both are charged
to its bound.
"""
import numpy

U = 2.0 ** -53          # unit roundoff of fp64
U32 = 2.0 ** -24        # unit roundoff of fp32


def gamma(n, u=U):
    return n * u / (1 - n * u)


def _blocks(n, features):
    step = max(1, min(n, (1 << 24) // max(1, n * features)))
    return range(0, n, step), step


def squared_differences(a):
    """``sum_k (a_ik - a_jk)^2`` in fp64, directly."""
    a = numpy.asarray(a, dtype=numpy.float64)
    n, features = a.shape
    out = numpy.empty((n, n))
    starts, step = _blocks(n, features)
    for first in starts:
        difference = a[first:first + step, None, :] - a[None, :, :]
        out[first:first + step] = numpy.einsum(
            "ijk,ijk->ij", difference, difference)
    return out


def euclidean_oracle(x):
    return numpy.sqrt(squared_differences(x))


def cosine_oracle(x):
    """A row of zero norm has similarity 0 to every other row (scikit-learn's
    convention: ``normalize`` leaves such a row as it is) and distance 0 to
    itself."""
    x = numpy.asarray(x, dtype=numpy.float64)
    norms = numpy.sqrt(numpy.einsum("ik,ik->i", x, x))
    zero = norms == 0
    unit = x / numpy.where(zero, 1.0, norms)[:, None]
    d = 0.5 * squared_differences(unit)
    d[zero, :] = 1.0
    d[:, zero] = 1.0
    numpy.fill_diagonal(d, 0.0)
    return d


def _gram_terms(x):
    """``g_ii`` and ``sum_k |x_ik x_jk|`` in fp64 (only their size matters
    to the bounds)."""
    x = numpy.asarray(x, dtype=numpy.float64)
    absolute = numpy.abs(x)
    return numpy.einsum("ik,ik->i", x, x), absolute @ absolute.T


def _rounded(error, value):
    """The error after the kernel's last steps: one fp64 operation on the
    result (two roundings allowed), the one rounding to fp32 and the fp32
    denormal spacing."""
    return (error * (1 + 2 * U32) + numpy.abs(value) * (U32 + 2 * U)
            + 2.0 ** -149)


def euclidean_bound(x, oracle, u=U):
    """|kernel - oracle| allowed per element.  The computed
    ``s = g_ii + g_jj - 2 g_ij`` is within
    ``E = gamma(F + 3) (g_ii + g_jj + 2 sum_k |x_ik x_jk|)`` of the true
    squared distance ``D`` (F additions per Gram entry over exact products,
    then the two of the combination; the zero products of the K padding add
    nothing).  ``max(0, .)`` moves ``s`` towards ``D >= 0``.  Through the
    root: ``|sqrt(s) - sqrt(D)| = |s - D| / (sqrt(s) + sqrt(D)) <= E /
    sqrt(D)``, and ``<= sqrt(E)`` always.  The oracle's own error,
    ``gamma(F + 4) d``, is added."""
    features = numpy.asarray(x).shape[1]
    g, s = _gram_terms(x)
    error_squared = gamma(features + 3, u) * (g[:, None] + g[None, :] + 2 * s)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        through_root = numpy.where(
            oracle > 0, error_squared / oracle, numpy.inf)
    error = numpy.minimum(numpy.sqrt(error_squared), through_root)
    return _rounded(error + gamma(features + 4) * oracle, oracle)


def cosine_bound(x, oracle, u=U):
    """|kernel - oracle| allowed per element.  ``g_ij`` is within
    ``gamma(F) sum_k |x_ik x_jk|`` of its value and ``g_ii``, a sum of
    squares, within ``gamma(F) g_ii``; the product, its root and the quotient
    add four roundings, so the similarity ``c = g_ij / sqrt(g_ii g_jj)`` is
    within ``gamma(F + 2) (sum_k |x_ik x_jk| / sqrt(g_ii g_jj) + |c|) + 4 u``
    (both terms are at most 1); the subtraction from 1 rounds once more and
    the clip to [0, 2] moves the result towards the true value.  The oracle's
    own error, ``gamma(F + 4) (d + 2 sqrt(2 d))``, is added."""
    features = numpy.asarray(x).shape[1]
    g, s = _gram_terms(x)
    den = numpy.sqrt(g[:, None] * g[None, :])
    with numpy.errstate(divide="ignore", invalid="ignore"):
        ratio = numpy.where(den > 0, s / den, 0.0)
    error = gamma(features + 2, u) * (ratio + numpy.abs(1 - oracle)) + 4 * u
    return _rounded(error + gamma(features + 4) * (
        oracle + 2 * numpy.sqrt(2 * oracle)), oracle)
