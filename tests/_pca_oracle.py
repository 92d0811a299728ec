"""The oracle of the PCA tests: the fp64 ``numpy.linalg.svd`` of the centred
matrix of the same fp32 values, with the sign rule of the decomposition (for
each component the loading of largest magnitude positive, the lowest index on
ties), the count-like test sets, and the bounds the tests hold the device to.
"""
import functools

import numpy

#: unit roundoff of fp64
U = 2.0 ** -53

#: (n, f, seed) of the five count-like sets
SETS = [(300, 2101, 1), (130, 2050, 2), (517, 2333, 3), (64, 4099, 4),
        (1000, 3000, 5)]
#: convergence must come within this many iterations: 4 x the 9 seen in an
#: fp64 model of the algorithm -- a cap, not a measurement
MAXIMUM_ITERATIONS = 40


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a sum
    of k rounded operations, whatever their order."""
    return k * U / (1 - k * U)


@functools.lru_cache(maxsize=None)
def count_like(n, f, seed):
    """About 73 % zeros, largest count 83-202, four groups of cells."""
    rng = numpy.random.default_rng(seed)
    g = rng.integers(0, 4, n)
    base = rng.gamma(0.3, 2.0, f)
    prog = numpy.exp(rng.normal(0, 1, (4, f)) * (rng.random((4, f)) < 0.15))
    depth = rng.gamma(8, 1 / 8, n)
    x = rng.poisson(depth[:, None] * base * prog[g]).astype(numpy.float32)
    x.setflags(write=False)
    return x


def flip(components):
    components = numpy.array(components, dtype=numpy.float64)
    for row in components:
        if row[numpy.argmax(numpy.abs(row))] < 0:
            row *= -1
    return components


class Oracle:
    def __init__(self, x):
        x = numpy.asarray(x, dtype=numpy.float64)
        self.rows, self.features = x.shape
        self.mean = x.mean(axis=0)
        self.centred = x - self.mean
        _, s, vt = numpy.linalg.svd(self.centred, full_matrices=False)
        self.singular_values = s
        self.eigenvalues = s ** 2
        self.components = flip(vt)
        self.total = float((self.centred ** 2).sum())

    def gap(self, k):
        """The distance from eigenvalue k to the rest of the spectrum."""
        others = numpy.delete(self.eigenvalues, k)
        return float(numpy.min(numpy.abs(others - self.eigenvalues[k])))

    def assert_separated(self):
        """A condition on the input: a changed generator fails loudly."""
        s = self.singular_values
        assert s[0] / s[1] >= 1.1 and s[1] / s[2] >= 1.1, (
            s[0] / s[1], s[1] / s[2])

    # -- bounds ----------------------------------------------------------
    # Rounding.  The device forms Z = Xc^T (Xc Q) with fl(x - mu) and fp64
    # accumulation: element by element |error| <= gamma_{N+F+4} |Xc|^T |Xc|
    # |Q|, and || |Xc|^T |Xc| ||_2 <= ||Xc||_F^2 = total, so the device
    # iterates on a matrix within gamma_{N+F+4} total of Xc^T Xc in norm; the
    # oracle's SVD is backward stable to a modest multiple of u ||Xc||_2.
    # Both are covered by 4 (N + F) u total on an eigenvalue (Weyl) and by
    # that over the gap on an eigenvector (Davis-Kahan).
    def eigenvalue_rounding(self):
        return 4 * (self.rows + self.features) * U * self.total

    def eigenvalue_bound(self, k, residual):
        """|lambda_k - lambda_k^ref| <= residual_k lambda_1 + rounding: a
        Ritz value lies within its residual norm of an eigenvalue."""
        return residual * self.eigenvalues[0] + self.eigenvalue_rounding()

    def vector_bound(self, k, residual):
        """||v_k - v_k^ref||_2 <= residual_k lambda_1 / gap_k + rounding:
        sin(theta) <= residual norm / gap (Davis-Kahan); the difference of
        two unit vectors is 2 sin(theta / 2) <= sin(theta) (1 + sin(theta)^2)
        for theta <= pi / 2, and the gap seen from the Ritz value is the
        oracle's less the eigenvalue bound: both second order, in `rounding`
        with the rounding of the eigenvectors themselves."""
        gap = self.gap(k)
        first = residual * self.eigenvalues[0] / gap
        rounding = self.eigenvalue_rounding() / gap
        gap_seen = gap - self.eigenvalue_bound(k, residual)
        assert gap_seen > 0.5 * gap
        sine = (residual * self.eigenvalues[0]
                + self.eigenvalue_rounding()) / gap_seen
        second_order = (sine - first - rounding) + sine ** 3
        return first + rounding + max(second_order, 0.0)

    def mean_bound(self, x):
        """|mu_j - mu_j^ref| <= 2 gamma_{N+1} sum_i |x_ij| / N: a sum of N
        values and a division, on the device and in the oracle."""
        x = numpy.abs(numpy.asarray(x, dtype=numpy.float64))
        return 2 * gamma(self.rows + 1) * x.sum(axis=0) / self.rows
