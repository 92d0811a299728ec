"""``tests/_px_oracle.py`` against ``oracle.likelihoods`` where the raw-moment
variance of the reference is well conditioned, and against its own evaluation
in ``numpy.longdouble`` everywhere else (no GPU).

The inputs are those of ``tests/test_gpu_px_statistics.py``: every combination
of the heads' edge values, and for the categorised distribution the flat and
the confident rows of logits for 1, 3 and 64 classes.

fp64 against the oracle: 1e-12 relative, on the elements whose variance is
above 1e-6 of the second moment -- plus the ORACLE's own rounding there: its
difference of two moments carries 2^-53 of the second moment per operation
behind either moment.  Counted on its code: m = r exp(a) (3, twice in m^2),
the four-term sum and the product with the share (4), the softmax of C
classes (C + 3) and the sums over them, all of it once in the second moment
and twice in mean^2: 2 C + 30 at most, 3e-9 of a variance at the edge of
that set for one class, where 1e-12 alone would hold the oracle to more than
fp64 gives it.

fp64 against longdouble (u = 2^-64 here):
every form is a product or sum of non-negative terms behind exponentials of
arguments up to 100 in magnitude -- a few hundred roundings of 1.1e-16,
1e-13 relative.
"""
import numpy as np
import pytest
import torch

from oracle import likelihoods as lk

import _px_oracle as px

KINDS = ["poisson", "negative binomial", "zero-inflated poisson",
         "zero-inflated negative binomial", "bernoulli"]


def _relative(got, want):
    got = np.asarray(got, dtype=np.longdouble)
    want = np.asarray(want, dtype=np.longdouble)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())


def _well_conditioned(mean, var):
    return var > 1e-6 * (var + mean * mean)


def _variance_pinned(var, mean, want, classes=0):
    """on the well-conditioned elements: 1e-12 of the variance + the raw-moment
    form's own (2 C + 30) 2^-53 of the second moment."""
    good = _well_conditioned(mean, var)
    second = var + mean * mean
    excess = np.abs(var - want) - (
        1e-12 * var + (2 * classes + 30) * 2.0 ** -53 * second)
    return good, float(excess[good].max())


@pytest.mark.parametrize("name", KINDS)
def test_elementwise_forms(name):
    pre = px.cycle(name, 2, 7, 200)       # 1400 elements: a whole period
    mean, var, cm, cv = px.mean_variance(name, pre)
    assert mean.dtype == np.float64 and (var >= 0).all()
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert np.isfinite(cm).all() and np.isfinite(cv).all()
    want_mean, want_var = lk.mean_variance(
        name, tuple(torch.from_numpy(a.astype(np.float64)) for a in pre))
    assert _relative(mean, want_mean.numpy()) <= 1e-12
    good, excess = _variance_pinned(var, mean, want_var.numpy())
    assert good.mean() > 0.5 and excess <= 0
    long_mean, long_var, _, _ = px.mean_variance(name, pre, np.longdouble)
    assert _relative(mean, long_mean) <= 1e-13
    assert _relative(var, long_var) <= 1e-13


def test_constrained_poisson_rate_passes_through():
    pre = px.cycle("constrained poisson", 1, 3, 50)
    mean, var, cm, cv = px.mean_variance("constrained poisson", pre)
    assert (mean == pre[0]).all() and (var == pre[0]).all()
    assert not cm.any() and not cv.any()


@pytest.mark.parametrize("k_max", [1, 3, 64])
@pytest.mark.parametrize("name", ["poisson", "negative binomial"])
def test_categorised_forms(name, k_max):
    rows = px.logit_rows(k_max)
    pre = px.cycle(name, 1, len(rows), 98)
    logits = np.repeat(rows[:, None, :], 98, axis=1)
    mean, var, cm, cv = px.categorised_mean_variance(name, pre, logits, k_max)
    assert (var >= 0).all() and np.isfinite(var).all()
    assert np.isfinite(cm).all() and np.isfinite(cv).all()
    want_mean, want_var = lk.categorised_mean_variance(
        name, tuple(torch.from_numpy(a.astype(np.float64)) for a in pre),
        torch.from_numpy(logits.astype(np.float64)), k_max)
    assert _relative(mean, want_mean.numpy()) <= 1e-12
    good, excess = _variance_pinned(var, mean, want_var.numpy(), k_max + 1)
    assert good.any() and excess <= 0
    assert k_max == 1 or not good.all()
    # (what the raw-moment form does elsewhere is the reason for this helper)
    long_mean, long_var, _, _ = px.categorised_mean_variance(
        name, pre, logits, k_max, np.longdouble)
    assert _relative(mean, long_mean) <= 1e-13
    assert _relative(var, long_var) <= 1e-13


def test_statistics_and_mixture_sums():
    """The three statistics as ``test_pxmean_stats`` restates them."""
    rng = np.random.default_rng(0)
    S, B, F = 3, 5, 11
    mean = rng.gamma(2.0, 2.0, (S, B, F))
    var = rng.gamma(2.0, 2.0, (S, B, F))
    pm, mov, vom = px.statistics(mean, var)
    assert np.allclose(pm, mean.mean(axis=0), rtol=1e-15)
    assert np.allclose(mov, var.mean(axis=0), rtol=1e-15)
    assert np.allclose(vom, mean.var(axis=0), rtol=1e-12)
    w = rng.random(B)
    pm, mov, vom = px.statistics(mean, var, w)
    wt = w.reshape(B, 1)
    assert np.allclose(pm, mean.mean(axis=0) * wt, rtol=1e-15)
    assert np.allclose(mov, var.mean(axis=0) * wt, rtol=1e-15)
    assert np.allclose(
        vom, ((mean - mean.mean(axis=0) * wt) ** 2).mean(axis=0) * wt,
        rtol=1e-15)


def test_every_combination_of_the_edge_values_occurs():
    pre = px.cycle("zero-inflated negative binomial", 1, 5, 600, spread=0.0)
    seen = {tuple(float(a[i, j]) for a in pre)
            for i in range(5) for j in range(600)}
    assert len(seen) == 14 * 14 * 7
