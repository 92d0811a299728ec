"""Pins ``tests/_loglik_oracle.py`` on the host: values and gradients against
mpmath (400 bits: more than 50 digits survive log(1 - 2^-126)), scipy's ``logpmf`` and autograd of
``oracle/likelihoods.py``; every grid value and bound finite with no element
excused; the grid clear of the gate boundaries."""
import functools

import mpmath
import numpy as np
import pytest
import torch

from oracle import likelihoods as lk

import _loglik_oracle as lo

TARGETS = lo.INTEGER_TARGETS + lo.FRACTIONAL_TARGETS
#: fp64's conditioning of the oracle's own form
EPS = 2.0 ** -50


@functools.lru_cache(maxsize=None)
def _grid(name):
    t, pre = lo.grid(name, TARGETS)
    # (values in long double, rounded to fp64: what the device tests' fp64
    #  evaluation is pinned to below)
    out = lo.element(name, t, pre, dtype=np.longdouble)
    return t, pre, out


def _outputs(out):
    yield "lp0", out["lp0"]
    yield "lp", out["lp"]
    for j, g in enumerate(out["g"]):
        yield "g%d" % j, g


@pytest.mark.parametrize("name", lo.KINDS)
def test_grid_is_finite_and_nothing_is_excused(name):
    t, pre, out = _grid(name)
    C = len(lo.combinations(name)[0])
    assert t.size == C * len(TARGETS)
    excused = 0
    for what, x in _outputs(out):
        for part in (x.v, x.e, x.s, lo.bound(x)):
            excused += int((~np.isfinite(part)).sum())
        assert (x.e >= 0).all() and (x.s >= 0).all(), what
        assert np.abs(x.v).max() < 65535 * 87 * 20, what
    print("{}: {} elements, excused {}".format(name, t.size, excused))
    assert excused == 0
    # closed gates: exactly zero, value and bound
    for j, open_ in enumerate(lo.gates(name, pre)):
        g = out["g"][j]
        assert (g.v[~open_] == 0).all() and (g.e[~open_] == 0).all()
        assert (~open_).any() or lo.HEADS[name][j] == "logits"


@pytest.mark.parametrize("name", lo.KINDS)
def test_grid_keeps_clear_of_the_gates(name):
    t, pre, _ = _grid(name)
    assert lo.gate_distance(name, pre) >= 1e-3
    for head, a in zip(lo.HEADS[name], pre):
        for value in lo.HEAD_PRE[head]:       # every value itself occurs
            assert (a == np.float32(value)).any(), (head, value)
        if head in ("log_lambda", "log_r"):
            assert (a == -10).any() and (a == 10).any()


@pytest.mark.parametrize("name", ["zero-inflated poisson",
                                  "zero-inflated negative binomial"])
def test_zero_branch_has_both_regimes(name):
    t, pre, _ = _grid(name)
    zero = t == 0
    T = torch.from_numpy
    a = [T(p[zero].astype(np.float64)) for p in pre]
    log_pi = torch.nn.functional.logsigmoid(a[0].clamp(min=lk.LOGIT_OF_TINY))
    lp = lk.log_prob(name, T(t[zero].astype(np.float64)), tuple(a))
    share = torch.exp(log_pi - lp).numpy()     # pi / p(0)
    assert (share > 0.99).sum() > 10 and (share < 0.01).sum() > 10
    assert ((share > 0.2) & (share < 0.8)).sum() > 10


# ---- mpmath ----------------------------------------------------------------
def _mp_element(name, t, a):
    mp = mpmath.mp
    # (the clip constant as the oracle holds it: the fp64 rounding of
    #  log(2^-126); the device's fp32 rounding of it is part of the count)
    tiny_logit = mp.mpf(lo.LOGIT_OF_TINY)
    t = mp.mpf(float(t))
    a = [mp.mpf(float(v)) for v in a]
    sig = lambda v: 1 / (1 + mp.exp(-v))

    def sigmoid_head(v):
        return (max(v, tiny_logit), 1 if v >= tiny_logit else 0)

    def log_head(v):
        return (min(max(v, -10), 10), 1 if -10 <= v <= 10 else 0)

    def poisson(v):
        ll, gate = log_head(v)
        lam = mp.exp(ll)
        return t * ll - lam, [gate * (t - lam)]

    def nb(vp, vr):
        ap, pg = sigmoid_head(vp)
        lr, rg = log_head(vr)
        r = mp.exp(lr)
        p, q = sig(ap), sig(-ap)
        lp = (r * mp.log(q) + t * mp.log(p)
              + mp.loggamma(r + t) - mp.loggamma(r))
        return lp, [pg * (t * q - r * p),
                    rg * r * (mp.log(q) + mp.psi(0, r + t) - mp.psi(0, r))]

    if name == "bernoulli":
        lp = t * mp.log(sig(a[0])) + (1 - t) * mp.log(sig(-a[0]))
        return lp, lp, [t * sig(-a[0]) - (1 - t) * sig(a[0])]
    if name == "poisson":
        lp, g = poisson(a[0])
    elif name == "negative binomial":
        lp, g = nb(*a)
    else:
        lpb, gb = poisson(a[1]) if len(a) == 2 else nb(a[1], a[2])
        api, gate = sigmoid_head(a[0])
        pi, qi = sig(api), sig(-api)
        if t > 0:
            lp, g = mp.log(qi) + lpb, [-gate * pi] + gb
        else:
            p0 = pi + qi * mp.exp(lpb)
            u, w = pi / p0, qi * mp.exp(lpb) / p0
            lp = mp.log(p0)
            g = [gate * (u * qi - w * pi)] + [w * x for x in gb]
    return lp, lp - mp.loggamma(1 + t), g


@pytest.mark.parametrize("name", lo.KINDS)
def test_oracle_against_mpmath(name):
    t, pre, out = _grid(name)
    n = t.size
    # ~25 elements of every target: a stride coprime to the combinations
    C = n // len(TARGETS)
    pick = np.unique(np.concatenate(
        [k * C + (np.arange(25) * 151 + 7 * k) % C for k in range(len(TARGETS))]))
    worst = {}
    with mpmath.workprec(400):
        for i in pick:
            lp0, lp, g = _mp_element(name, t[i], [p[i] for p in pre])
            want = dict(lp0=lp0, lp=lp, **{"g%d" % j: x for j, x in enumerate(g)})
            for what, x in _outputs(out):
                err = abs(float(mpmath.mpf(float(x.v[i])) - want[what]))
                tol = EPS * float(x.s[i])
                ratio = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
                assert ratio <= 1, (name, what, float(t[i]),
                                    [float(p[i]) for p in pre], float(x.v[i]),
                                    float(want[what]), tol)
                worst[what] = max(worst.get(what, 0.0), ratio)
    print(name, "error / (2^-50 term scale):",
          {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name", lo.KINDS)
def test_fp64_evaluation_is_the_pinned_one(name):
    """The device tests evaluate the oracle in fp64: within a thousandth of
    every bound of the long double evaluation pinned above, and the same error
    and scale."""
    t, pre, out = _grid(name)
    out64 = lo.element(name, t, pre)
    for (what, x), (_, y) in zip(_outputs(out), _outputs(out64)):
        assert (np.abs(x.v - y.v) <= 1e-3 * lo.bound(x)).all(), what
        assert np.allclose(x.e, y.e, rtol=1e-6, atol=0), what
        assert np.allclose(x.s, y.s, rtol=1e-6, atol=0), what


# ---- scipy and autograd of oracle/likelihoods.py -----------------------------
def _lgamma_slack(name, t, pre):
    """what the references' own forms lose: they take lgamma(r + t) - lgamma(r)
    - lgamma(1 + t) (and the digammas) as differences of the large values."""
    from scipy.special import digamma, gammaln
    if "negative binomial" not in name:
        return gammaln(1 + t), 0 * t
    r = np.exp(np.clip(pre[-1].astype(np.float64), -10, 10))
    return (np.abs(gammaln(r + t)) + np.abs(gammaln(r)) + gammaln(1 + t),
            r * (np.abs(digamma(r + t)) + np.abs(digamma(r))))


@pytest.mark.parametrize("name", lo.KINDS)
def test_oracle_against_autograd_of_the_reference_forms(name):
    t, pre, out = _grid(name)
    T = torch.from_numpy
    t64 = t.astype(np.float64)
    a = [T(p.astype(np.float64)).requires_grad_(True) for p in pre]
    lp = lk.log_prob(name, T(t64), tuple(a))
    lp.sum().backward()
    slack_v, slack_g = _lgamma_slack(name, t64, pre)
    # the reference forms round the arguments of the zero branch's
    # exponentials in fp64: ``cond`` times the relative error
    tol = 64 * 2.0 ** -53 * (out["lp"].s + slack_v)
    assert (np.abs(lp.detach().numpy() - out["lp"].v) <= tol).all()
    cond = out["cond"]
    for j, open_ in enumerate(lo.gates(name, pre)):
        got = a[j].grad.numpy()
        g = out["g"][j]
        extra = slack_g if j == len(a) - 1 else 0.0
        if name.startswith("zero-inflated"):
            # the zero branch's weights come from the base log-probability,
            # which the reference forms as (... + lgamma(r)) - lgamma(r)
            extra = extra + np.where(t64 == 0, slack_v * g.s, 0.0)
        assert (np.abs(got - g.v)
                <= 64 * 2.0 ** -53 * cond * (g.s + extra)
                + np.finfo(np.float64).tiny).all(), j   # (fp64's own floor)
        assert (got[~open_] == 0).all() and (g.v[~open_] == 0).all()


@pytest.mark.parametrize("name", ["poisson", "negative binomial"])
def test_oracle_against_scipy_logpmf(name):
    from scipy import stats
    t, pre, out = _grid(name)
    whole = t == np.rint(t)
    t64 = t[whole].astype(np.float64)
    a = [p[whole].astype(np.float64) for p in pre]
    if name == "poisson":
        want = stats.poisson.logpmf(t64, np.exp(np.clip(a[0], -10, 10)))
    else:
        ap = np.maximum(a[0], lo.LOGIT_OF_TINY)
        e = np.exp(-np.abs(ap))
        fail = np.where(ap >= 0, e / (1 + e), 1 / (1 + e))   # 1 - p, stable
        want = stats.nbinom.logpmf(t64, np.exp(np.clip(a[1], -10, 10)), fail)
    finite = np.isfinite(want)
    assert finite.mean() > 0.5
    slack_v, _ = _lgamma_slack(name, t64, a)
    tol = 64 * 2.0 ** -53 * (out["lp"].s[whole] + slack_v)
    if name == "negative binomial":
        # scipy takes log1p(-(1 - p)): the rounding of 1 - p, 2^-53, over p
        # and r log(1 - p) from that rounded 1 - p
        tol = tol + 4 * 2.0 ** -53 * (t64 * (1 + np.exp(-ap))
                                      + np.exp(np.clip(a[1], -10, 10)))
    assert (np.abs(want - out["lp"].v[whole])[finite] <= tol[finite]).all()


def test_lgamma_units_is_a_few_u():
    L = lo.lgamma_units()
    print("L = {:.3f} u".format(L))
    assert 1.0 <= L <= 16.0


def test_difference_forms_at_the_seam():
    """A and D of the two oracle forms (direct sums / shift by 16) agree where
    both apply, and with mpmath at the path boundary of the kernel."""
    r = np.exp(np.linspace(-10, 10, 41))
    for t in (7.0, 8.0, 9.0, 64.0):
        A, D = lo.lgamma_digamma_diff(r, t)
        A2, D2 = lo.lgamma_digamma_diff(r, np.nextafter(t, 100.0))
        scale = t * np.abs(np.log(r + t)) + np.abs(np.log(r)) + 1
        assert (np.abs(A - A2) <= 1e-12 * scale).all()
        assert (np.abs(D - D2) <= 1e-12 * D).all()
    with mpmath.workprec(400):
        for rv in (np.exp(-10.0), 1.0, np.exp(6.4), np.exp(10.0)):
            for t in (1e-3, 0.25, 7.5, 8.5, 9.0, 1e6):
                A, D = lo.lgamma_digamma_diff(np.float64(rv), np.float64(t))
                x = mpmath.mpf(float(rv)) + mpmath.mpf(t)
                wa = mpmath.loggamma(x) - mpmath.loggamma(rv)
                wd = mpmath.psi(0, x) - mpmath.psi(0, rv)
                scale = t * abs(np.log(rv + t)) + abs(np.log(rv)) + 1
                assert abs(float(mpmath.mpf(float(A)) - wa)) <= EPS * scale
                # (the scale of the kernel's general path: D and the four
                #  recurrence terms it takes a difference of)
                scale = float(wd) + sum(1 / (rv + i) for i in range(4))
                assert abs(float(mpmath.mpf(float(D)) - wd)) <= EPS * scale
