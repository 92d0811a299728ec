"""The oracle of the evaluation-statistics tests: mean and variance of the
decoder distributions (va:2665-2713, zero_inflated.py:180-199,
categorised.py:210-253) in forms that are themselves well conditioned, the
three statistics over the samples with the mixture sums of gm:3311-3386, and the
bounds the tests hold the device to.

``oracle.likelihoods`` restates the reference's raw-moment variances,
``E[x^2] - E[x]^2``; fp64 loses them where the variance is below 2^-53 of the
second moment (a confident class of the categorised distribution came out at
-2.8e-14).  Here every variance is a sum of non-negative terms,

    zero-inflated:  (1 - pi) (v + pi m^2)              = mean (q + pi m)
    categorised:    sum_c pi_c (c - mean)^2 + pi_K (v + (m + K - mean)^2)
    Bernoulli:      sigmoid(a) sigmoid(-a)

(m, v = m q: the base distribution's), evaluated in fp64 -- or in
``numpy.longdouble``, which pins the fp64 evaluation -- on the fp32 values the
device holds.

The bounds.  With u = 2^-24 an element's chain of fp32 operations is counted
in units of u of the (non-negative) term it acts on:

* an addition, multiplication or division: 1; the hardware reciprocal: 2;
* the fast exponential of an argument x: 2 (1 + |x|), the (1 + |x|) 2^-23 that
  ``tsne.hip`` states for the same instruction -- and |x| more where x is
  itself the rounded sum or difference of two inputs;
* a sum of n non-negative terms: n - 1 on the whole sum, and the terms' own
  counts weighted by their share of it.

The counts of an element's mean and variance, ``cm`` and ``cv``, come out of
the functions below next to the values; the statistics add ``chain(S, ...)``
for the sum over the samples, the division by S and the weight.  The total is
allowed twice (as ``test_batch_norm_stats_under_cancellation`` does).  Below
the smallest normal fp32, 2^-126, the format holds no relative precision and
the fast exponential returns zero: that much is the absolute floor of every
bound, and nothing else in them is absolute.
"""
import numpy

U = 2.0 ** -24
TINY = 2.0 ** -126
FLOAT32_MAX = float(numpy.finfo(numpy.float32).max)
#: log(float32.tiny) as ``oracle.likelihoods`` holds it; the device's fp32
#: constant is one more rounding of the exponential's argument
LOGIT_OF_TINY = float(numpy.log(numpy.float64(TINY)))

#: pre-activations of a sigmoid head (tests/test_gpu_head_edges.py: PRE) and
#: of a log head: both sides of every clip, the p -> 1 region
SIGMOID_PRE = (-95.0, -88.0, -87.4, -87.2, -11.0, -10.0, -9.99, 0.0, 9.99,
               10.0, 11.0, 16.5, 17.0, 40.0)
LOG_PRE = (-11.0, -10.0, -9.99, 0.0, 9.99, 10.0, 11.0)
HEAD_PRE = {"pi": SIGMOID_PRE, "p": SIGMOID_PRE, "logits": SIGMOID_PRE,
            "log_lambda": LOG_PRE, "log_r": LOG_PRE}

HEADS = {
    "poisson": ("log_lambda",),
    "negative binomial": ("p", "log_r"),
    "zero-inflated poisson": ("pi", "log_lambda"),
    "zero-inflated negative binomial": ("pi", "p", "log_r"),
    "constrained poisson": ("lambda",),
    "bernoulli": ("logits",),
}


def exp_cost(x, formed=False):
    """Roundings of ``__expf(x)``; ``formed``: x is a rounded sum of inputs."""
    x = numpy.abs(numpy.asarray(x, dtype=numpy.float64))
    return 2.0 * (1.0 + x) + (x if formed else 0.0)


def _sigmoid(a):
    """sigmoid(a) without cancellation on either side."""
    e = numpy.exp(-numpy.abs(a))
    s = 1 / (1 + e)
    return numpy.where(a >= 0, s, e * s)


#: sigmoidf: the exponential, 1 + e, the reciprocal (2), e * s
def _sigmoid_cost(a):
    return exp_cost(a) + 4.0


def _count(name, pre, dtype):
    """(m, q, cm, cq): mean, variance / mean and their roundings."""
    if name == "poisson":
        ll = numpy.clip(pre[0].astype(dtype), -10, 10)
        one = numpy.ones_like(ll)
        return numpy.exp(ll), one, exp_cost(ll), 0.0 * exp_cost(ll)
    ap = numpy.maximum(pre[0].astype(dtype), dtype(LOGIT_OF_TINY))
    lr = numpy.clip(pre[1].astype(dtype), -10, 10)
    # exp(lr + ap): a formed argument; 1 + exp(ap): the exponential (of an
    # argument that may be the fp32 clip constant: formed) and the sum
    return (numpy.exp(lr + ap), 1 + numpy.exp(ap), exp_cost(lr + ap, True),
            exp_cost(ap, True) + 1.0)


def mean_variance(name, pre, dtype=numpy.float64):
    """(mean, var, cm, cv) of an element-wise kind.  ``pre``: the head
    pre-activations in registry order (constrained Poisson: the rate)."""
    pre = [numpy.asarray(a) for a in pre]
    if name == "constrained poisson":
        rate = pre[0].astype(dtype)
        zero = numpy.zeros(rate.shape)
        return rate, rate, zero, zero
    if name == "bernoulli":
        a = pre[0].astype(dtype)
        p = _sigmoid(a)
        c = _sigmoid_cost(a)
        return p, p * _sigmoid(-a), c, 2 * c + 1.0
    if name in ("poisson", "negative binomial"):
        m, q, cm, cq = _count(name, pre, dtype)
        return m, m * q, cm, cm + cq + 1.0
    base = name[len("zero-inflated "):]
    m, q, cm, cq = _count(base, pre[1:], dtype)
    api = numpy.maximum(pre[0].astype(dtype), dtype(LOGIT_OF_TINY))
    cs = _sigmoid_cost(api) + numpy.abs(api)      # (the clip constant)
    omp, pi = _sigmoid(-api), _sigmoid(api)
    mean = omp * m
    czm = cs + cm + 1.0
    # q + pi m: the two terms' counts by their share, the product and the sum
    pim = pi * m
    share = pim / (q + pim)
    cf = (1 - share) * cq + share * (cs + cm + 1.0) + 1.0
    return mean, mean * (q + pim), czm, czm + cf + 1.0


def categorised_mean_variance(name, pre, logits, k_max,
                              dtype=numpy.float64):
    """(mean, var, cm, cv) of ``Categorised(dist, cat)``; ``logits``:
    [..., k_max + 1].  The kernel's chain: e_c = exp(l_c - max) (a formed
    argument), their sum (C - 1), one division, p_c = e_c / sum (1); the mean
    as the sum of the C terms c p_c and p_K (m + K); the variance as the sum
    of the C centred terms."""
    K, C = k_max, k_max + 1
    m, q, cdm, cq = _count(name, [numpy.asarray(a) for a in pre], dtype)
    l = numpy.asarray(logits).astype(dtype)
    x = l - l.max(axis=-1, keepdims=True)
    e = numpy.exp(x)
    p = e / e.sum(axis=-1, keepdims=True)
    ce = exp_cost(x, True)
    cp = ce + (p * ce).sum(axis=-1, keepdims=True).astype(numpy.float64) + C + 1.0
    ks = numpy.arange(K).astype(dtype)
    tail = p[..., K]
    terms = numpy.concatenate(
        [p[..., :K] * ks, (tail * (m + K))[..., None]], axis=-1)
    mean = terms.sum(axis=-1)
    costs = numpy.concatenate(
        [cp[..., :K] + 1.0, (cp[..., K] + cdm + 2.0)[..., None]], axis=-1)
    cm = _weighted(terms, costs, mean) + C
    # the tail's distance from the mean as a sum of non-negative terms,
    # (m + K)(1 - p_K) - sum_c c p_c = sum_{c<K} p_c (m + K - c)
    dk = (p[..., :K] * (m[..., None] + K - ks)).sum(axis=-1)
    d = numpy.concatenate([ks - mean[..., None], dk[..., None]], axis=-1)
    centred = p * d * d
    spread = tail * m * q
    var = centred.sum(axis=-1) + spread
    # a centred term: p_c, the difference (1 of |d|: 2 on the square), two
    # products -- the error of ``mean`` inside d is the bound's second and
    # third term, not part of this count.  The tail's distance: K + m is off
    # by u (K + m) + cdm u m, which is at most (K + cdm) u of K + m - c >= m + 1;
    # the difference and the product 2 more; the sum K - 1; squared
    cdm_ = numpy.asarray(cdm, dtype=numpy.float64)[..., None]
    cd = _weighted(p[..., :K] * (m[..., None] + K - ks),
                   cp[..., :K] + K + cdm_ + 2.0, dk) + K
    vterms = numpy.concatenate([centred, spread[..., None]], axis=-1)
    vcosts = numpy.concatenate(
        [cp[..., :K] + 4.0, (cp[..., K] + 2 * cd + 2.0)[..., None],
         (cp[..., K] + cdm + cq + 2.0)[..., None]], axis=-1)
    cv = _weighted(vterms, vcosts, var) + C + 1.0
    return mean, var, cm, cv


def _weighted(terms, costs, total):
    """sum_c terms_c costs_c / total (0 where the total is 0)."""
    t = (terms * costs).sum(axis=-1).astype(numpy.float64)
    total = numpy.asarray(total, dtype=numpy.float64)
    return numpy.divide(t, total, out=numpy.zeros_like(t), where=total > 0)


def statistics(mean, var, weight=None):
    """va:2665-2713 over the leading (sample) axis of [S, B, F] arrays: the
    mean over the samples, the mean of the variances, the variance of the
    means; with ``weight`` [B] the mixture terms of gm:3311-3386: each times
    the cluster's share, the variance taken about the ALREADY WEIGHTED mean
    (gm:3357-3368, reproduced as it is)."""
    w = 1 if weight is None else numpy.asarray(weight).astype(
        mean.dtype).reshape(-1, 1)
    pm = mean.mean(axis=0) * w
    mov = var.mean(axis=0) * w
    vom = ((mean - pm) ** 2).mean(axis=0) * w
    return pm, mov, vom


def peaks(mean, var, weight=None):
    """The largest value each statistic passes through on its way: the sums
    over the samples before the division by S and the weight.  Where one is
    above the fp32 maximum the statistic is +inf on the device, whatever the
    weight makes of it afterwards."""
    pm = statistics(mean, var, weight)[0]
    return mean.sum(axis=0), var.sum(axis=0), ((mean - pm) ** 2).sum(axis=0)


def chain(S, weighted):
    """Roundings of a statistic behind its elements: S - 1 additions, the
    reciprocal of S and the product with it, the weight."""
    return (S - 1) + 2.0 + (1.0 if weighted else 0.0)


def mean_bound(want, c):
    """|got - want| <= 2 c u |want| (+ the subnormal floor)."""
    return 2 * c * U * numpy.abs(want) + TINY


def variance_bound(var, mean, c):
    """|got - want| <= c' u var + 2 c' u |mean| sqrt(var) + (c' u mean)^2 with
    c' = 2 c: the products of a sum of non-negative terms, then the mean the
    squares are centred on.  Nothing in it grows with the second moment."""
    cu = 2 * c * U
    mean = numpy.abs(mean)
    return (cu * var + 2 * cu * mean * numpy.sqrt(var) + (cu * mean) ** 2
            + TINY)


def statistics_bounds(mean, var, cm, cv, weight=None):
    """Bounds of the three statistics of ``statistics(mean, var, weight)``
    from the elements' fp64 values and counts, all [S, B, F].

    mean:      the samples' counts at their worst + the chain.
    mean of variances: ``variance_bound`` per sample, averaged, with c the
               larger of the two counts + the chain (the chain acts on
               non-negative terms: it belongs to the first term, and the
               other two only grow with it).
    variance of means: the same shape on mean_s (m_s - pm)^2.  m_s is off by
               c u m_s and pm by c u pm, so a difference by c u (m_s + pm)
               at most: M = max_s m_s + pm stands where the mean stood, the
               samples' spread sqrt(vom) where sqrt(var) stood."""
    S = mean.shape[0]
    weighted = weight is not None
    w = 1.0 if weight is None else numpy.asarray(
        weight, dtype=numpy.float64).reshape(-1, 1)
    k = chain(S, weighted)
    cm = numpy.asarray(cm, dtype=numpy.float64) + k
    c = numpy.maximum(cm, numpy.asarray(cv, dtype=numpy.float64) + k)
    mean = mean.astype(numpy.float64)
    var = var.astype(numpy.float64)
    pm, mov, vom = statistics(mean, var, weight)
    b_mean = mean_bound(pm, cm.max(axis=0))
    b_mov = variance_bound(var, mean, c).mean(axis=0) * w
    spread = ((mean - pm) ** 2).mean(axis=0)
    b_vom = variance_bound(spread, mean.max(axis=0) + pm,
                           cm.max(axis=0) + 2.0) * w
    return b_mean, b_mov, b_vom


def cycle(name, S, B, F, offset=0, seed=0, spread=0.03):
    """[S * B, F] pre-activations of every head of ``name``: the digits of the
    element number ``b F + f + offset`` in the mixed radix of the heads' value
    lists, so that every combination of the heads' values occurs within one
    period (14, 98 or 1372 elements).  The samples of an element sit at the
    same combination: the first on the values themselves for half of the
    elements, everything else moved by N(0, ``spread``) -- a spread of the
    means far below the means.  As the fp32 values the device holds."""
    rng = numpy.random.default_rng(seed)
    e = numpy.arange(B * F).reshape(1, B, F) + offset
    out = []
    for head in HEADS[name]:
        moved = numpy.ones((S, B, F), dtype=bool)
        moved[0] = rng.random((B, F)) < 0.5
        shift = moved * rng.normal(0, spread, (S, B, F))
        if head == "lambda":       # a rate: e^-11 to 3 e^11
            a = numpy.exp(numpy.asarray(LOG_PRE)[e % 7] + shift) * (1 + e % 3)
        else:
            values = numpy.asarray(HEAD_PRE[head])
            a = values[e % len(values)] + shift
            e = e // len(values)
        out.append(numpy.ascontiguousarray(
            a.reshape(S * B, F).astype(numpy.float32)))
    return out


def logit_rows(k_max, seed=0):
    """[20, k_max + 1] class logits: a flat row; class 0, a middle class and
    the tail class raised by 5, 20 and 40 over it; the same ten again over
    N(0, 1) logits."""
    C = k_max + 1
    rows = [numpy.zeros(C)]
    for c in (0, k_max // 2, k_max):
        for lift in (5.0, 20.0, 40.0):
            row = numpy.zeros(C)
            row[c] = lift
            rows.append(row)
    rows = numpy.asarray(rows)
    noise = numpy.random.default_rng(seed).normal(0, 1, rows.shape)
    return numpy.concatenate([rows, rows + noise]).astype(numpy.float32)
