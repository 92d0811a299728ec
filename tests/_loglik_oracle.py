"""The oracle of the per-element log-likelihood tests: ``log_prob`` of the five
element-wise kinds (Poisson, negative binomial, their zero-inflated forms,
Bernoulli) and its gradient with respect to every head pre-activation, in fp64
on the float32 values the device holds, with the bound each device result is
held to.  ``tests/test_loglik_oracle_host.py`` pins it to mpmath (50 digits),
scipy and autograd of ``oracle/likelihoods.py``.

Values.  Every formula is the stable form of ``csrc/likelihood.hpp`` (log
sigmoid pair from one exponential, the zero branch as a two-term logsumexp),
which in fp64 is the function itself, except the two differences

    A = lgamma(r + t) - lgamma(r),      D = digamma(r + t) - digamma(r):

integer t <= 64 as sum_i log(r + i) and sum_i 1 / (r + i); everything else with
both arguments shifted up by 16 through the recurrence, the shifted difference
taken analytically with seven Bernoulli terms in each tail (the first term
left out is below 3e-20), and the sixteen recurrence terms of D as
sum_i t / ((r + i)(r + t + i)) -- no difference of two sums anywhere.

``element(..., dtype=numpy.longdouble)`` evaluates the same forms beyond fp64
and rounds once; the host test pins that evaluation, and the fp64 one the
device tests use differs from it by fp64's own rounding of the exponentials'
arguments, far below u.

Bounds.  u = 2^-24.  The kernel's chain of fp32 operations is replayed on the
fp64 values by ``V``, which carries next to a value ``v`` the first-order bound
``e`` of its absolute error and its *term scale* ``s``, the sum of the absolute
values of the terms the expression adds (products multiply their factors'
scales).  The accounting is that of ``_px_oracle``:

* an addition, subtraction, multiplication or fused multiply-add: 1 u of its
  result; a constant that is not a float32: 1 u of it;
* the hardware reciprocal: 2 u;
* the fast exponential of x: ``_px_oracle.exp_cost``, 2 (1 + |x|) u, and the
  error of x itself (a formed argument) carried into it; its result may be
  flushed below 2^-126: that much absolute, carried on like any other error;
* the hardware logarithm ``v_log_f32``: no document on the build machine states
  its accuracy, so it was measured once on an MI355X against fp64 ``log2``
  over all 2 130 706 432 normal positive float32: at most 1.9991 u of
  |log2 x| (1 ulp), in every binade and on both sides of 1.  Allowed twice:
  ``LOG_HW`` = 4 u.  ``fast_log`` multiplies by fl(ln 2): 2 more.
  ``fast_log1p(x)`` = log(w) x / (w - 1), w = fl(1 + x): the logarithm, the
  reciprocal (2), two products, and 1 for d = w - 1 standing where x stood;
* ``lgammaf`` (the data term, ``lgamma1p``): ``L`` u of the value.  ROCm ships
  no statement of it on the build machine; ``lgamma_units()`` is twice the worst
  error of float32 ``torch.lgamma`` on the CPU against fp64 over the integers
  1 ... 65 536 (measured on the device over the same integers: 3.33 u at 266).
  The rounding of 1 + t, where it is not exact, enters through digamma(1 + t);
* the series the general path of A and D truncates: the first terms left out,
  1 / (1188 y^9) and 1 / (132 y^10) at both shifted arguments.

The bound of an output is 2 e + 2^-126 -- every count allowed twice, as
everywhere in this suite -- and the count the tests print is e / (u s).
Nothing in ``e`` comes from a device result: a count changes only by pointing
at the operation that was missed.

The fused head kernels take the general path of A and D for a whole wave as
soon as one of its lanes holds a target above 8 or a fractional one, so an
integer target up to 8 may take either: ``path="either"`` bounds it by the
larger of the two chains.
"""
import functools
import itertools

import numpy

from _px_oracle import (LOGIT_OF_TINY, LOG_PRE, SIGMOID_PRE, TINY, U,  # noqa: F401
                        exp_cost)

#: worst error of v_log_f32 measured on an MI355X, in u of |log2 x|; allowed twice
LOG_HW_MEASURED = 1.9991
LOG_HW = 4.0
RCP = 2.0
#: fast_log: the instruction, fl(ln 2), the product
LOG_COST = LOG_HW + 2.0
#: fast_log1p: fast_log, the reciprocal, x * rcp, the product, d for x
LOG1P_COST = LOG_COST + RCP + 3.0

KINDS = ("poisson", "negative binomial", "zero-inflated poisson",
         "zero-inflated negative binomial", "bernoulli")
HEADS = {
    "poisson": ("log_lambda",),
    "negative binomial": ("p", "log_r"),
    "zero-inflated poisson": ("pi", "log_lambda"),
    "zero-inflated negative binomial": ("pi", "p", "log_r"),
    "bernoulli": ("logits",),
}
SIGMOID_HEADS = ("pi", "p", "logits")
#: heads whose gate is a >= logit(tiny) / -10 <= a <= 10 (Bernoulli's logits
#: have no clip)
CLIPPED_SIGMOID = ("pi", "p")
INTERIOR = (-3.0, -1.0, 1.0, 3.0)
HEAD_PRE = {
    "pi": SIGMOID_PRE + INTERIOR, "p": SIGMOID_PRE + INTERIOR,
    "logits": SIGMOID_PRE + INTERIOR,
    "log_lambda": LOG_PRE + INTERIOR, "log_r": LOG_PRE + INTERIOR,
}
INTEGER_TARGETS = (0, 1, 2, 7, 8, 9, 16, 255, 256, 4000, 30000, 65535)
FRACTIONAL_TARGETS = (1e-3, 0.25, 0.5, 1.5, 7.5, 8.5, 100.5, 1e5, 1e6)


# --------------------------------------------------------------------------
# values with their error and term scale
# --------------------------------------------------------------------------
class V:
    """v: fp64 value; e: bound of the absolute error of the fp32 chain that
    formed it; s: its term scale."""
    __slots__ = ("v", "e", "s")

    def __init__(self, v, e=None, s=None):
        v = numpy.asarray(v)
        if v.dtype not in (numpy.float64, numpy.longdouble):
            v = v.astype(numpy.float64)
        self.v = v              # (fp64, or long double to pin the fp64 value)
        zero = numpy.zeros(v.shape)
        self.e = zero if e is None else numpy.asarray(e).astype(
            numpy.float64) + zero
        self.s = (numpy.abs(v) if s is None else numpy.asarray(s)).astype(
            numpy.float64) + zero

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    @staticmethod
    def const(c):
        """a literal of the kernel: one rounding unless it is a float32."""
        exact = float(numpy.float32(c)) == float(c)
        return V(c, 0.0 if exact else U * abs(c))

    def _rounded(self, v, e, s):
        return V(v, e + U * numpy.abs(v), s)

    def __add__(self, o):
        o = V.of(o)
        return self._rounded(self.v + o.v, self.e + o.e, self.s + o.s)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return self._rounded(self.v - o.v, self.e + o.e, self.s + o.s)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return self._rounded(
            self.v * o.v,
            numpy.abs(self.v) * o.e + numpy.abs(o.v) * self.e, self.s * o.s)

    __rmul__ = __mul__

    def __neg__(self):
        return V(-self.v, self.e, self.s)

    def gated(self, gate):
        """times an exact 0 / 1."""
        return V(self.v * gate, self.e * gate, self.s * gate)


def fma(a, b, c):
    a, b, c = V.of(a), V.of(b), V.of(c)
    v = a.v * b.v + c.v
    return V(v, numpy.abs(a.v) * b.e + numpy.abs(b.v) * a.e + c.e
             + U * numpy.abs(v), a.s * b.s + c.s)


def rcp(a):
    v = 1.0 / a.v
    return V(v, a.e * v * v + RCP * U * numpy.abs(v))


def vexp(a):
    v = numpy.exp(a.v)
    return V(v, v * (a.e + exp_cost(a.v) * U) + TINY)


def vlog(a):
    v = numpy.log(a.v)
    return V(v, a.e / numpy.abs(a.v) + LOG_COST * U * numpy.abs(v))


def vlog1p(a):
    v = numpy.log1p(a.v)
    return V(v, a.e / (1.0 + a.v) + LOG1P_COST * U * numpy.abs(v))


def where(c, a, b):
    a, b = V.of(a), V.of(b)
    return V(numpy.where(c, a.v, b.v), numpy.where(c, a.e, b.e),
             numpy.where(c, a.s, b.s))


def larger(a, b):
    """the same value from two chains: the larger error and scale."""
    return V(a.v, numpy.maximum(a.e, b.e), numpy.maximum(a.s, b.s))


def bound(x):
    return 2.0 * x.e + TINY


def count(x):
    """roundings in u of the term scale."""
    return numpy.divide(x.e, U * x.s, out=numpy.zeros_like(x.e),
                        where=x.s > 0)


# --------------------------------------------------------------------------
# A = lgamma(r + t) - lgamma(r), D = digamma(r + t) - digamma(r)
# --------------------------------------------------------------------------
#: B_2k, k = 1 ... 7
_BERNOULLI = (1 / 6, -1 / 30, 1 / 42, -1 / 30, 5 / 66, -691 / 2730, 7 / 6)
_SHIFT = 16


def _stirling_tail(y):
    return sum(B / (2 * k * (2 * k - 1) * y ** (2 * k - 1))
               for k, B in enumerate(_BERNOULLI, 1))


def _digamma_tail(y):
    return 0.5 / y + sum(B / (2 * k * y ** (2 * k))
                         for k, B in enumerate(_BERNOULLI, 1))


def lgamma_digamma_diff(r, t):
    """(A, D) in fp64 for r > 0, t >= 0, without cancellation."""
    r = V(r).v
    t = numpy.asarray(t).astype(r.dtype) + 0 * r
    r = r + 0 * t
    A, D = numpy.zeros_like(r), numpy.zeros_like(r)
    whole = (t == numpy.rint(t)) & (t <= 64)
    for k in range(64):
        on = whole & (k < t)
        if not on.any():
            break
        A[on] += numpy.log(r[on] + k)
        D[on] += 1.0 / (r[on] + k)
    rest = ~whole
    rr, tt = r[rest], t[rest]
    x = rr + tt
    b, a = rr + _SHIFT, x + _SHIFT
    l1 = numpy.log1p(tt / b)
    Ar = (tt * numpy.log(a) + (b - 0.5) * l1 - tt
          + (_stirling_tail(a) - _stirling_tail(b)))
    Dr = l1 - (_digamma_tail(a) - _digamma_tail(b))
    for i in range(_SHIFT):
        Ar = Ar - numpy.log1p(tt / (rr + i))
        Dr = Dr + tt / ((rr + i) * (x + i))
    A[rest], D[rest] = Ar, Dr
    return A, D


def _stirling_chain(iy):
    iy2 = iy * iy
    h = V.const(-1 / 1680)
    h = V.const(1 / 1260) + iy2 * h
    h = V.const(-1 / 360) + iy2 * h
    h = V.const(1 / 12) + iy2 * h
    return iy * h


def _digamma_chain(iy):
    iy2 = iy * iy
    h = V.const(-1 / 240)
    h = V.const(1 / 252) + iy2 * h
    h = V.const(-1 / 120) + iy2 * h
    h = V.const(1 / 12) + iy2 * h
    return V.const(0.5) * iy + iy2 * h


def _small_chain(r, t):
    """lgamma_digamma_diff_small: the product recurrence, t in 1 ... 8."""
    P, Q = V(numpy.ones_like(r.v)), V(numpy.zeros_like(r.v))
    for i in range(8):
        on = i < t
        f = r + float(i) if i else r
        Q = where(on, fma(Q, f, P), Q)
        P = where(on, P * f if i else f, P)
    return vlog(P), Q * rcp(P)


def _general_chain(r, t):
    """lgamma_digamma_diff_general: shift by 4, operation by operation."""
    t = V(t)
    x = r + t
    b, a = r + 4.0, x + 4.0
    ib, ia = rcp(b), rcp(a)
    l1 = vlog1p(t * ib)
    A4 = ((t * vlog(a) + (b - 0.5) * l1) - t) + (
        _stirling_chain(ia) - _stirling_chain(ib))
    ux, ur = x * (x + 3.0), r * (r + 3.0)
    n, d = ux * (ux + 2.0), ur * (ur + 2.0)
    in_, id_ = rcp(n), rcp(d)
    A = A4 - vlog(n * id_)
    D4 = l1 - (_digamma_chain(ia) - _digamma_chain(ib))
    np_ = fma(2.0, x, 3.0) * fma(2.0, ux, 2.0)
    dp = fma(2.0, r, 3.0) * fma(2.0, ur, 2.0)
    D = D4 + (dp * id_ - np_ * in_)
    # the series' first terms left out, at both shifted arguments
    A.e = A.e + 1 / (1188 * a.v ** 9) + 1 / (1188 * b.v ** 9)
    D.e = D.e + 1 / (132 * a.v ** 10) + 1 / (132 * b.v ** 10)
    return A, D


def diff_chain(r, t, path="auto"):
    """(A, D) as ``V``: the values of ``lgamma_digamma_diff``, error and scale
    of the kernel's chain.  ``r``: V; ``t`` > 0 fp64.  path "auto": the product
    recurrence for integer t <= 8 (``lgamma_digamma_diff``); "either": such an
    element may also have taken the general path (fused head kernels)."""
    small = (t <= 8) & (t == numpy.rint(t))
    As, Ds = _small_chain(r, numpy.where(small, t, 1.0))
    Ag, Dg = _general_chain(r, t)
    if path == "either":
        As, Ds = larger(As, Ag), larger(Ds, Dg)
    A, D = where(small, As, Ag), where(small, Ds, Dg)
    A.v, D.v = lgamma_digamma_diff(r.v, t)
    return A, D


# --------------------------------------------------------------------------
# the element
# --------------------------------------------------------------------------
def _log_sigmoid_pair(a):
    """log_sigmoid_pair of common.hpp: (log s(a), log s(-a), s(a), s(-a))."""
    neg = V(-numpy.abs(a.v), a.e, numpy.abs(a.v))
    e = vexp(neg)
    l = vlog1p(e)
    ls_pos = V(numpy.minimum(a.v, 0), a.e * (a.v < 0)) - l
    ls_neg = V(numpy.minimum(-a.v, 0), a.e * (a.v > 0)) - l
    s = rcp(1.0 + e)
    es = e * s
    return (ls_pos, ls_neg, where(a.v >= 0, s, es), where(a.v >= 0, es, s))


def _sigmoid_head(a):
    """(clipped pre-activation, gate): the device's clip constant is the fp32
    rounding of logit(tiny)."""
    gate = (a >= LOGIT_OF_TINY).astype(numpy.float64)
    ap = numpy.maximum(a, LOGIT_OF_TINY)
    return V(ap, U * numpy.abs(ap) * (1 - gate)), gate


def _log_head(a):
    gate = ((a >= -10) & (a <= 10)).astype(numpy.float64)
    return V(numpy.clip(a, -10, 10)), gate


def _poisson_dense(t, a):
    ll, gate = _log_head(a)
    lam = vexp(ll)
    return V(t) * ll - lam, [(V(t) - lam).gated(gate)]


def _nb_dense(t, ap_pre, ar_pre):
    ap, pgate = _sigmoid_head(ap_pre)
    logp, log1mp, p, q = _log_sigmoid_pair(ap)
    lr, rgate = _log_head(ar_pre)
    r = vexp(lr)
    lp = r * log1mp + V(t) * logp
    g = [(V(t) * q - r * p).gated(pgate), (r * log1mp).gated(rgate)]
    return lp, g, r, rgate


def lgamma_units():
    """L: twice the worst error of float32 ``torch.lgamma`` on the CPU against
    fp64 over the integers 1 ... 65 536, in u of the value (no ROCm document on
    the build machine states a figure that could be larger)."""
    return _lgamma_units()


@functools.lru_cache(maxsize=None)
def _lgamma_units():
    import torch
    x = torch.arange(1, 65537, dtype=torch.float64)
    want = torch.lgamma(x)
    got = torch.lgamma(x.float()).double()
    err = (got - want).abs()
    assert bool((err[want == 0] == 0).all())
    rel = err[want != 0] / (U * want[want != 0].abs())
    return 2.0 * float(rel.max())


def lgamma(x):
    """lgamma(x), x >= 1, in the precision of x: shifted up by 16, Stirling's
    series with seven Bernoulli terms (scipy's is fp64 only)."""
    y = x + _SHIFT
    v = (y - 0.5) * numpy.log(y) - y + 0.5 * numpy.log(8 * numpy.arctan(x / x)) \
        + _stirling_tail(y)
    for i in range(_SHIFT):
        v = v - numpy.log(x + i)
    return numpy.where((x == 1) | (x == 2), 0 * v, v)


def data_term(t, L=None):
    """lgamma1p(t) = lgammaf(1 + t) as ``V`` (exactly 0 at t == 0)."""
    from scipy.special import digamma
    L = lgamma_units() if L is None else L
    x = 1.0 + t
    ex = numpy.where(x.astype(numpy.float32).astype(x.dtype) == x, 0.0,
                     U * x).astype(numpy.float64)
    v = lgamma(x)
    e = numpy.abs(digamma(x.astype(numpy.float64))) * ex + L * U * numpy.abs(
        v).astype(numpy.float64)
    live = t != 0
    return V(v * live, e * live)


def element(name, t, pre, path="auto", L=None, fused=False, gw=None,
            dtype=numpy.float64):
    """One element of every kind.  ``t``, ``pre[j]``: float32 arrays of one
    shape.  Returns a dict of ``V``:

    lp0     log_prob + lgamma(1 + t), what ``lik_elem`` returns
    lp      log_prob, as the element-wise entry forms it (lp0 - lgamma1p)
    lg      the data term lgamma(1 + t) (zero for Bernoulli)
    g       d log_prob / d pre_j, clip gates included

    ``dtype``: ``numpy.longdouble`` evaluates the values beyond fp64 (the
    exponentials of the zero branch amplify an fp64 rounding of their arguments
    by the arguments' size); error and scale are fp64 either way.

    ``fused``: the head kernels' order for the last head of the negative-
    binomial kinds, G = fma(gw, r D, gw g_dense); then, and with ``gw`` given,
    ``g`` is the gradient times gw (one rounding more)."""
    t = numpy.asarray(t).astype(dtype)
    pre = [numpy.asarray(a).astype(dtype) + 0 * t for a in pre]
    t = t + 0 * pre[0]
    pos = t > 0
    r = rgate = None
    zi = name.startswith("zero-inflated")
    if name == "bernoulli":
        ls_pos, ls_neg, sig, sig_neg = _log_sigmoid_pair(V(pre[0]))
        omt = 1.0 - V(t)
        lp = V(t) * ls_pos + omt * ls_neg
        g = [V(t) * sig_neg - omt * sig]
    elif name == "poisson":
        lp, g = _poisson_dense(t, pre[0])
    elif name == "negative binomial":
        lp, g, r, rgate = _nb_dense(t, pre[0], pre[1])
    else:
        if name == "zero-inflated poisson":
            lpb, gb = _poisson_dense(t, pre[1])
        else:
            lpb, gb, r, rgate = _nb_dense(t, pre[1], pre[2])
        api, gate = _sigmoid_head(pre[0])
        logpi, log1mpi, pi, qi = _log_sigmoid_pair(api)
        u1, u2 = logpi, log1mpi + lpb
        m = where(u1.v >= u2.v, u1, u2)
        diff = u1 - u2
        y0 = m + vlog1p(vexp(V(-numpy.abs(diff.v), diff.e, diff.s)))
        uu, w = vexp(u1 - y0), vexp(u2 - y0)
        lp = where(pos, u2, y0)
        g = [where(pos, -pi, uu * qi - w * pi).gated(gate)]
        # (the value without the kernel's difference of two nearly equal
        #  products: u (1 - pi) - w pi = pi (1 - pi) (1 - e^lpb) / p(0))
        g[0].v = numpy.where(pos, g[0].v, gate * pi.v * qi.v
                             * -numpy.expm1(numpy.where(pos, 0.0, lpb.v))
                             * numpy.exp(-y0.v))
        g += [where(pos, gj, w * gj) for gj in gb]
    up = None if gw is None else V(numpy.asarray(gw, dtype=numpy.float64))
    if r is not None:
        A, D = diff_chain(r, numpy.where(pos, t, 1.0), path)
        lp = where(pos, lp + A, lp)
        rd = (r * D).gated(rgate)
        if fused:
            g[-1] = where(pos, fma(up, rd, up * g[-1]), up * g[-1])
            g[:-1] = [up * gj for gj in g[:-1]]
        else:
            g[-1] = where(pos, g[-1] + rd, g[-1])
            if up is not None:
                g = [up * gj for gj in g]
    elif up is not None:
        g = [up * gj for gj in g]
    if name == "bernoulli":
        lg = V(numpy.zeros_like(t))
        full = lp
    else:
        lg = data_term(t, L)
        full = lp - lg
    out = {"lp0": lp, "lp": full, "lg": lg, "g": g}
    for x in [lp, full, lg] + g:        # (long double: rounded to fp64 once)
        x.v = x.v.astype(numpy.float64)
    # how far the exponentials of the zero branch amplify a rounding of their
    # arguments (for references that form the same weights in fp64)
    out["cond"] = 1.0 + (numpy.where(pos, 0.0, numpy.abs(u1.v) + numpy.abs(u2.v))
                         .astype(numpy.float64) if zi else 0.0 * lp.s)
    return out


def gates(name, pre):
    """per head: 1 where the clip gate is open (the gradient is exactly zero
    elsewhere)."""
    out = []
    for head, a in zip(HEADS[name], pre):
        a = numpy.asarray(a).astype(numpy.float64)
        if head in CLIPPED_SIGMOID:
            out.append(a >= LOGIT_OF_TINY)
        elif head == "logits":
            out.append(numpy.ones(a.shape, dtype=bool))
        else:
            out.append((a >= -10) & (a <= 10))
    return out


# --------------------------------------------------------------------------
# the grid
# --------------------------------------------------------------------------
def gate_distance(name, pre):
    """smallest distance of a pre-activation to a gate boundary of its head,
    the exactly representable -10 and 10 (inside the gate) left out."""
    best = numpy.inf
    for head, a in zip(HEADS[name], pre):
        a = numpy.asarray(a).astype(numpy.float64)
        if head in CLIPPED_SIGMOID:
            best = min(best, float(numpy.abs(a - LOGIT_OF_TINY).min()))
        elif head != "logits":
            for edge in (-10.0, 10.0):
                off = numpy.abs(a - edge)
                off = off[off > 0]
                if off.size:
                    best = min(best, float(off.min()))
    return best


def combinations(name, seed=0, spread=0.03):
    """[P][C] float32: every combination of the heads' values, the first head
    fastest; half of them on the values themselves, the others moved by
    N(0, spread) so that lanes differ -- and put back where the move would
    land within 1e-3 of a gate boundary."""
    lists = [HEAD_PRE[h] for h in HEADS[name]]
    combos = numpy.asarray(list(itertools.product(*lists[::-1])),
                           dtype=numpy.float64)[:, ::-1].T
    rng = numpy.random.default_rng(seed)
    moved = rng.random(combos.shape) < 0.5
    out = []
    for head, base, mv in zip(HEADS[name], combos, moved):
        a = (base + mv * rng.normal(0, spread, base.shape)).astype(
            numpy.float32)
        edges = ((LOGIT_OF_TINY,) if head in CLIPPED_SIGMOID else
                 () if head == "logits" else (-10.0, 10.0))
        for edge in edges:
            near = numpy.abs(a.astype(numpy.float64) - edge) < 2e-3
            a[near] = base[near].astype(numpy.float32)
        out.append(a)
    return out


def grid(name, targets, seed=0):
    """(t [T * C], pre [P][T * C]) float32: every combination of the heads'
    values against every target, target-major; each target's copy of the
    combinations is moved on its own."""
    ts, pres = [], []
    for k, target in enumerate(targets):
        pre = combinations(name, seed=seed * 1000 + k)
        pres.append(pre)
        ts.append(numpy.full(pre[0].shape, target, dtype=numpy.float32))
    return (numpy.concatenate(ts),
            [numpy.concatenate([p[j] for p in pres])
             for j in range(len(HEADS[name]))])
