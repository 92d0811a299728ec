"""Single-product probes of the fused decoder-head kernels (host side: NumPy
fp64 / fp32 and torch on the CPU, no GPU).

The head kernels cut every fp32 operand exactly into three bf16 terms
x = b1 + b2 + b3 (``split3_rn`` of ``decoder_fused3.hip``: round to nearest)
and accumulate the nine exact products of a pair in fp32.  A term of second
order (b2 c2, b1 c3, b3 c1) is at most 2^-18 of a product, far below any
tolerance on a dense contraction.  The probes here make every checked output
element ONE product of two fp32 numbers plus exact zeros, so that the only
error left is the rounding of the fp32 accumulation, and they build the two
numbers so that every guarded term is large against that rounding.

u = 2^-24 throughout.

Operands (``operands``): assembled bitwise as b1 + b2 + b3 with
|b2| in [0.80, 0.98] 2^-9 |x| and |b3| in [0.70, 0.98] 2^-18 |x| (the lower
edge of |b2| is tighter than the 0.55 the terms could have: see "Room for a
defect").  The function asserts that the RN split of the sum returns the
three terms.

Bounds, relative to the one product p = x y (``product_bound``):

* nine terms: the first add to a zero accumulator is exact, the other eight
  round once each by at most u of the partial sum, and a partial sum is at
  most (1 + 2^-8)^2 / (1 - 2^-8)^2 < 1 + 2^-5 of |p| (every term against the
  smallest |p| its leading term allows): 8 u (1 + 2^-5).  The packed block
  (three MFMAs, each one rounding, then two adds of the three accumulator
  rows in GEMM2 / GEMM3) rounds at most four times and is held to the same
  figure;
* six terms: the same and the three missing terms, at most
  (2 . 2^-27 + 2^-36) (1 + 2^-5) < 2^-26 (1 + 2^-5);
* fp32 matrix cores: one rounding, u.

A head's gradient at pre = 0, t = 0 is a constant c_j, and
G_j[r, f] = fl(gw_r c_j).  For the Poisson head c = -1 exactly (t - exp(0)).
Every other c_j is taken from ``oracle.likelihoods`` in fp64, and the bound is
widened by the error of that one scalar: 4 e32_j + 2 u, e32_j the relative
error of the same formula in torch-CPU fp32 against fp64 at that point (the 4
covers the device's fast logarithm and reciprocal against libm, the reasoning
of the 8 x e32 of ``test_gpu_fullcov_kernels.py``), and by u for the rounding
of gw_r c_j where c_j is no power of two.  Measured here (``constants``):

    negative binomial                p   c = -1/2    e32 = 0
                                 log_r   c = -ln 2   e32 = 2.7e-9
    zero-inflated negative binomial pi   c = +1/6    e32 = 3.0e-8
                                     p   c = -1/6    e32 = 3.0e-8
                                 log_r   c = -ln 2/3 e32 = 2.7e-9

Room for a defect.  A lost term T leaves the other eight, whose accumulation
errs by at most 7 u: the result is at least |T| - 7 u |p| (1 + 2^-5) from the
product the device's G makes, which itself is within the constant's widening
w_j (0 to 5 u) of the exact value; that has to exceed TWICE the bound
8 u (1 + 2^-5) + w_j.  So |T| > (23.7 + 3 w_j) u |p|, at most 38.7 u.  With the
operands above |b2 c2| >= 0.64 . 2^-18 = 41 u, |b1 c3| >= 0.70 . 2^-18
(1 - 2^-8) = 44.6 u and the first-order terms are 2^-10: every one of hh, hm,
mh, mm, hl, lh stands clear on every head (at |b2| >= 0.55 the mm term could
be 19.4 u and did not).

The terms of G.  On a head whose constant is not exact, G = fl(gw c) with c
any fp32 value within the widening of c64 (``c_candidates``: up to six
values).  gw is drawn from a pool (``_gw_pool``) in which, for EVERY head and
EVERY such c, the three terms of G keep MID, LOW and the mid term's sign: a
shift of c by a few of its last places moves the lo term of G by a few of its
18 to 63 units.  So the probes control the terms of both operands of every
product on every head.

The mid term's sign.  In all operands of one probe b2 has the sign of b1
(even seeds) or the other sign (odd seeds); b3 is of either sign.  Then
b1 c2 + b2 c1 of a pair never cancels, and terms paired only by their own
index (three products instead of nine) are seen on every element too.

One product per checked element.  With two or three heads dd[r, h] is a sum
over the heads.  The GEMM2 probe keeps one product per head as non-zero, but
scales the heads other than the LEADING one, (h + seed) mod P, by 2^-40: they
then add less than 2^-31 of the leading product, the exact value carries them,
and the bound has their whole size twice over.  Over three seeds every head
leads in every column h.

GEMM1 probe (``gemm1_probe``).  pre = d W + b is no output; it is observed
through G, which is exponential in it.  Row r has one live column h(r), row
h of ONE head J(h) = (h + seed) mod P has one live gene f(h), and
pre_J[r, f(h(r))] = d[r, h(r)] W_J[h(r), f(h(r))] has magnitude 6 to 9.5; every
other pre-activation is 0 and t = 0.  (One live head per row, not one gene
per head: with all heads live dd[r, h(r)] would again be a sum of products
of very different sizes.)  dd[r, h(r)] = G_J[r, f] W_J[h(r), f] then shows a
relative error eps of the product d W as |pre| eps.  Its operands carry
larger terms still (MID1, LOW1), because its bound also holds the
exponential's own 2 u |pre| and the likelihood's error.  The sign of pre is
the side on which the head's gradient is exponential: either for log_lambda
and the log_r of the negative binomial, negative for p, pi and the log_r of
the zero-inflated kind.  The pi head is probed with t = 1 on its live gene:
in the zero branch its gradient u qi - w pi is a difference a third the size
of its terms, whose own rounding leaves no room for a factor of two; at
t > 0 it is -sigmoid(pre).  A forward-only launch (|pre| from 8) probes ONLY
the exponential heads (log_lambda, log_r, at pre > 0, where the live gene's
-e^pre dominates ll[r]) -- for the zero-inflated kind with t = 1 on the live
gene, since at t = 0 its log likelihood never falls below log 1/2; the
sigmoid heads' forward GEMM1 stays with the existing tests.  ``lik_dense_t0``
and ``lik_zinb_t1`` count the likelihood's own fp32 error along ``lik_dense``
/ ``lik_elem`` (likelihood.hpp).  Columns without a live row (H > rows) are
listed as ``dead_cols``: their rows of dW are exactly 0.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -5            # a partial sum against |p| (docstring)
NAMES = ["poisson", "negative binomial", "zero-inflated negative binomial"]
HEADS = {"poisson": 1, "negative binomial": 2,
         "zero-inflated negative binomial": 3}
MINOR = 2.0 ** -40                  # the heads beside the leading one (GEMM2)

# the nine term pairs (a, b): term a of the first operand, b of the second
ALL9 = [(a, b) for a in range(3) for b in range(3)]
SIX = [(a, b) for a, b in ALL9 if a + b < 3]
GUARDED = {"hh": (0, 0), "hm": (0, 1), "mh": (1, 0), "mm": (1, 1),
           "hl": (0, 2), "lh": (2, 0)}
ORDERS = {
    # as the kernels issue them: a = 2..0 outside, b = 2..0 inside
    "small first": [(a, b) for a in (2, 1, 0) for b in (2, 1, 0)],
    "large first": [(a, b) for a in (0, 1, 2) for b in (0, 1, 2)],
    "by size": sorted(ALL9, key=lambda ab: (-(ab[0] + ab[1]), ab[0])),
}


# ---------------------------------------------------------------- operands
def _bf16_rn(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    bits = (bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1)))
    return (bits & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x):
    """The RN split of ``split3_rn``: three fp32 arrays, each a bf16 value,
    that add up to x exactly."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b1 = _bf16_rn(x)
    r1 = x - b1                      # at most 16 significant bits: exact
    b2 = _bf16_rn(r1)
    b3 = r1 - b2                     # at most 8: exact
    assert np.array_equal(b1.astype(np.float64) + b2 + b3, x.astype(np.float64))
    assert np.array_equal(_bf16_rn(b3), b3)
    return b1, b2, b3


MID = (0.80, 0.98)                   # |b2| / (2^-9 |x|)
LOW = (0.70, 0.98)                   # |b3| / (2^-18 |x|)
# the GEMM1 probe's operands: its bound also carries the exponential's own
# 2 u |pre| and the likelihood's error, so its terms are larger still
MID1 = (0.85, 0.98)
LOW1 = (0.80, 0.98)


def term_ratios(x):
    """(|b2| / 2^-9 |x|, |b3| / 2^-18 |x|, sign(b1 b2)) of fp32 values."""
    b1, b2, b3 = split3(x)
    ax = np.abs(np.asarray(x, dtype=np.float64))
    return (np.abs(b2) / (2.0 ** -9 * ax), np.abs(b3) / (2.0 ** -18 * ax),
            np.sign(b1) * np.sign(b2))


def operands(shape, rng, lo=0.25, hi=4.0, mid=MID, low=LOW, mid_sign=None):
    """fp32 values with random sign, |x| log-uniform in [lo, hi] (scalars or
    arrays of ``shape``), assembled as b1 + b2 + b3 with |b2| in mid 2^-9 |x|
    and |b3| in low 2^-18 |x|.  ``mid_sign``: +1 / -1 -- b2 of the sign of b1 /
    of the other sign everywhere (then b1 c2 + b2 c1 of two such values cannot
    cancel); None: either.  Asserts that ``split3`` returns the terms."""
    n = int(np.prod(shape))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), shape).reshape(n)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), shape).reshape(n)
    out = np.zeros(n, dtype=np.float32)
    todo = np.arange(n)
    for _ in range(400):
        if todo.size == 0:
            break
        m = todo.size
        mag = np.exp(rng.uniform(np.log(lo[todo]), np.log(hi[todo])))
        b1 = _bf16_rn((mag * rng.choice([-1.0, 1.0], m)).astype(np.float32))
        a1 = np.abs(b1.astype(np.float64))
        s2 = rng.choice([-1.0, 1.0], m) if mid_sign is None else mid_sign * np.sign(b1)
        # b2: a bf16 value near the drawn size; b3: a multiple of the last
        # place of an fp32 number of the size of b1 (anything finer would not
        # fit the 24 bits of x)
        b2 = _bf16_rn((rng.uniform(mid[0] + 0.005, mid[1] - 0.005, m) * 2.0 ** -9
                       * a1 * s2).astype(np.float32))
        place = 2.0 ** (np.floor(np.log2(a1)) - 23)
        b3 = np.rint(rng.uniform(low[0] + 0.005, low[1] - 0.005, m) * 2.0 ** -18
                     * a1 / place) * place * rng.choice([-1.0, 1.0], m)
        x64 = b1.astype(np.float64) + b2.astype(np.float64) + b3
        x = x64.astype(np.float32)
        ok = (x.astype(np.float64) == x64)
        s1, t2, t3 = split3(x)
        ok &= (s1 == b1) & (t2 == b2) & (t3.astype(np.float64) == b3)
        ax = np.abs(x64)
        r2, r3 = np.abs(b2) / (2.0 ** -9 * ax), np.abs(b3) / (2.0 ** -18 * ax)
        ok &= (r2 >= mid[0]) & (r2 <= mid[1]) & (r3 >= low[0]) & (r3 <= low[1])
        ok &= (ax >= lo[todo]) & (ax <= hi[todo])
        out[todo[ok]] = x[ok]
        todo = todo[~ok]
    assert todo.size == 0, "operands: no value found for %d places" % todo.size
    check_operands(out, mid, low, mid_sign)
    return out.reshape(shape)


def check_operands(x, mid=MID, low=LOW, mid_sign=None):
    """The promise of ``operands`` on a finished array (non-zero entries)."""
    x = np.asarray(x, dtype=np.float32).ravel()
    x = x[x != 0]
    r2, r3, s = term_ratios(x)
    assert r2.min() >= mid[0] and r2.max() <= mid[1], (r2.min(), r2.max())
    assert r3.min() >= low[0] and r3.max() <= low[1], (r3.min(), r3.max())
    assert mid_sign is None or (s == mid_sign).all()


def mid_sign_of(seed):
    """The probes' b2 is of the sign of b1 on even seeds, of the other on odd."""
    return 1.0 if seed % 2 == 0 else -1.0


# --------------------------------------------------------------- emulation
PLAIN, SWAPPED, DOUBLED = (0, 1, 2), (0, 2, 1), (0, 2, 2)


def _terms(x, planes=PLAIN):
    """The three terms as a kernel with a plane mix-up would read them:
    SWAPPED -- planes 1 and 2 exchanged; DOUBLED -- plane 2 read where plane 1
    is meant as well."""
    t = split3(x)
    return [t[k] for k in planes]


def emulate(a, b, terms=ALL9, order=ORDERS["small first"], planes_a=PLAIN,
            planes_b=PLAIN):
    """fp32 result of accumulating, in ``order``, those of the nine exact
    products a_i b_j whose pair is in ``terms``: one fp32 rounding per add.
    ``planes_a``, ``planes_b``: which plane each term index reads."""
    A, B = _terms(a, planes_a), _terms(b, planes_b)
    acc = np.zeros(np.shape(a), dtype=np.float32)
    terms = set(terms)
    for i, j in order:
        if (i, j) in terms:
            prod = A[i].astype(np.float64) * B[j].astype(np.float64)
            p32 = prod.astype(np.float32)
            assert np.array_equal(p32.astype(np.float64), prod)   # 8 x 8 bits
            acc = acc + p32          # fp32 add, round to nearest even
    return acc


def emulate_packed(a, b, terms=ALL9, order=(2, 1, 0), planes_a=PLAIN,
                   planes_b=PLAIN):
    """The packed block: for each term j of the second operand ONE matrix
    instruction sums the products with the (up to) three terms of the first
    and the accumulator, with one rounding."""
    A, B = _terms(a, planes_a), _terms(b, planes_b)
    acc = np.zeros(np.shape(a), dtype=np.float32)
    terms = set(terms)
    for j in order:
        s = acc.astype(np.float64)
        for i in range(3):
            if (i, j) in terms:
                s = s + A[i].astype(np.float64) * B[j].astype(np.float64)
        acc = s.astype(np.float32)
    return acc


DIAGONAL = [(0, 0), (1, 1), (2, 2)]  # term a of d against term a of W only


def product_bound(arith):
    """Relative bound of one product by the arithmetic (module docstring)."""
    if arith == "fp32":
        return U
    if arith == "bf16x9":
        return 8 * U * SLACK
    if arith == "bf16x6":
        return (8 * U + 2.0 ** -26) * SLACK
    raise ValueError(arith)


# ---------------------------------------------------- the heads' constants
@functools.lru_cache(maxsize=None)
def constants(name):
    """(c64, e32, exact) per head at pre = 0, t = 0: the gradient of the log
    likelihood in fp64, the relative error of the same formula in torch-CPU
    fp32, and whether gw c is formed without error (a power of two, e32 = 0)."""
    import torch
    from oracle import likelihoods as lk
    out = {}
    for dtype in (torch.float64, torch.float32):
        pre = [torch.zeros(1, dtype=dtype, requires_grad=True)
               for _ in range(HEADS[name])]
        lk.log_prob(name, torch.zeros(1, dtype=dtype), tuple(pre)).sum().backward()
        out[dtype] = [float(p.grad[0]) for p in pre]
    c64 = out[torch.float64]
    e32 = [abs(a - b) / abs(b) for a, b in zip(out[torch.float32], c64)]
    exact = [e == 0.0 and math.frexp(abs(c))[0] == 0.5 for c, e in zip(c64, e32)]
    if name == "poisson":
        assert c64 == [-1.0] and exact == [True]
    return c64, e32, exact


def constant_widening(name, j):
    """Relative error allowed for G = fl(gw c_j) against gw c64_j."""
    c64, e32, exact = constants(name)
    if name == "poisson":
        return 0.0                   # t - exp(0) = -1
    return 4 * e32[j] + 2 * U + (0.0 if exact[j] else U)


def c_candidates(name, j):
    """Every fp32 value the device's constant c_j may be: those within the
    widening 4 e32 + 2 u of c64 (one value where the constant is exact)."""
    c64, e32, exact = constants(name)
    if name == "poisson" or exact[j]:
        return np.array([c64[j]], dtype=np.float32)
    widen = (4 * e32[j] + 2 * U) * abs(c64[j])
    near = np.float32(c64[j])
    out = [near]
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        c = near
        while True:
            c = np.nextafter(c, toward)
            if abs(float(c) - c64[j]) > widen:
                break
            out.append(c)
    return np.sort(np.array(out, dtype=np.float32))


def G_of(gw, c32):
    """fl(gw c): the fp64 product of two fp32 numbers is exact, its rounding
    to fp32 the device's one multiply."""
    return (_f64(gw) * np.float64(c32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _gw_pool(name, mid_sign, n):
    """n values gw such that G_j = fl(gw c) keeps the promise of ``operands``
    (MID, LOW, the sign of the mid term) for EVERY head j and EVERY candidate
    c of that head: a shift of c by a few of its last places moves the lo term
    of G by a few units of 18 to 63, and gw is drawn until it stays inside.
    Head 0's G is built by ``operands`` and divided by c; the rest by
    rejection."""
    P = HEADS[name]
    rng = np.random.default_rng([9, P, int(mid_sign > 0), n])
    cands = [c_candidates(name, j) for j in range(P)]
    found = []
    have = 0
    for _ in range(4000):
        if have >= n:
            break
        c0 = float(cands[0][len(cands[0]) // 2])
        g0 = operands((20000,), rng, 0.25 * abs(c0), 4.0 * abs(c0), mid_sign=mid_sign)
        gw = (_f64(g0) / c0).astype(np.float32)
        for j in range(P):
            for c in cands[j]:
                if gw.size == 0:
                    break
                r2, r3, sg = term_ratios(G_of(gw, c))
                gw = gw[(r2 >= MID[0]) & (r2 <= MID[1]) & (r3 >= LOW[0])
                        & (r3 <= LOW[1]) & (sg == mid_sign)]
        found = [np.unique(np.concatenate(found + [gw]))]
        have = found[0].size
    assert have >= n, "gw pool: %d of %d" % (have, n)
    pool = rng.permutation(found[0])[:n]
    pool.setflags(write=False)
    return pool


def gw_values(name, n, mid_sign, rng):
    """n distinct values of the pool, in random order (Poisson: G = -gw)."""
    if name == "poisson":
        return operands((n,), rng, mid_sign=mid_sign)
    pool = _gw_pool(name, mid_sign, 640 if HEADS[name] == 2 else 256)
    return pool[rng.permutation(pool.size)[:n]].copy()


def _c32(name, heads):
    """{"lo", "near", "hi"}: the smallest, nearest and largest candidate of
    the constant of each head in ``heads`` (an array of head indices)."""
    cands = [c_candidates(name, j) for j in range(HEADS[name])]
    pick = {"lo": lambda c: c[0], "near": lambda c: c[len(c) // 2], "hi": lambda c: c[-1]}
    return {k: np.array([f(c) for c in cands], dtype=np.float32)[heads]
            for k, f in pick.items()}


# ------------------------------------------------------------------ probes
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _finish(probe):
    for a in [probe["d"], probe["t"], probe["gw"]] + probe["W"] + probe["b"]:
        assert a.dtype == np.float32
        a.setflags(write=False)
    return probe


def _live_rows(rows, H, seed, rng):
    """r(h): the live row of column h.  The first 32 columns take the
    positions (h + 11 seed) mod 32 of a 32-row tile -- over seeds 0, 1, 2
    every position, whatever H >= 20 -- in a random whole tile; the others
    any row not yet taken, and beyond ``rows`` columns the rows serve again."""
    r = np.empty(H, dtype=np.int64)
    full = rows // 32
    free = np.ones(rows, dtype=bool)
    for h in range(min(H, 32)):
        r[h] = 32 * rng.integers(0, full) + (h + 11 * seed) % 32
        free[r[h]] = False
    rest = rng.permutation(np.flatnonzero(free))
    again = rng.permutation(rows)
    for h in range(32, H):
        k = h - 32
        r[h] = rest[k] if k < rest.size else again[(k - rest.size) % rows]
    return r


def gemm3_probe(name, rows, H, F, seed, arith="bf16x9", two_groups=False):
    """dW = d^T G with one live row per column h.  W = b = t = 0: every
    pre-activation is 0 and G_j[r, f] = fl(gw_r c_j); gw = 0 on the rows that
    are not live.  Checked: dW_j[h, f] = d[r(h), h] gw_r(h) c_j for EVERY
    (h, f), db_j[f] = c_j sum of gw (a sum: held to its own bound), dd = 0."""
    P = HEADS[name]
    rng = np.random.default_rng([3, seed, H, rows, P])
    r = _live_rows(rows, H, seed, rng)
    if two_groups:
        assert (r < rows // 2).any() and (r >= (rows + 1) // 2 + 32).any()
    live = np.unique(r)
    d = np.zeros((rows, H), dtype=np.float32)
    ms = mid_sign_of(seed)
    d[r, np.arange(H)] = operands((H,), rng, mid_sign=ms)
    gw = np.zeros(rows, dtype=np.float32)
    gw[live] = gw_values(name, live.size, ms, rng)
    c64, _, exact = constants(name)
    checks = []
    x = np.broadcast_to(d[r, np.arange(H)][:, None], (H, F))
    y = np.broadcast_to(gw[r][:, None], (H, F))
    for j in range(P):
        rel = product_bound(arith) + constant_widening(name, j)
        value = _f64(x) * _f64(y) * c64[j]
        checks.append({"out": "dW", "head": j, "x": x, "y": y, "c": c64[j],
                       "exact_c": exact[j], "exact": value, "c32": _c32(name, j),
                       "bound": rel * np.abs(value), "rel": rel,
                       "row": np.broadcast_to(r[:, None], (H, F))})
        # db_j[f]: n live rows through the ones row (or the producers' adds):
        # n - 1 adds of at most u of the sum of sizes, on top of each term's
        # own bound
        sizes = np.abs(_f64(gw[live]) * c64[j]).sum()
        checks.append({"out": "db", "head": j,
                       "exact": np.full(F, _f64(gw[live]).sum() * c64[j]),
                       "bound": np.full(F, (rel + live.size * U) * sizes),
                       "rel": None})
    zero = np.zeros
    return _finish({
        "name": name, "probe": "gemm3", "rows": rows, "H": H, "F": F, "P": P,
        "seed": seed, "d": d, "gw": gw, "t": zero((rows, F), dtype=np.float32),
        "W": [zero((H, F), dtype=np.float32) for _ in range(P)],
        "b": [zero(F, dtype=np.float32) for _ in range(P)],
        "checks": checks, "zeros": ["dd"], "live_row": r})


def gemm2_probe(name, rows, H, F, seed, arith="bf16x9"):
    """dd = sum_j G_j W_j^T with one non-zero gene per row of W_j.  d = b =
    t = 0; gw full-mantissa on every row.  Checked: dd[r, h] = sum_j gw_r c_j
    W_j[h, f_j(h)] for EVERY (r, h) -- the leading head's product and 2^-40
    of the others' (module docstring); dW = 0."""
    P = HEADS[name]
    assert F >= P * H, "disjoint genes for every (head, h)"
    rng = np.random.default_rng([2, seed, H, rows, P])
    genes = rng.permutation(F)[:P * H].reshape(P, H)      # f_j(h)
    lead = (np.arange(H) + seed) % P
    ms = mid_sign_of(seed)
    gw = gw_values(name, rows, ms, rng)
    W = [np.zeros((H, F), dtype=np.float32) for _ in range(P)]
    w = operands((P, H), rng, mid_sign=ms)
    for j in range(P):
        w[j, lead != j] *= np.float32(MINOR)              # (a power of two)
        W[j][np.arange(H), genes[j]] = w[j]
    c64, _, exact = constants(name)
    c = np.asarray(c64)
    wl = w[lead, np.arange(H)]                            # the leading terms
    x = np.broadcast_to(gw[:, None], (rows, H))
    y = np.broadcast_to(wl[None, :], (rows, H))
    cl = np.broadcast_to(c[lead][None, :], (rows, H))
    leading = _f64(x) * _f64(y) * cl
    every = _f64(gw)[:, None, None] * (c[:, None] * _f64(w))[None]   # [r, j, h]
    minor = np.abs(every).sum(axis=1) - np.abs(leading)
    assert (minor <= 2.0 ** -31 * np.abs(leading)).all()
    rel = np.array([product_bound(arith) + constant_widening(name, j)
                    for j in range(P)])[lead][None, :]
    checks = [{"out": "dd", "head": np.broadcast_to(lead[None, :], (rows, H)),
               "x": x, "y": y, "c": cl, "c32": {
                   k: np.broadcast_to(v[None, :], (rows, H))
                   for k, v in _c32(name, lead).items()},
               "exact_c": np.broadcast_to(
                   np.asarray(exact)[lead][None, :], (rows, H)),
               "exact": every.sum(axis=1), "leading": leading, "minor": minor,
               "bound": rel * np.abs(leading) + 2 * minor,
               "rel": np.broadcast_to(rel, (rows, H)),
               "gene": np.broadcast_to(genes[lead, np.arange(H)][None, :], (rows, H))}]
    for j in range(P):
        sizes = np.abs(_f64(gw) * c64[j]).sum()
        checks.append({"out": "db", "head": j,
                       "exact": np.full(F, _f64(gw).sum() * c64[j]),
                       "bound": np.full(F, (product_bound(arith) + rows * U
                                            + constant_widening(name, j)) * sizes),
                       "rel": None})
    zero = np.zeros
    return _finish({
        "name": name, "probe": "gemm2", "rows": rows, "H": H, "F": F, "P": P,
        "seed": seed, "d": zero((rows, H), dtype=np.float32), "gw": gw,
        "t": zero((rows, F), dtype=np.float32), "W": W,
        "b": [zero(F, dtype=np.float32) for _ in range(P)],
        "checks": checks, "zeros": ["dW"], "genes": genes, "lead": lead})


# ------------------------------------- lik_dense with a running error bound
# Every quantity is (value in fp64, bound of the absolute error of the fp32
# device value), to first order; ``gemm1_bound`` adds 2^-10 of the result for
# the second order.  The device operations, as likelihood.hpp / common.hpp use
# them: an fp32 add or multiply rounds by u of its result; __expf(z) is
# v_exp_f32 (1 ulp = 2 u) of fl(z log2 e), the constant and the product 2 u |z|
# (as tests/test_gpu_tsne.py counts them); fast_rcp is v_rcp_f32, 1 ulp = 2 u;
# fast_log is v_log_f32 (2 u) times ln 2 (the constant and the product 2 u):
# 4 u of its value; fast_log1p(x) = fast_log(1 + x) x rcp((1 + x) - 1) -- the
# rounding of 1 + x cancels to second order, leaving the logarithm (4 u), the
# reciprocal (2 u), two products (2 u) and u for the method: 9 u of its value.
# min / max / negation / a product with an exact 0 or 1 add nothing.
def _add(a, b, sign=1.0):
    v = a[0] + sign * b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _mul(a, b):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + U * np.abs(v)


def _exp(z):
    v = np.exp(z[0])
    return v, v * (z[1] + 2 * U * np.abs(z[0]) + 2 * U)


def _rcp(a):
    v = 1.0 / a[0]
    return v, np.abs(v) * (a[1] / np.abs(a[0]) + 2 * U)


def _log1p(x):
    v = np.log1p(x[0])
    return v, x[1] / (1.0 + x[0]) + 9 * U * np.abs(v)


def _neg(a):
    return -a[0], a[1]


def _log_sigmoid_pair(a):
    e = _exp((-np.abs(a[0]), a[1]))
    l = _log1p(e)
    ls_pos = _add((np.minimum(a[0], 0.0), a[1]), l, -1.0)
    ls_neg = _add((np.minimum(-a[0], 0.0), a[1]), l, -1.0)
    s = _rcp(_add((np.ones_like(a[0]), np.zeros_like(a[0])), e))
    es = _mul(e, s)
    pos = a[0] >= 0
    pick = lambda x, y: (np.where(pos, x[0], y[0]), np.where(pos, x[1], y[1]))
    return ls_pos, ls_neg, pick(s, es), pick(es, s)


def lik_dense_t0(name, pre):
    """``lik_dense<KIND, true>`` at t = 0 inside the clips: (lp, [g_j]) as
    (value, error bound) pairs; ``pre``: one pair per head."""
    for a in pre:
        assert (np.abs(a[0]) < 10.0).all()
    if name == "poisson":
        lam = _exp(pre[0])
        return _neg(lam), [_neg(lam)]          # 0 ll - lam, 0 - lam: exact
    nb = pre if name == "negative binomial" else pre[1:]
    logp, log1mp, p, q = _log_sigmoid_pair(nb[0])
    r = _exp(nb[1])
    lpb = _mul(r, log1mp)                       # + 0 logp
    gb = [_neg(_mul(r, p)), _mul(r, log1mp)]   # 0 q - r p; rgate = 1
    if name == "negative binomial":
        return lpb, gb
    logpi, log1mpi, pi, qi = _log_sigmoid_pair(pre[0])
    u1, u2 = logpi, _add(log1mpi, lpb)
    m = (np.maximum(u1[0], u2[0]), np.maximum(u1[1], u2[1]))
    diff = _add(u1, u2, -1.0)
    y0 = _add(m, _log1p(_exp((-np.abs(diff[0]), diff[1]))))
    uu, w = _exp(_add(u1, y0, -1.0)), _exp(_add(u2, y0, -1.0))
    g0 = _add(_mul(uu, qi), _mul(w, pi), -1.0)
    return y0, [g0, _mul(w, gb[0]), _mul(w, gb[1])]


def lik_zinb_t1(pre):
    """``lik_elem<LK_ZINB, true>`` at t = 1 (the t > 0 branch and the sparse
    correction: P = r, A = fast_log(r), D = rcp(r); lgamma(1 + t) = 0)."""
    for a in pre:
        assert (np.abs(a[0]) < 10.0).all()
    logp, log1mp, p, q = _log_sigmoid_pair(pre[1])
    r = _exp(pre[2])
    lpb = _add(_mul(r, log1mp), logp)
    logpi, log1mpi, pi, qi = _log_sigmoid_pair(pre[0])
    A = (pre[2][0], r[1] / r[0] + 4 * U * np.abs(pre[2][0]))
    lp = _add(_add(log1mpi, lpb), A)
    g2 = _add(_mul(r, log1mp), _mul(r, _rcp(r)))
    return lp, [_neg(pi), _add(q, _mul(r, p), -1.0), g2]


def lik_live(name, pre, tl):
    """(lp, [g_j]) with the running bound at t = tl (0 or 1 per element; 1
    only for the zero-inflated kind)."""
    lp, g = lik_dense_t0(name, pre)
    if not np.any(tl):
        return lp, g
    assert name == NAMES[2]
    lp1, g1 = lik_zinb_t1(pre)
    sel = lambda x, y: (np.where(tl > 0, y[0], x[0]), np.where(tl > 0, y[1], x[1]))
    return sel(lp, lp1), [sel(x, y) for x, y in zip(g, g1)]


def oracle_t0(name, pre, tl=None):
    """(lp, [g_j]) of the oracle in fp64 at t = 0 (or ``tl``); ``pre``: arrays
    per head."""
    import torch
    from oracle import likelihoods as lk
    ps = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
          .requires_grad_(True) for a in pre]
    t = torch.zeros_like(ps[0]) if tl is None else torch.from_numpy(
        np.array(np.broadcast_to(tl, ps[0].shape), dtype=np.float64))
    lp = lk.log_prob(name, t, tuple(ps))
    lp.sum().backward()
    return lp.detach().numpy(), [p.grad.numpy() for p in ps]


# which sign of pre makes the gradient of head j exponential in it at t = 0
# (0: either).  log_r of the zero-inflated kind: at pre > 0 the zero is
# explained by the inflation and the gradient vanishes.
# The pi head of the zero-inflated kind is probed at t = 1 ON ITS LIVE GENE:
# in the zero branch its gradient u qi - w pi is a difference a third the size
# of its terms, whose rounding alone eats the room for a defect; at t > 0 it
# is -sigmoid(a), exponential at a < 0 like the p head of the negative
# binomial.
LIVE_SIGN = {"poisson": [0], "negative binomial": [-1, 0],
             "zero-inflated negative binomial": [-1, -1, -1]}
LIVE_T1 = {"zero-inflated negative binomial": [1, 0, 0]}
# the head whose FORWARD value is exponential in pre (at pre > 0).  The
# zero-inflated log likelihood at t = 0 is log(pi + ...) >= log(1/2) with the
# other heads at 0, so ITS live gene carries t = 1: ll = log(1 - pi) +
# r log(1 - p) + log p + log r, in which r = e^pre of the log_r head dominates.
FORWARD_HEAD = {"poisson": 0, "negative binomial": 1,
                "zero-inflated negative binomial": 2}
# adds of the row sum from the one that brings the live gene in, the most any
# forward kernel has inside a workgroup: decoder_forward_kernel's lane sums 32
# elements (31), the sparse correction (1) and one cross-lane add (1); the
# head kernels a lane's <= 16 elements and <= 16 parts.  Then one per strip.
LL_ADDS = 34
FORWARD_PRE = (8.0, 9.5)            # |pre| of a forward-only probe


def gemm1_probe(name, rows, H, F, seed, arith="bf16x9", forward=False):
    """pre = d W through the exponential (module docstring).  Checked in a
    training launch: dd[r, h(r)] for every row, dW_J[h, f(h)] for every live
    column (a sum over the rows that share it); in a forward-only launch
    ll[r] for every row."""
    P = HEADS[name]
    rng = np.random.default_rng([1, seed, H, rows, P, int(forward)])
    hr = (np.arange(rows) + seed * rows) % H if H > rows else \
        (np.arange(rows) + 7 * seed) % H                    # h(r)
    ms = mid_sign_of(seed)
    plo, phi = FORWARD_PRE if forward else (6.0, 9.5)
    if forward:
        J = np.full(H, FORWARD_HEAD[name])
        sign = np.ones(H)
    else:
        J = (np.arange(H) + seed) % P
        sign = np.asarray(LIVE_SIGN[name], dtype=np.float64)[J]
        sign = np.where(sign == 0, rng.choice([-1.0, 1.0], H), sign)
    gene = rng.permutation(F)[:H]                           # f(h)
    # |w| in [1, 1.15] 2^k, |d| in [6 / |w|, 9.5 / |w|]: the product's sign by
    # the sign of d
    w = operands((H,), rng, 1.0, 1.15, MID1, LOW1, ms) \
        * np.float32(2.0) ** rng.integers(-2, 3, H)
    aw = np.abs(_f64(w))[hr]
    dl = operands((rows,), rng, (plo + 0.02) / aw, (phi - 0.02) / aw, MID1, LOW1, ms)
    dl = (np.abs(dl) * (sign[hr] * np.sign(_f64(w))[hr])).astype(np.float32)
    check_operands(dl, MID1, LOW1, ms)
    check_operands(w, MID1, LOW1, ms)
    d = np.zeros((rows, H), dtype=np.float32)
    d[np.arange(rows), hr] = dl
    W = [np.zeros((H, F), dtype=np.float32) for _ in range(P)]
    for h in range(H):
        W[J[h]][h, gene[h]] = w[h]
    gw = operands((rows,), rng, mid_sign=ms)
    a = _f64(dl) * _f64(w)[hr]                              # pre, exact
    assert (np.abs(a) >= plo).all() and (np.abs(a) <= phi).all()
    assert (np.sign(a) == sign[hr]).all()
    Jr = J[hr]
    # t on the live gene of each row
    if forward:
        tl = np.full(rows, 1.0 if P == 3 else 0.0)
    else:
        tl = np.asarray(LIVE_T1.get(name, [0] * P), dtype=np.float64)[Jr]
    t = np.zeros((rows, F), dtype=np.float32)
    t[np.arange(rows), gene[hr]] = tl
    B = product_bound(arith)
    zero = np.zeros(rows)
    pre_v = [np.where(Jr == j, a, 0.0) for j in range(P)]
    # the likelihood's own error at the exact pre (running bound), and what
    # the product's relative error B does to g and lp: the oracle at
    # pre (1 +- B), both monotone in pre over that width
    lp, g = lik_live(name, [(v, zero) for v in pre_v], tl)
    lp64, g64 = oracle_t0(name, pre_v, tl)
    pick = lambda per_head: np.choose(Jr, [np.asarray(x) for x in per_head])
    gv, ge = pick([x[0] for x in g]), pick([x[1] for x in g])
    gx = pick(g64)
    assert np.allclose(gv, gx, rtol=1e-9, atol=0) and np.allclose(lp[0], lp64, rtol=1e-9)
    moved = [oracle_t0(name, [v * s for v in pre_v], tl) for s in (1.0 + B, 1.0 - B)]
    ge = ge + np.maximum(*[np.abs(pick(m[1]) - gx) for m in moved])
    lp = (lp[0], lp[1] + np.maximum(*[np.abs(m[0] - lp64) for m in moved]))
    second = 1.0 + 2.0 ** -10
    # G = fl(gw g): the error of g and one rounding
    G = _f64(gw) * gx
    eG = (np.abs(_f64(gw)) * ge + U * np.abs(G)) * second
    probe = {"name": name, "probe": "gemm1", "rows": rows, "H": H, "F": F,
             "P": P, "seed": seed, "d": d, "gw": gw, "W": W,
             "t": t, "tl": tl,
             "b": [np.zeros(F, dtype=np.float32) for _ in range(P)],
             "zeros": [], "hr": hr, "J": J, "gene": gene, "pre": a,
             "forward": forward,
             # columns without a live row (H > rows): their rows of dW are 0
             "dead_cols": np.setdiff1d(np.arange(H), hr)}
    if forward:
        # ll[r] = lp(live gene) + (F - 1) lp(0): each with its own error, and
        # the adds from the one that brings the live gene in: LL_ADDS inside
        # the workgroup, then one per strip (the other adds of ll_reduce_kernel
        # add exact zeros), each at most u of the row's sum of sizes
        lp0, _ = lik_dense_t0(name, [(zero, zero)] * P)
        lp0_64, _ = oracle_t0(name, [zero] * P)
        exact = lp64 + (F - 1) * lp0_64
        size = np.abs(lp64) + (F - 1) * np.abs(lp0_64)
        strips = (F + 31) // 32 - 1          # (the narrowest strip any kernel has)
        bound = (lp[1] + (F - 1) * lp0[1]) * second + (LL_ADDS + strips) * U * size
        probe["checks"] = [{"out": "ll", "exact": exact, "bound": bound,
                            "pre": a, "head": Jr, "x": dl, "y": w[hr],
                            "rest": (F - 1) * lp0_64}]
        return _finish(probe)
    wl = _f64(w)[hr]
    dd = G * wl
    checks = [{"out": "dd_live", "rows": np.arange(rows), "cols": hr,
               "exact": dd, "bound": np.abs(wl) * eG + B * np.abs(dd),
               "pre": a, "head": Jr, "x": dl, "y": w[hr]}]
    # dW_J[h, f(h)] = sum over the rows of column h of d[r, h] G[r, f(h)]:
    # every term's own bound, and n_h - 1 adds of at most u of the sizes
    term = _f64(dl) * G
    eterm = np.abs(_f64(dl)) * eG + B * np.abs(term)
    n_h = np.bincount(hr, minlength=H)
    lives = np.flatnonzero(n_h)
    tot = np.bincount(hr, weights=term, minlength=H)[lives]
    size = np.bincount(hr, weights=np.abs(term), minlength=H)[lives]
    bnd = np.bincount(hr, weights=eterm, minlength=H)[lives] + n_h[lives] * U * size
    checks.append({"out": "dW_live", "heads": J[lives], "rows": lives,
                   "cols": gene[lives], "exact": tot, "bound": bnd})
    probe["checks"] = checks
    return _finish(probe)
