"""The evaluation statistics -- ``px_statistics_kernel``,
``px_statistics_cat_kernel``, ``sqrt_sum_kernel``, ``loglik_elementwise_kernel``
and the device functions ``lik_mean_var`` / ``cat_mean_var`` -- element by
element against ``tests/_px_oracle.py`` (fp64, stable forms, pinned on the host
by ``tests/test_px_oracle_host.py``).

Inputs: every combination of the heads' edge values (``_px_oracle.cycle``: the
sigmoid heads from -95 to 40, both sides of logit(tiny) and the p -> 1 region;
the log heads at -11, -10, -9.99, 0, 9.99, 10, 11), the samples of an element a
few hundredths apart; for the categorised distribution a flat row of logits and
class 0, a middle class and the tail class raised by 5, 20 and 40, for 1, 3 and
64 classes, through an evaluation step of the engine.

Asserted per element, with the counts ``c`` that ``_px_oracle`` derives from
the kernel's chain of operations (nothing below was chosen from the device's
output; u = 2^-24, every count allowed twice):

* mean:                 |got - want| <= c u |want|
* mean of variances:    |got - want| <= c u var + 2 c u |mean| sqrt(var)
                                        + (c u mean)^2
* variance of means:    S > 1 (or a weight): the same shape on
                        mean_s (m_s - pm)^2; S = 1: <= 1e-12 m^2
* an accumulating call adds one rounding of the sum it leaves behind
* every variance >= 0, nothing NaN; above the fp32 maximum (negative-binomial
  logit 40 with log r from 9.99 up: 3 of the 98 combinations of its two heads)
  the output is +inf.  Those elements alone are excused, and they are fewer
  than 2 % of a case's elements: a case runs all six kinds, 3.06 % of the
  negative binomial's and 2.4 % of the zero-inflated negative binomial's
  elements, none of the others' (computed on the host when the cases were
  written: 0.6 % of a case at most)
* pi logit <= -88: the zero-inflated statistics ARE the plain distribution's,
  bit for bit
* 2^-126, the smallest normal fp32, is the only absolute term.

Worst error / bound measured on an MI355X (every test prints its own):

    scvae_pxmean_stats, over the 120 cases  mean   mean of var  var of mean
      poisson                               0.333  0.333        0.277
      negative binomial                     1.000  0.999        0.295
      zero-inflated poisson                 0.333  0.333        0.332
      zero-inflated negative binomial       0.998  0.998        0.333
      constrained poisson                   0.361  0.333        0.252
      bernoulli                             0.997  0.997        0.321
    scvae_likelihood_elementwise            mean   variance
      poisson / zero-inflated poisson       0.278 / 0.134   0.177 / 0.134
      negative binomial / zero-inflated     0.998 / 0.999   0.998 / 0.999
      bernoulli                             0.999           0.999
    categorised (12 cases)     p_x_mean <= 0.156, p_x_stddev <= 0.126,
                               stddev of the mean <= 0.076 (1.000 where the
                               value is below its bound and the device holds
                               0), decode <= 0.172

The ratios next to 1 are values below 2^-126 that the fast exponential
returns as zero, measured against that floor (exp(-87.4) = 1.1e-38 against
1.18e-38); away from the floor nothing is above 0.37.  Above the fp32
maximum: at most 0.59 % of a case's elements.

Against the parent commit's library the same file fails 130 of its 133
tests: the statistics entry refuses the constrained-Poisson kind; the
zero-inflated statistics are not the plain distribution's where pi -> 0 and
the zero-inflated negative binomial's variance is NaN (inf - inf) where its
mean^2 overflows; the Bernoulli variance p (1 - p) and the zero-inflated
Poisson's are outside the bound; the negative-binomial mean r exp(a) is zero
at the lower clip; p_x_stddev of the categorised models is NaN or outside
the bound in 9 of 12 cases.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import likelihoods as lk
from oracle import models as om

import _px_oracle as px

pytestmark = pytest.mark.gpu

KINDS = list(px.HEADS)
#: an accumulating call starts from these (one per output: a swap would show)
PREFILL = (0.75, 1.5, 0.375)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)


def _host(t):
    return t.detach().cpu().double().numpy()


def _hold(got, want, bound, what, floor=0.0, peak=None):
    """Every element within its bound, or +inf where the fp64 value (or, at the
    edge, the value and its bound) is above the fp32 maximum -- the value
    itself or ``peak``, the sum over the samples it is the mean of.  Returns
    the worst error / bound and the number of elements excused as overflow."""
    assert not np.isnan(got).any(), what + ": NaN"
    assert (got >= floor).all(), what + ": below {}".format(floor)
    over = np.maximum(want, want if peak is None else peak) > px.FLOAT32_MAX
    assert (got[over] == np.inf).all(), what + ": finite above the fp32 maximum"
    edge = ~over & (want + bound > px.FLOAT32_MAX) & (got == np.inf)
    inside = ~over & ~edge
    assert np.isfinite(got[inside]).all(), what + ": not finite"
    ratio = np.abs(got[inside] - want[inside]) / bound[inside]
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1:
        i = np.flatnonzero(inside.reshape(-1))[ratio.argmax()]
        raise AssertionError(
            "{}: element {} got {!r} want {!r}, error / bound {:.3g}".format(
                what, np.unravel_index(i, got.shape), got.reshape(-1)[i],
                want.reshape(-1)[i], worst))
    return worst, int(over.sum() + edge.sum())


@functools.lru_cache(maxsize=None)
def _reference(name, S, B, F, weighted):
    """pre-activations, the weight, the fp64 statistics and their bounds."""
    pre = px.cycle(name, S, B, F, offset=37 * (S + B))
    weight = None
    if weighted:
        weight = np.random.default_rng(B).random(B).astype(np.float32)
    mean, var, cm, cv = px.mean_variance(name, pre)
    shape = (S, B, F)
    mean, var = mean.reshape(shape), var.reshape(shape)
    cm, cv = np.reshape(cm, shape), np.reshape(cv, shape)
    want = px.statistics(mean, var, weight)
    bounds = px.statistics_bounds(mean, var, cm, cv, weight)
    peak = px.peaks(mean, var, weight)
    for a in pre + list(want) + list(bounds) + list(peak):
        a.setflags(write=False)
    return pre, weight, mean, want, bounds, peak


def _launch(lib, kind, pre, S, B, F, weight, ldw, accumulate, device):
    from scvae_amd import _lib
    pred = [_dev(a, device) for a in pre]
    arr = (ctypes.c_void_p * len(pred))(*[t.data_ptr() for t in pred])
    wd = None
    if weight is not None:      # [B] with stride ldw, NaN in the gaps
        wd = torch.full((B, ldw), float("nan"), device=device)
        wd[:, 0] = _dev(weight, device)
    outs = [torch.full((B, F), v if accumulate else float("nan"), device=device)
            for v in PREFILL]
    _lib.check(lib.scvae_pxmean_stats(
        kind, arr, S, B, F, _p(wd), ldw if wd is not None else 0, accumulate,
        _p(outs[0]), _p(outs[1]), _p(outs[2]), _stream()), "pxmean_stats")
    torch.cuda.synchronize()
    return [_host(t) for t in outs]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("weight", ["none", "ldw1", "ldw4"])
@pytest.mark.parametrize("F", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("S", [1, 3])
def test_pxmean_stats_per_element(cuda_device, S, B, F, weight, accumulate):
    from scvae_amd import _lib
    lib = _lib.load()
    ldw = {"none": 0, "ldw1": 1, "ldw4": 4}[weight]
    worst, failed = {}, []
    excused = elements = 0
    for name in KINDS:
        kind = _lib.LIKELIHOOD_KINDS[name][0]
        pre, w, mean, want, bounds, peak = _reference(name, S, B, F, ldw > 0)
        try:
            got = _launch(lib, kind, pre, S, B, F, w, ldw, accumulate,
                          cuda_device)
        except _lib.HipLibraryError as error:
            failed.append("{}: {}".format(name, error))
            continue
        for i, what in enumerate(("mean", "mean of var", "var of mean")):
            fill = PREFILL[i] if accumulate else 0.0
            total = want[i] + fill
            # (the accumulating sum: one rounding of what it leaves, twice)
            bound = bounds[i] + (2 * px.U * np.abs(total) if accumulate else 0)
            try:
                if i == 2 and S == 1 and w is None:
                    # one sample: zero up to the rounding of (m - 1.0 * m)
                    assert (got[i] - fill
                            <= 1e-12 * (mean[0] ** 2 + 1e-30)).all(), name
                    assert (got[i] >= fill).all(), name
                    continue
                ratio, n = _hold(got[i], total, bound,
                                 "{} {}".format(name, what), fill, peak[i])
            except AssertionError as error:     # (every kind gets its say)
                failed.append(str(error))
                continue
            worst[name, what] = ratio
            excused += n
            elements += got[i].size
        if name.startswith("zero-inflated"):
            # pi -> 0: the plain distribution's statistics, bit for bit
            base = name[len("zero-inflated "):]
            plain = _launch(lib, _lib.LIKELIHOOD_KINDS[base][0], pre[1:], S, B,
                            F, w, ldw, accumulate, cuda_device)
            off = (pre[0].reshape(S, B, F) <= -88.0).all(axis=0)
            assert off.any() or B * F < 14
            for a, b in zip(got, plain):
                if not (a[off] == b[off]).all():
                    failed.append(name + ": not the plain distribution's "
                                  "where pi -> 0")
                    break
    print("px_statistics S={} B={} F={} {} acc={}: worst error / bound {}; "
          "{} of {} elements above the fp32 maximum".format(
              S, B, F, weight, accumulate,
              {k: round(v, 3) for k, v in worst.items()}, excused, elements))
    assert not failed, "\n".join(failed)
    assert excused < 0.02 * elements


def test_likelihood_elementwise_mean_and_variance(cuda_device):
    """``.mean()`` / ``.variance()`` of the DISTRIBUTIONS classes: the same
    device function behind ``loglik_elementwise_kernel`` (grid-stride loop:
    more elements than one block, not a multiple of it), on the same inputs."""
    from scvae_amd import _lib
    lib = _lib.load()
    B, F = 5, 600
    n = B * F
    failed = []
    excused = elements = 0
    for name in KINDS:
        if name == "constrained poisson":     # (no class of the registry)
            continue
        kind = _lib.LIKELIHOOD_KINDS[name][0]
        pre = _reference(name, 1, B, F, False)[0]
        pred = [_dev(a, cuda_device) for a in pre]
        arr = (ctypes.c_void_p * len(pred))(*[t.data_ptr() for t in pred])
        mean = torch.full((n,), float("nan"), device=cuda_device)
        var = torch.full((n,), float("nan"), device=cuda_device)
        _lib.check(lib.scvae_likelihood_elementwise(
            kind, None, arr, None, _p(mean), _p(var), n, _stream()),
            "likelihood_elementwise")
        torch.cuda.synchronize()
        wm, wv, cm, cv = px.mean_variance(name, pre)
        wm, wv = wm.reshape(-1), wv.reshape(-1)
        cm, cv = np.reshape(cm, -1), np.reshape(cv, -1)
        try:
            r_mean, _ = _hold(_host(mean), wm, px.mean_bound(wm, cm),
                              name + " mean")
            r_var, over = _hold(_host(var), wv,
                                px.variance_bound(wv, wm, np.maximum(cm, cv)),
                                name + " variance")
        except AssertionError as error:
            failed.append(str(error))
            continue
        print("likelihood_elementwise {}: worst error / bound mean {:.3f} "
              "variance {:.3f}; {} of {} above the fp32 maximum".format(
                  name, r_mean, r_var, over, n))
        excused += over
        elements += 2 * n
    assert not failed, "\n".join(failed)
    assert excused < 0.02 * elements


# ---- the categorised kernel: through an evaluation step of the engine ----
# F genes: the block edge of the 256-wide grid; 13 turns of the 20 rows of logits
CAT_F, CAT_L, CAT_H, CAT_B, CAT_K = 257, 4, (12, 10), 5, 2


def _scope(model_type):
    return "X/DISTRIBUTION/" if model_type == "GMVAE" else "X_TILDE/"


def _set_parameters(named, model_type, likelihood, k_max):
    """Head and logit biases per gene, head weights of 0.002 (the method of
    ``_engine_step_case`` in test_gpu_head_edges.py): gene f takes row f % 20
    of ``logit_rows`` and, of head j, value (f (1 + 4 j) + f // 20) of its
    list -- another combination under every turn of the rows."""
    scope = _scope(model_type)
    heads = lk.LIKELIHOOD_PARAMETERS[likelihood]
    g = torch.Generator().manual_seed(3)
    f = np.arange(CAT_F)
    rows = px.logit_rows(k_max)
    for name, p in named.items():
        if name.startswith(scope) and name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.002)
        elif name.startswith(scope + "P_K") and name.endswith("biases"):
            p.copy_(torch.from_numpy(rows[f % len(rows)].reshape(-1)))
        elif name.startswith(scope) and name.endswith("biases"):
            head = name[len(scope):].split("/")[0].lower()
            values = np.asarray(px.HEAD_PRE[head], dtype=np.float32)
            j = heads.index(head)
            p.copy_(torch.from_numpy(
                values[(f * (1 + 4 * j) + f // 20) % len(values)]))
        elif not name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)


class _Recorded:
    """The oracle's ``dense_layer`` with the outputs of the decoder
    distribution's layers recorded: (pre-activation, sum_h |d_h| |W_h|)."""

    def __init__(self, scope):
        self.scope, self.seen, self.real = scope, [], om.dense_layer

    def __call__(self, x, params, scope, *args, **kwargs):
        out = self.real(x, params, scope, *args, **kwargs)
        if scope.startswith(self.scope):
            w = params[scope + "/DENSE/weights"]
            self.seen.append((out.detach().numpy(),
                              (x.abs() @ w.abs()).detach().numpy()))
        return out

    def run(self, fn):
        om.dense_layer = self
        try:
            return fn()
        finally:
            om.dense_layer = self.real

    def inputs(self, block, rows, k_max):
        """fp32-held pre-activations and how far off the device's may be:
        each is the fp32 sum of its bias and a product of about 0.01 with the
        last hidden layer, which the device holds to 1e-5 of its scale at
        worst:  delta = 2 u |a| + 1e-5 sum_h |d_h W_h|."""
        arrays = [a.astype(np.float32).astype(np.float64) for a, _ in block]
        deltas = [2 * px.U * np.abs(a) + 1e-5 * s for a, s in block]
        arrays[-1] = arrays[-1].reshape(rows, CAT_F, k_max + 1)
        deltas[-1] = deltas[-1].reshape(rows, CAT_F, k_max + 1)
        return arrays, deltas


def _reach(fn, arrays, deltas):
    """sum_j |fn(a + delta_j e_j) - fn(a)| over every head and every class, per
    output of ``fn``: the first-order reach of the input errors."""
    base = fn(arrays)
    reach = [np.zeros_like(b) for b in base]
    for j, delta in enumerate(deltas):
        classes = arrays[j].shape[-1] if arrays[j].ndim == 3 else 1
        for c in range(classes):
            moved = list(arrays)
            moved[j] = arrays[j].copy()
            if arrays[j].ndim == 3:
                moved[j][..., c] += delta[..., c]
            else:
                moved[j] += delta
            for r, a, b in zip(reach, fn(moved), base):
                r += np.abs(a - b)
    return reach


def _categorised_reference(model_type, likelihood, S, k_max, params, moving,
                           x, eps):
    """(p_x_mean, mean of variances, variance of means) of an evaluation step
    in fp64 stable forms on the oracle forward's pre-activations, the bounds
    (the statistics' own + twice the reach of the input errors + the
    accumulating sums over the clusters), the largest intermediate."""
    gm = model_type == "GMVAE"
    P = len(lk.LIKELIHOOD_PARAMETERS[likelihood])
    cfg = om.ModelConfig(feature_size=CAT_F, latent_size=CAT_L,
                         hidden_sizes=CAT_H, likelihood=likelihood,
                         n_clusters=CAT_K, n_iw=S, n_mc=1, k_max=k_max)
    rec = _Recorded(_scope(model_type))
    forward = om.gmvae_forward if gm else om.vae_forward
    full = rec.run(lambda: forward(cfg, params, moving, x, x, eps, False,
                                   evaluation_statistics=True))
    passes = CAT_K if gm else 1
    assert len(rec.seen) == passes * (P + 1)
    shape = (S, CAT_B, CAT_F)
    want = [0.0, 0.0, 0.0]
    bound = [0.0, 0.0, 0.0]
    peak = [0.0, 0.0, 0.0]
    for k in range(passes):
        arrays, deltas = rec.inputs(rec.seen[k * (P + 1):(k + 1) * (P + 1)],
                                    S * CAT_B, k_max)
        weight = full["y"].numpy()[:, k] if gm else None

        def elements(a):
            return px.categorised_mean_variance(likelihood, a[:P], a[P], k_max)

        def three(a):
            m, v, _, _ = elements(a)
            return px.statistics(m.reshape(shape), v.reshape(shape), weight)

        m, v, cm, cv = (np.reshape(a, shape) for a in elements(arrays))
        # the case reaches the regime where the raw-moment form has no bits
        # left (one class of Poisson counts cannot: its variance is >= e^-10)
        assert (v < px.U * m * m).any() or (k_max, likelihood) == (1, "poisson")
        reach = _reach(three, arrays, deltas)
        for i, (part, limit, top) in enumerate(zip(
                px.statistics(m, v, weight),
                px.statistics_bounds(m, v, cm, cv, weight),
                px.peaks(m, v, weight))):
            want[i] = want[i] + part
            bound[i] = bound[i] + limit + 2 * reach[i]
            peak[i] = np.maximum(peak[i], top)
    if gm:      # one rounding of every partial sum over the clusters, twice
        bound = [b + 2 * CAT_K * px.U * np.abs(w) for b, w in zip(bound, want)]
    # (the bookkeeping: the oracle's own mean, of the unrounded inputs)
    assert np.allclose(want[0], full["p_x_mean"].numpy(), rtol=1e-4)
    return cfg, want, bound, peak


def _interval(got, want_var, bound, peak, what):
    """A standard deviation against the root of a variance held to ``bound``:
    sqrt(max(v - b, 0)) (1 - 2u) <= got <= sqrt(v + b) (1 + 2u); +inf where
    the variance (or the sum it was made of) is above the fp32 maximum."""
    assert not np.isnan(got).any(), what + ": NaN"
    assert (got >= 0).all(), what + ": negative"
    over = np.maximum(want_var, peak) > px.FLOAT32_MAX
    assert (got[over] == np.inf).all(), what + ": finite above the fp32 maximum"
    edge = ~over & (want_var + bound > px.FLOAT32_MAX) & (got == np.inf)
    inside = ~over & ~edge
    assert np.isfinite(got[inside]).all(), what + ": not finite"
    low = np.sqrt(np.maximum(want_var - bound, 0)) * (1 - 2 * px.U)
    high = np.sqrt(want_var + bound) * (1 + 2 * px.U)
    centre = np.sqrt(want_var)
    ratio = np.where(got >= centre,
                     (got - centre) / np.maximum(high - centre, 1e-300),
                     (centre - got) / np.maximum(centre - low, 1e-300))
    ratio = np.where((got == centre) | ~inside, 0.0, ratio)
    worst = float(ratio.max())
    i = np.unravel_index(ratio.argmax(), ratio.shape)
    assert worst <= 1, "{}: element {} got {!r} want {!r} error / bound {:.3g}" \
        .format(what, i, got[i], centre[i], worst)
    return worst, int(over.sum() + edge.sum())


def _hold_categorised(outs, S, gm, want, bound, peak):
    """the three outputs of the step against the reference; the ratios."""
    pm, mov, vom = want
    r_mean, _ = _hold(outs["p_x_mean"], pm, bound[0], "p_x_mean")
    if S == 1 and not gm:
        sd = outs["stddev_of_p_x_given_z_mean"]
        assert (sd ** 2 <= 1e-12 * (pm ** 2 + 1e-30)).all()
        r_sd = 0.0
    else:
        r_sd, _ = _interval(outs["stddev_of_p_x_given_z_mean"], vom, bound[2],
                            peak[2], "stddev_of_p_x_given_z_mean")
    r_total, over = _interval(outs["p_x_stddev"], vom + mov,
                              bound[1] + bound[2],
                              np.maximum(peak[1], peak[2]), "p_x_stddev")
    assert over < 0.02 * pm.size
    return r_mean, r_sd, r_total, over


CAT_CASES = [("VAE", "negative binomial", 1), ("VAE", "poisson", 3),
             ("GMVAE", "negative binomial", 3), ("GMVAE", "poisson", 1)]


@pytest.mark.parametrize("k_max", [1, 3, 64])
@pytest.mark.parametrize("model_type,likelihood,S", CAT_CASES)
def test_categorised_statistics_per_element(cuda_device, model_type,
                                            likelihood, S, k_max):
    """``px_statistics_cat_kernel`` + ``sqrt_sum_kernel``: the three outputs of
    an evaluation step, and ``decode``, on an engine whose head and logit
    biases put every gene at an edge (``_set_parameters``), against the helper
    on the pre-activations of the fp64 oracle forward.  Those are not the
    device's to the last bit; ``_Recorded.inputs`` says how far off they may
    be, and every bound gains the first-order reach of that through the fp64
    helper, one head and one class at a time, allowed twice."""
    from scvae_amd.engine import Engine
    gm = model_type == "GMVAE"
    eng = Engine(CAT_F, CAT_L, CAT_H, likelihood, batch_norm=True,
                 model_type=model_type, n_clusters=CAT_K, device=cuda_device,
                 seed=2, k_max=k_max)
    _set_parameters(eng.named_parameters(), model_type, likelihood, k_max)
    params = {k: v.detach().cpu().double()
              for k, v in eng.named_parameters().items()}
    moving = {k: v.detach().cpu().double()
              for k, v in eng.named_moving_statistics().items()}
    rng = np.random.default_rng(3)
    x = torch.from_numpy((rng.poisson(2.5, (CAT_B, CAT_F))
                          * (rng.random((CAT_B, CAT_F)) > 0.4)).astype(
                              np.float64))
    eps = torch.from_numpy(rng.standard_normal(
        (CAT_K, S, CAT_B, CAT_L) if gm else (S, CAT_B, CAT_L)))
    xd, epsd = x.float().to(cuda_device), eps.float().to(cuda_device)
    outs = {k: torch.full((CAT_B, CAT_F), float("nan"), device=cuda_device)
            for k in ("p_x_mean", "p_x_stddev", "stddev_of_p_x_given_z_mean")}
    eng.step(xd, xd, eps=epsd, training=False, n_iw=S, n_mc=1, outputs=outs)
    torch.cuda.synchronize()
    cfg, want, bound, peak = _categorised_reference(
        model_type, likelihood, S, k_max, params, moving, x, eps)
    ratios = _hold_categorised({k: _host(v) for k, v in outs.items()}, S, gm,
                               want, bound, peak)
    print("categorised {} {} S={} k={}: worst error / bound p_x_mean {:.3f} "
          "stddev of mean {:.3f} p_x_stddev {:.3f}; {} of {} above the fp32 "
          "maximum".format(model_type, likelihood, S, k_max, *ratios,
                           CAT_B * CAT_F))

    # decoder-only entry on the same engine: the mean alone
    P = len(lk.LIKELIHOOD_PARAMETERS[likelihood])
    z = torch.from_numpy(rng.standard_normal((7, CAT_L)))
    rec = _Recorded(_scope(model_type))
    rec.run(lambda: om.decode_mean(cfg, params, moving, z, model_type))
    arrays, deltas = rec.inputs(rec.seen, 7, k_max)

    def mean_of(a):
        return px.categorised_mean_variance(likelihood, a[:P], a[P], k_max)

    mean, _, cm, _ = mean_of(arrays)
    reach = _reach(lambda a: mean_of(a)[:1], arrays, deltas)
    got = _host(eng.decode(z.float().to(cuda_device)))
    r_dec, _ = _hold(got, mean, px.mean_bound(mean, cm) + 2 * reach[0],
                     "decode")
    print("categorised decode: worst error / bound {:.3f}".format(r_dec))
