"""fp64 restatement of the GMVAE mixture stage (scvae_amd/csrc/gmvae_kernels.hip)
entry by entry, with the error a correct fp32 evaluation of the same
formulation may carry, and a plain NumPy fp32 evaluation of each entry in the
kernel's order of operations.

Every oracle takes the fp32-ROUNDED inputs the device holds (as
``test_batch_norm_stats_under_cancellation`` does) and returns ``Held`` triples
per output: ``value`` (fp64), ``mag`` (the sum of the magnitudes of the terms the
element is summed from) and ``bound`` (the derived bound on |got - value|, the
total ALREADY allowed twice).  ``hold`` is the one assert both the GPU test
(tests/test_gpu_mixture_stage.py) and the host test
(tests/test_mixture_oracle_host.py, on the fp32 evaluation) go through.

The roundings, with u = 2^-24 (one rounding to nearest):
  + - * / sqrt     u each (fp32 division and square root are correctly rounded
                   in this build: no fast-math flag in csrc/build.sh)
  log              v_log_f32, 1 ulp = 2 u of log2 x, times ln 2 (u):  3 u |log x|
  exp              v_exp_f32, 1 ulp = 2 u, of the argument x log2(e) rounded to
                   fp32 with a rounded constant (2 u |x log2 e| absolute in the
                   exponent = 2 u |x| relative in the value):  (2 |x| + 2) u,
                   and 0 for a value below FLT_MIN (likelihood.hpp: "the fast
                   exponential returns 0 below it"): FLT_MIN absolute
  rcp              v_rcp_f32, 1 ulp = 2 u
  a sum of n terms at most (n - 1) u sum |terms| for a serial loop; for one wave
                   strided over K, ceil(K/64) - 1 additions per lane and 6
                   butterfly steps; block_sum<256> adds 4 more
"""
import collections
import math

import numpy as np
import torch

from oracle import models as om
from _parity import close_elementwise

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
BIG = om.FLOAT32_MAX_HALF
F32 = np.float32

Held = collections.namedtuple("Held", "value mag bound")


ROUND_INPUTS = True       # (the host test pins the fp64 forms to om with it off)


def r32(a):
    """The fp64 value of the fp32 rounding of ``a``."""
    if not ROUND_INPUTS:
        return np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def hold(what, got, held, mask=None, report=None):
    """|got - value| <= bound for every element (of ``mask``); prints and
    records the largest err / bound."""
    if hasattr(got, "detach"):
        got = got.detach().cpu().numpy()
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(held.value))
    want = np.asarray(held.value, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(held.bound, dtype=np.float64), want.shape)
    if mask is None:
        mask = np.ones(want.shape, dtype=bool)
    mask = np.broadcast_to(mask, want.shape)
    assert np.isfinite(want[mask]).all() and np.isfinite(bound[mask]).all(), what
    assert np.isfinite(got[mask]).all(), "{}: non-finite output".format(what)
    with np.errstate(invalid="ignore"):      # (inf - inf outside the mask)
        err = np.abs(got - want)[mask]
    # (an element whose bound is 0 has to be exact)
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound[mask], 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("{}: max err / bound {:.3f} over {} elements".format(what, worst, ratio.size))
    if report is not None:
        key = what.split(" [")[0]
        report[key] = max(report.get(key, 0.0), worst)
    if worst > 1.0:
        flat = int(np.argmax(ratio))
        idx = tuple(int(v[flat]) for v in np.nonzero(mask)) if want.ndim else ()
        what = ("{}: element {} got {!r} want {!r} (|diff| {:.3e} > bound {:.3e}); "
                "err / bound").format(what, idx, got[idx], want[idx],
                                      abs(got[idx] - want[idx]), bound[idx])
    # |got - want| <= bound, element by element (rtol = 0; the bound is the atol)
    close_elementwise(ratio, np.zeros_like(ratio), rtol=0.0, atol=1.0, what=what)
    return worst


# --------------------------------------------------------------------------
# fp32 arithmetic of the kernels, in NumPy
# --------------------------------------------------------------------------
_LOG2E = F32(1.4426950408889634)
_LN2 = F32(0.6931471805599453)


def exp32(x):
    """__expf: v_exp_f32 of the fp32 product x log2(e); 0 below FLT_MIN."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", under="ignore"):
        r = np.exp2((x * _LOG2E).astype(np.float64)).astype(F32)
    return np.where(r < F32(FLT_MIN), F32(0), r).astype(F32)


def log32(x):
    x = np.asarray(x, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.log2(x.astype(np.float64)).astype(F32) * _LN2).astype(F32)


def log1p32(x):     # common.hpp fast_log1p
    x = np.asarray(x, dtype=F32)
    u = F32(1) + x
    d = u - F32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = log32(u) * (x * (F32(1) / d))
    return np.where(d == 0, x, v).astype(F32)


def softplus32(a):
    a = np.asarray(a, dtype=F32)
    return (np.maximum(a, F32(0)) + log1p32(exp32(-np.abs(a)))).astype(F32)


def sigmoid32(a):
    a = np.asarray(a, dtype=F32)
    e = exp32(-np.abs(a))
    s = F32(1) / (F32(1) + e)
    return np.where(a >= 0, s, e * s).astype(F32)


def clip32(a):
    return np.clip(np.asarray(a, dtype=F32), F32(-BIG), F32(BIG))


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


# --------------------------------------------------------------------------
# log-softmax with its error terms
# --------------------------------------------------------------------------
def wave_roundings(K):
    """Additions a value passes through in a wave-wide sum strided over K."""
    return (K + 63) // 64 - 1 + 6


def _log_softmax(m, n_sum):
    """``m`` [..., K] fp64.  lse = mx + log(sum exp(m - mx)) as the kernels form
    it, and per element the log-probability ly = m - lse and p = exp(ly):
      d = m - mx         u |d|
      e = exp(d)         relative (2 |d| + 2) u + u |d| (its argument's rounding)
      se = sum e         relative E = sum e (3 |d| + 2) u / se + n_sum u
      log(se)            absolute 3 u log(se) + E
      lse = mx + log se  u |lse|: THE u * max|logit| term every ly inherits
        A_lse = E + u (3 log se + |lse|)
      ly = m - lse       A_ly = A_lse + u |ly|
      p = exp(ly)        relative R_p = A_ly + (2 |ly| + 2) u, FLT_MIN absolute"""
    mx = m.max(axis=-1, keepdims=True)
    d = m - mx
    e = np.exp(d)
    se = e.sum(axis=-1, keepdims=True)
    lse = mx + np.log(se)
    E = U * ((e * (3 * np.abs(d) + 2)).sum(axis=-1, keepdims=True) / se + n_sum)
    A_lse = E + U * (3 * np.log(se) + np.abs(lse))
    ly = m - lse
    A_ly = A_lse + U * np.abs(ly)
    R_p = A_ly + U * (2 * np.abs(ly) + 2)
    return dict(lse=lse, ly=ly, p=np.exp(ly), A_lse=A_lse, A_ly=A_ly, R_p=R_p,
                max_logit=np.abs(m).max(axis=-1))


def categorical_fwd(logits, prior=None):
    """scvae_categorical_entropy_kl_fwd: y [B, K], kl_y_cell [B].
      y   = p:  p R_p + FLT_MIN
      KL  = sum_k p_k rel_k (+ log K for the uniform prior, rel = ly), with
            rel = ly - (prior - lse_p):   A_rel = A_ly + A_lp + u |rel|
            a term p rel:   p |rel| (R_p + u) + p A_rel; one flushed to 0: FLT_MIN |rel|
            their sum:      wave_roundings(K) u sum |terms|
            log K - h:      3 u log K + u |KL|"""
    logits = r32(logits)
    K = logits.shape[-1]
    ns = wave_roundings(K)
    q = _log_softmax(logits, ns)
    rel, A_rel = q["ly"], q["A_ly"]
    if prior is not None:
        pr = _log_softmax(r32(prior).reshape(1, K), ns)
        rel = q["ly"] - pr["ly"]
        A_rel = q["A_ly"] + pr["A_ly"] + U * np.abs(rel)
    p = q["p"]
    terms = p * rel
    A_terms = p * np.abs(rel) * (q["R_p"] + U) + p * A_rel + FLT_MIN * np.abs(rel)
    kl = terms.sum(axis=-1)
    mag = np.abs(terms).sum(axis=-1)
    bound = A_terms.sum(axis=-1) + ns * U * mag
    if prior is None:
        kl = math.log(K) + kl
        mag = mag + math.log(K)
        bound = bound + 3 * U * math.log(K)
    bound = bound + U * np.abs(kl)
    info = dict(max_logit=q["max_logit"], abs_log_y=np.abs(q["ly"]), A_lse=q["A_lse"])
    return dict(y=Held(p, p, 2 * (p * q["R_p"] + FLT_MIN)),
                kl=Held(kl, mag, 2 * bound)), info


def sim_categorical_fwd(logits, prior=None):
    x = _f(logits)

    def lse_of(m):
        mx = m.max(axis=-1, keepdims=True)
        se = exp32(m - mx).sum(axis=-1, keepdims=True, dtype=F32)
        return (mx + log32(se)).astype(F32)
    ly = (x - lse_of(x)).astype(F32)
    p = exp32(ly)
    K = x.shape[-1]
    if prior is None:
        h = -(p * ly).sum(axis=-1, dtype=F32)
        kl = log32(F32(K)) - h
    else:
        pl = _f(prior).reshape(1, K)
        kl = (p * (ly - (pl - lse_of(pl)))).sum(axis=-1, dtype=F32)
    return p, kl.astype(F32)


def _entropy_terms(prior, n_sum):
    """H[p] = -sum p lp of softmax(prior), serial over K (gmvae_elbo_finish,
    prior_logits_bwd):  a term p lp: p |lp| (R_p + u) + p A_lp (+ FLT_MIN |lp|)."""
    pr = _log_softmax(r32(prior).reshape(-1), n_sum)
    p, lp = pr["p"], pr["ly"]
    H = -(p * lp).sum()
    A_H = ((p * np.abs(lp) * (pr["R_p"] + U) + p * pr["A_ly"] + FLT_MIN * np.abs(lp)).sum()
           + n_sum * U * np.abs(p * lp).sum())
    return pr, H, A_H


def categorical_bwd(y, dy, gate, c, prior=None):
    """scvae_categorical_entropy_kl_bwd on the y THE DEVICE holds:
      dlogits = y (dy - dot) + cc y (rel + h),  cc = c gate,  dot = sum y dy,
      rel = log y - log p (0 where y == 0),  h = -sum y rel.
    (tests/test_mixture_oracle_host.py pins this closed form to autograd.)
      dot          (wave_roundings + 1) u sum |y dy|   (one product each)
      log y        3 u |log y|
      rel          A_rel = 3 u |log y| + A_lp + u |rel|
      h            A_h = sum y (A_rel + u |rel|) + wave_roundings u sum |y rel|
      y (dy - dot) y (A_dot + 2 u |dy - dot|)
      cc y (rel+h) |cc| y (A_rel + A_h + 4 u |rel + h|)   (cc, the sum, two products)
      their sum    u (|t1| + |t2|)"""
    y, dy = r32(y), r32(dy)
    c = float(r32(c))
    K = y.shape[-1]
    ns = wave_roundings(K)
    with np.errstate(divide="ignore"):
        lq = np.where(y > 0, np.log(np.where(y > 0, y, 1.0)), 0.0)
    A_rel = 3 * U * np.abs(lq)
    rel = lq
    if prior is not None:
        pr = _log_softmax(r32(prior).reshape(1, K), ns)
        rel = lq - pr["ly"]
        A_rel = A_rel + pr["A_ly"] + U * np.abs(rel)
    h = -(y * rel).sum(axis=-1, keepdims=True)
    A_h = ((y * (A_rel + U * np.abs(rel))).sum(axis=-1, keepdims=True)
           + ns * U * np.abs(y * rel).sum(axis=-1, keepdims=True))
    dot = (y * dy).sum(axis=-1, keepdims=True)
    A_dot = (ns + 1) * U * np.abs(y * dy).sum(axis=-1, keepdims=True)
    cc = c * float(gate)
    t1 = y * (dy - dot)
    t2 = cc * y * (rel + h)
    A = (y * (A_dot + 2 * U * np.abs(dy - dot))
         + abs(cc) * y * (A_rel + A_h + 4 * U * np.abs(rel + h))
         + U * (np.abs(t1) + np.abs(t2)))
    mag = y * (np.abs(dy) + np.abs(dot)) + abs(cc) * y * (np.abs(rel) + np.abs(h))
    return Held(t1 + t2, mag, 2 * A)


def sim_categorical_bwd(y, dy, gate, c, prior=None):
    y, dy = _f(y), _f(dy)
    K = y.shape[-1]
    lq = np.where(y > 0, log32(np.where(y > 0, y, F32(1))), F32(0)).astype(F32)
    rel = lq
    if prior is not None:
        pl = _f(prior).reshape(1, K)
        mx = pl.max(axis=-1, keepdims=True)
        lse = mx + log32(exp32(pl - mx).sum(axis=-1, keepdims=True, dtype=F32))
        rel = (lq - (pl - lse)).astype(F32)
    h = -(y * rel).sum(axis=-1, keepdims=True, dtype=F32)
    dot = (y * dy).sum(axis=-1, keepdims=True, dtype=F32)
    cc = F32(c) * F32(gate)
    return (y * (dy - dot) + cc * y * (rel + h)).astype(F32)


def prior_logits_bwd(y, prior, gate, c, off_scale, free_nats):
    """scvae_prior_logits_bwd (one workgroup, the softmax serial over K):
      gate on:  c sum_b (p_j - y_bj): the B differences (u each), ceil(B/256) - 1
                additions per thread and 10 in block_sum, p_j's own error B times,
                the product with c
      gate off: s (-p_j (lp_j + H)), s = off_scale free_nats:
                |s| p_j (R_p |lp + H| + A_lp + A_H + 5 u |lp + H|)"""
    y = r32(y)
    B, K = y.shape
    pr, H, A_H = _entropy_terms(prior, K)
    p, lp = pr["p"], pr["ly"]
    c, s = float(r32(c)), float(r32(off_scale)) * float(r32(free_nats))
    if gate:
        diff = p.reshape(1, K) - y
        acc = diff.sum(axis=0)
        mag = np.abs(diff).sum(axis=0)
        nB = (B + 255) // 256 + 10
        A = abs(c) * ((nB + 1) * U * mag + B * (p * pr["R_p"] + FLT_MIN) + U * np.abs(acc))
        return Held(c * acc, abs(c) * mag, 2 * A)
    v = s * (-p * (lp + H))
    A = abs(s) * (p * (pr["R_p"] * np.abs(lp + H) + pr["A_ly"] + A_H + 5 * U * np.abs(lp + H))
                  + FLT_MIN * np.abs(lp + H))
    return Held(v, abs(s) * p * (np.abs(lp) + abs(H)), 2 * A)


def _sim_prior_softmax(prior):
    pl = _f(prior).reshape(-1)
    mx = pl.max()
    lse = F32(mx + log32(exp32(pl - mx).sum(dtype=F32)))
    lp = (pl - lse).astype(F32)
    p = exp32(lp)
    return lp, p, F32(-(p * lp).sum(dtype=F32))


def sim_prior_logits_bwd(y, prior, gate, c, off_scale, free_nats):
    y = _f(y)
    lp, p, H = _sim_prior_softmax(prior)
    if gate:
        return (F32(c) * (p.reshape(1, -1) - y).sum(axis=0, dtype=F32)).astype(F32)
    return (F32(off_scale) * F32(free_nats) * (-p * (lp + H))).astype(F32)


# --------------------------------------------------------------------------
# the softplus-Gaussian pair
# --------------------------------------------------------------------------
def _softplus_rel(a):
    """softplusf(a) = max(a, 0) + log1p(exp(-|a|)): the exponential (2 |a| + 2) u,
    fast_log1p a log (3 u), a reciprocal (2 u), two products and the sums 1 + x,
    u - 1 it compensates (3 u), the final sum (u).  For a > 0 the logarithm is at
    most e^-a of the value and 2 a e^-a < 1."""
    a = np.asarray(a, dtype=np.float64)
    return U * (2 * np.maximum(-a, 0.0) + 12)


def _sigmoid_rel(a):
    """sigmoidf: the exponential, 1 + e, the reciprocal (2 u), e s."""
    return U * (2 * np.abs(np.asarray(a, dtype=np.float64)) + 6)


def pair(arrays, K, S, B, L):
    """scvae_softplus_gaussian_logprob_pair_fwd / _bwd.  ``arrays``: qm, qs
    [K*B, L]; Wpm, Wps [K, L]; bpm, bps [L]; eps, dz [K,S,B,L]; gklz [K,S,B].
    Values by autograd on om's restatement (du:52-73, gm:3272-3292) with the
    prior's parameters expanded per cell, so that dprior comes out per element.

    With R_sg = R_softplus / 2 + u (the root) the relative error of sigma, and
    the same for the prior's sp:
      qvar = sg sg          2 R_sg + u
      z = fma(sg, e, m)     A_z = |sg e| R_sg + u |z|
      pm = Wpm + bpm        A_pm = u |pm|
      d = z - pm            A_d = A_z + A_pm + u |d|
      v = d / sp            A_v = A_d / sp + |v| (R_sp + u)
      klz terms, per l:     e^2/2 (u), log sg (3 u |log sg| + R_sg), v^2/2
                            (|v| A_v + u v^2/2), log sp (3 u |log sp| + R_sp), three
                            additions (3 u sum |terms|); over L: 6 butterfly steps and
                            ceil(L/64) serial additions
      q1 = g v / sp         A_q1 = |g| A_v / sp + |q1| (R_sp + 2 u)
      dze = dz + q1         A_dze = A_q1 + u |dze|
      dqm = sum_s dze       sum A_dze + S u sum (|dz| + |q1|)
      gs = sum_s dze e - g / sg:  |e| A_dze + u |dze e|, |g / sg| (R_sg + u), and
                            (S + 1) u of the magnitudes for the additions
      dqs = gs sigmoid(qs) / (2 sg):  A_gs f + mag (R_sigmoid + R_sg + 3 u), f the factor
      d pm = -sum_s q1      sum A_q1 + S u sum |q1|
      gsp = sum_s g (1 - v^2) / sp:  A(1 - v^2) = 2 |v| A_v + u v^2 + u |1 - v^2|,
                            |g| A / sp + |t| (R_sp + 2 u), S u of the magnitudes
      d ps = gsp sigmoid(ps) / (2 sp)  as dqs
    Out-of-range pre-activations (beyond +-FLOAT32_MAX / 2) are clamped and get
    the gradient 0 exactly (``clipped_q``: [K*B, L] masks of qm, qs)."""
    a = {k: r32(v) for k, v in arrays.items()}
    t = {k: torch.from_numpy(np.array(v)) for k, v in a.items()}
    qm = t["qm"].reshape(K, B, L).clone().requires_grad_(True)
    qs = t["qs"].reshape(K, B, L).clone().requires_grad_(True)
    # (the device adds in fp32: the pre-activation it clamps is fl(W + b))
    pm_pre32 = r32(a["Wpm"] + a["bpm"])
    ps_pre32 = r32(a["Wps"] + a["bps"])
    pmp = torch.from_numpy(pm_pre32).reshape(K, 1, L).expand(K, B, L).clone().requires_grad_(True)
    psp = torch.from_numpy(ps_pre32).reshape(K, 1, L).expand(K, B, L).clone().requires_grad_(True)
    m = om._clip_big(qm)
    sq = om._clip_big(qs)
    sg = torch.sqrt(torch.nn.functional.softplus(sq))
    pm = om._clip_big(pmp)
    psc = om._clip_big(psp)
    sp = torch.sqrt(torch.nn.functional.softplus(psc))
    eps, dz, g = t["eps"], t["dz"], t["gklz"].reshape(K, S, B, 1)
    zz = m.unsqueeze(1) + sg.unsqueeze(1) * eps
    # om._normal_log_prob(z, m, sg) with (z - m) / sg = eps put in: for sg e below an
    # fp64 ulp of m the difference z - m is 0 in fp64 too, and the quotient with it
    log_q = -0.5 * eps ** 2 - torch.log(sg.unsqueeze(1)) - om.HALF_LOG_2PI
    kl_dims = log_q - om._normal_log_prob(zz, pm.unsqueeze(1), sp.unsqueeze(1))
    klz = kl_dims.sum(dim=-1)
    with np.errstate(all="ignore"):
        loss = (zz * dz).sum() + (klz * g.reshape(K, S, B)).sum()
        grads = torch.autograd.grad(loss, [qm, qs, pmp, psp])
    n = lambda x: x.detach().numpy()
    m, sq, sg, pm, psc, sp, zz = map(n, (m, sq, sg, pm, psc, sp, zz))
    e, dzn, g = n(eps), n(dz), n(g)
    with np.errstate(all="ignore"):
        R_sg = _softplus_rel(sq) / 2 + U
        R_sp = _softplus_rel(psc) / 2 + U
        sg1, sp1, m1, pm1 = sg[:, None], sp[:, None], m[:, None], pm[:, None]
        R_sg1, R_sp1 = R_sg[:, None], R_sp[:, None]
        A_z = np.abs(sg1 * e) * R_sg1 + U * np.abs(zz)
        d = zz - pm1
        A_d = A_z + U * np.abs(pm1) + U * np.abs(d)
        v = d / sp1
        A_v = A_d / sp1 + np.abs(v) * (R_sp1 + U)
        terms = np.stack(np.broadcast_arrays(0.5 * e * e, np.abs(np.log(sg1)), 0.5 * v * v,
                                             np.abs(np.log(sp1))))
        A_terms = (U * terms[0] + 3 * U * terms[1] + R_sg1 + np.abs(v) * A_v + U * terms[2]
                   + 3 * U * terms[3] + R_sp1)
        klz_mag = terms.sum(axis=0).sum(axis=-1)
        n_l = 3 + 6 + (L + 63) // 64
        klz_bound = A_terms.sum(axis=-1) + n_l * U * klz_mag
        q1 = g * v / sp1
        A_q1 = np.abs(g) * A_v / sp1 + np.abs(q1) * (R_sp1 + 2 * U)
        dze = dzn + q1
        A_dze = A_q1 + U * np.abs(dze)
        mag_dze = np.abs(dzn) + np.abs(q1)
        dqm_mag = mag_dze.sum(axis=1)
        dqm_bound = A_dze.sum(axis=1) + S * U * dqm_mag
        t_b = g / sg1
        gs_mag = (mag_dze * np.abs(e) + np.abs(t_b)).sum(axis=1)
        A_gs = ((np.abs(e) * A_dze + U * np.abs(dze * e) + np.abs(t_b) * (R_sg1 + U)).sum(axis=1)
                + (S + 1) * U * gs_mag)
        fq = 1.0 / (1.0 + np.exp(-sq)) / (2 * sg)
        dqs_mag = gs_mag * fq
        dqs_bound = A_gs * fq + dqs_mag * (_sigmoid_rel(sq) + R_sg + 3 * U)
        dpm_mag = np.abs(q1).sum(axis=1)
        dpm_bound = A_q1.sum(axis=1) + S * U * dpm_mag
        one_v2 = 1.0 - v * v
        A_1v2 = 2 * np.abs(v) * A_v + U * v * v + U * np.abs(one_v2)
        t_sp = g * one_v2 / sp1
        gsp_mag = (np.abs(g) * (1.0 + v * v) / sp1).sum(axis=1)
        A_gsp = ((np.abs(g) * A_1v2 / sp1 + np.abs(t_sp) * (R_sp1 + 2 * U)).sum(axis=1)
                 + S * U * gsp_mag)
        fp = 1.0 / (1.0 + np.exp(-psc)) / (2 * sp)
        dps_mag = gsp_mag * fp
        dps_bound = A_gsp * fp + dps_mag * (_sigmoid_rel(psc) + R_sp + 3 * U)
    qm_in, qs_in = a["qm"].reshape(K, B, L), a["qs"].reshape(K, B, L)
    clipped = dict(qm=np.abs(qm_in) > BIG, qs=np.abs(qs_in) > BIG,
                   pm=np.broadcast_to((np.abs(pm_pre32) > BIG).reshape(K, 1, L), (K, B, L)),
                   ps=np.broadcast_to((np.abs(ps_pre32) > BIG).reshape(K, 1, L), (K, B, L)))
    dpr_value = np.concatenate([n(grads[2]), n(grads[3])], axis=-1)
    out = dict(
        z=Held(zz, np.abs(sg1 * e) + np.abs(m1), 2 * A_z),
        qvar=Held(sg * sg, sg * sg, 2 * sg * sg * (2 * R_sg + U)),
        klz=Held(n(klz), klz_mag, 2 * klz_bound),
        dqm=Held(n(grads[0]), dqm_mag, 2 * dqm_bound),
        dqs=Held(n(grads[1]), dqs_mag, 2 * dqs_bound),
        dpr=Held(dpr_value, np.concatenate([dpm_mag, dps_mag], axis=-1),
                 2 * np.concatenate([dpm_bound, dps_bound], axis=-1)))
    info = dict(clipped=clipped, inv_sg=1.0 / np.where(sg > 0, sg, np.nan),
                abs_u=np.abs(v), pm_pre=pm_pre32, ps_pre=ps_pre32)
    return out, info


def sim_pair(arrays, K, S, B, L):
    a = {k: _f(v) for k, v in arrays.items()}
    qm_pre, qs_pre = a["qm"].reshape(K, 1, B, L), a["qs"].reshape(K, 1, B, L)
    pm_pre = (a["Wpm"] + a["bpm"]).astype(F32).reshape(K, 1, 1, L)
    ps_pre = (a["Wps"] + a["bps"]).astype(F32).reshape(K, 1, 1, L)
    e, dz, g = a["eps"], a["dz"], a["gklz"].reshape(K, S, B, 1)
    with np.errstate(all="ignore"):
        m, sq = clip32(qm_pre), clip32(qs_pre)
        sg = np.sqrt(softplus32(sq))
        pm, pc = clip32(pm_pre), clip32(ps_pre)
        sp = np.sqrt(softplus32(pc))
        zz = (sg * e + m).astype(F32)
        v = ((zz - pm) / sp).astype(F32)
        kl = (F32(-0.5) * e * e - log32(sg) + F32(0.5) * v * v + log32(sp)).astype(F32)
        klz = kl.sum(axis=-1, dtype=F32)
        q1 = (g * v / sp).astype(F32)
        dze = (dz + q1).astype(F32)
        gm = dze.sum(axis=1, dtype=F32)
        gs = (dze * e - g / sg).astype(F32).sum(axis=1, dtype=F32)
        gpm = -(q1.sum(axis=1, dtype=F32))
        gsp = (g * (F32(1) - v * v) / sp).astype(F32).sum(axis=1, dtype=F32)
        big = F32(BIG)
        dqm = np.where(np.abs(qm_pre[:, 0]) <= big, gm, F32(0))
        dqs = np.where(np.abs(qs_pre[:, 0]) <= big,
                       gs * sigmoid32(sq[:, 0]) / (F32(2) * sg[:, 0]), F32(0))
        dps = gsp * sigmoid32(pc[:, 0]) / (F32(2) * sp[:, 0])
        dpr = np.concatenate([np.broadcast_to(gpm, (K, B, L)),
                              np.broadcast_to(dps, (K, B, L))], axis=-1)
    return dict(z=zz, klz=klz, qvar=np.broadcast_to((sg * sg)[:, 0], (K, B, L)),
                dqm=dqm, dqs=dqs, dpr=dpr.astype(F32))


def prior_stats(Wpm, bpm, Wps, bps):
    """scvae_prior_stats: clip(fl(Wpm + bpm)) (u) and softplus of the clamped
    fl(Wps + bps) (R_softplus)."""
    with np.errstate(all="ignore"):
        pm = np.clip(r32(r32(Wpm) + r32(bpm)), -BIG, BIG)
        pc = np.clip(r32(r32(Wps) + r32(bps)), -BIG, BIG)
    var = np.maximum(pc, 0) + np.log1p(np.exp(-np.abs(pc)))
    return dict(means=Held(pm, np.abs(pm), 0.0 * pm),     # (the sum rounded as the device's)
                variances=Held(var, var, 2 * var * _softplus_rel(pc)))


def sim_prior_stats(Wpm, bpm, Wps, bps):
    with np.errstate(all="ignore"):
        return (clip32((_f(Wpm) + _f(bpm)).astype(F32)),
                softplus32(clip32((_f(Wps) + _f(bps)).astype(F32))))


# --------------------------------------------------------------------------
# the mixture ELBO
# --------------------------------------------------------------------------
def elbo_fwd(ll, klz, y, kl_y_cell, inv_gb, w, free_nats, share, prior=None):
    """scvae_mixture_elbo_fwd -> sums [3], rec_cell [B], scalars [0..4], gate, thr.
      a cell:  sum_k (sum_s ll) inv_s y_k: S - 1 additions, inv_s (u), two products,
               K additions: (K + S + 3) u sum_k y_k mean_s |ll|
      sums:    ceil(B/256) - 1 additions per thread, 10 in block_sum<256>, inv_gb
      thr:     free_nats logf(K) on the host (2 u), free_nats H[p] on the device
      scalars: from the sums the device holds, their own errors carried:
               (rec - (kz + ky)) share, (rec - w (kz + max(ky, thr))) share: 3 / 4 u of
               the magnitudes"""
    ll, klz, y, kl_y_cell = r32(ll), r32(klz), r32(y), r32(kl_y_cell)
    K, S, B = ll.shape
    inv_gb, w, free_nats, share = (float(r32(v)) for v in (inv_gb, w, free_nats, share))
    nk = K + S + 3
    nB = (B + 255) // 256 + 10
    rc = (ll.mean(axis=1) * y.T).sum(axis=0)
    rc_mag = (np.abs(ll).mean(axis=1) * y.T).sum(axis=0)
    kc = (klz.mean(axis=1) * y.T).sum(axis=0)
    kc_mag = (np.abs(klz).mean(axis=1) * y.T).sum(axis=0)
    rec, kz, ky = inv_gb * rc.sum(), inv_gb * kc.sum(), inv_gb * kl_y_cell.sum()
    mags = np.array([inv_gb * rc_mag.sum(), inv_gb * kc_mag.sum(),
                     inv_gb * np.abs(kl_y_cell).sum()])
    A = U * mags * np.array([nk + nB + 1, nk + nB + 1, nB + 1])
    if prior is None:
        thr = free_nats * math.log(K)
        A_thr = 2 * U * thr
    else:
        _, H, A_H = _entropy_terms(prior, K)
        thr = free_nats * H
        A_thr = free_nats * A_H + U * thr
    gate = 1.0 if (free_nats == 0.0 or ky > thr) else 0.0
    ky_mod = max(ky, thr) if free_nats != 0.0 else ky
    A_mod = max(A[2], A_thr) if free_nats != 0.0 else A[2]
    sc = np.array([(rec - (kz + ky)) * share, (rec - w * (kz + ky_mod)) * share,
                   rec * share, kz * share, ky * share])
    sc_mag = share * np.array([mags.sum(), mags[0] + w * (mags[1] + max(mags[2], abs(thr))),
                               mags[0], mags[1], mags[2]])
    A_sc = share * np.array([
        A.sum() + 3 * U * (abs(rec) + abs(kz) + abs(ky)),
        A[0] + w * (A[1] + A_mod) + 4 * U * (abs(rec) + w * (abs(kz) + abs(ky_mod))),
        A[0] + U * abs(rec), A[1] + U * abs(kz), A[2] + U * abs(ky)])
    return dict(sums=Held(np.array([rec, kz, ky]), mags, 2 * A),
                rec_cell=Held(rc, rc_mag, 2 * nk * U * rc_mag),
                scalars=Held(sc, sc_mag, 2 * A_sc),
                gate=gate, thr=thr, margin=abs(ky - thr), margin_needed=2 * (A[2] + A_thr))


def sim_elbo_fwd(ll, klz, y, kl_y_cell, inv_gb, w, free_nats, share, prior=None):
    ll, klz, y, kl_y_cell = _f(ll), _f(klz), _f(y), _f(kl_y_cell)
    K, S, B = ll.shape
    inv_s = F32(1) / F32(S)
    rc = (ll.sum(axis=1, dtype=F32) * inv_s * y.T).sum(axis=0, dtype=F32)
    kc = (klz.sum(axis=1, dtype=F32) * inv_s * y.T).sum(axis=0, dtype=F32)
    igb = F32(inv_gb)
    rec, kz, ky = rc.sum(dtype=F32) * igb, kc.sum(dtype=F32) * igb, kl_y_cell.sum(dtype=F32) * igb
    if prior is None:
        thr = F32(free_nats) * F32(math.log(F32(K)))
    else:
        thr = F32(free_nats) * _sim_prior_softmax(prior)[2]
    use = F32(free_nats) != 0
    ky_mod = (ky if ky > thr else thr) if use else ky
    sh, w = F32(share), F32(w)
    sc = np.array([(rec - (kz + ky)) * sh, (rec - w * (kz + ky_mod)) * sh, rec * sh, kz * sh,
                   ky * sh], dtype=F32)
    gate = F32(1) if (not use or ky > thr) else F32(0)
    return dict(sums=np.array([rec, kz, ky], dtype=F32), rec_cell=rc, scalars=sc, gate=gate)


def elbo_bwd(ll, klz, y, w, inv_gb):
    """scvae_mixture_elbo_bwd, by autograd on -inv_gb sum_b sum_k y (mean_s ll -
    w mean_s klz):  gw: inv_s (u) and two products: 4 u; gklz: one more; dy: S - 1
    additions, inv_s, the products, the sum and inv_gb: (S + 5) u of the magnitudes."""
    K, S, B = np.shape(ll)
    inv_gb, w = float(r32(inv_gb)), float(r32(w))
    lt = torch.from_numpy(np.array(r32(ll))).requires_grad_(True)
    kt = torch.from_numpy(np.array(r32(klz))).requires_grad_(True)
    yt = torch.from_numpy(np.array(r32(y))).requires_grad_(True)
    loss = -inv_gb * ((lt.mean(dim=1) - w * kt.mean(dim=1)) * yt.t()).sum()
    gw, gk, dy = (g.numpy() for g in torch.autograd.grad(loss, [lt, kt, yt]))
    dy_mag = inv_gb * (np.abs(r32(ll)).mean(axis=1) + w * np.abs(r32(klz)).mean(axis=1)).T
    return dict(gw=Held(gw, np.abs(gw), 2 * 4 * U * np.abs(gw)),
                gklz=Held(gk, np.abs(gk), 2 * 5 * U * np.abs(gk)),
                dy=Held(dy, dy_mag, 2 * (S + 5) * U * dy_mag))


def sim_elbo_bwd(ll, klz, y, w, inv_gb):
    ll, klz, y = _f(ll), _f(klz), _f(y)
    K, S, B = ll.shape
    inv_s, igb, w = F32(1) / F32(S), F32(inv_gb), F32(w)
    yk = y.T.reshape(K, 1, B)
    gw = np.broadcast_to(-yk * inv_s * igb, (K, S, B)).astype(F32)
    gk = np.broadcast_to(w * yk * inv_s * igb, (K, S, B)).astype(F32)
    dy = ((-ll.sum(axis=1, dtype=F32) * inv_s + w * klz.sum(axis=1, dtype=F32) * inv_s)
          * igb).T
    return dict(gw=gw, gklz=gk, dy=dy.astype(F32))


# --------------------------------------------------------------------------
# the group reductions
# --------------------------------------------------------------------------
GROUP_MAX_CHUNKS = 64      # (kernels.hpp BN_MAX_CHUNKS)


def group_col_sum(a, R, G, N, scale):
    """scvae_group_col_sum on a [G*R, >= N]: a column passes ceil(chunk/16) - 1
    additions in a thread, 16 over the row lanes, one per chunk and the scale."""
    a = r32(a)[:, :N].reshape(G, R, N)
    chunks = min((R + 255) // 256, GROUP_MAX_CHUNKS)
    chunk = (R + chunks - 1) // chunks
    chunks = (R + chunk - 1) // chunk
    n = (chunk + 15) // 16 + 16 + chunks + 1
    scale = float(r32(scale))
    mag = abs(scale) * np.abs(a).sum(axis=1)
    return Held(scale * a.sum(axis=1), mag, 2 * n * U * mag)


def sim_group_col_sum(a, R, G, N, scale):
    return (_f(a)[:, :N].reshape(G, R, N).sum(axis=1, dtype=F32) * F32(scale)).astype(F32)


def sum_groups(a, w, G, R, N):
    """scvae_sum_groups: G products and G additions, serial."""
    a = r32(a).reshape(G, R, N)
    terms = a if w is None else a * r32(w).T.reshape(G, R, 1)
    mag = np.abs(terms).sum(axis=0)
    return Held(terms.sum(axis=0), mag, 2 * (G + 1) * U * mag)


def sim_sum_groups(a, w, G, R, N):
    a = _f(a).reshape(G, R, N)
    terms = a if w is None else (a * _f(w).T.reshape(G, R, 1)).astype(F32)
    return terms.sum(axis=0, dtype=F32)


def add_group_rows(a0, rows, relu):
    """scvae_add_group_rows: one addition (the ReLU of a rounded sum is within the
    sum's rounding of the ReLU of the exact one)."""
    v = r32(a0)[None, :, :] + r32(rows)[:, None, :]
    mag = np.abs(r32(a0))[None, :, :] + np.abs(r32(rows))[:, None, :]
    return Held(np.maximum(v, 0.0) if relu else v, mag, 2 * U * np.abs(v))


def sim_add_group_rows(a0, rows, relu):
    v = (_f(a0)[None, :, :] + _f(rows)[:, None, :]).astype(F32)
    return np.maximum(v, F32(0)) if relu else v


# --------------------------------------------------------------------------
# the inputs both test files use
# --------------------------------------------------------------------------
CAT_K = [1, 2, 63, 64, 65, 129, 200]
CAT_B = [1, 3, 4, 5, 513]
CAT_REGIMES = ["ordinary", "near-uniform", "equal", "spread-20", "spread-60"]
GAP_ROWS = {0: 95.0, 1: 120.0}      # row -> gap of its smallest logit to the maximum


def categorical_inputs(K, B, regime="ordinary", learned=False):
    rng = np.random.default_rng(1000 * K + B + 7 * CAT_REGIMES.index(regime))
    if regime == "ordinary":
        logits = rng.normal(0, 2, (B, K))
    elif regime == "near-uniform":
        logits = 1e-4 * rng.normal(0, 1, (B, K))
    elif regime == "equal":
        logits = np.full((B, K), 0.75)
    else:
        spread = float(regime.split("-")[1])
        logits = rng.uniform(-spread / 2, spread / 2, (B, K))
        for row, gap in GAP_ROWS.items():
            # (down from the row's maximum through the subnormal range to 0)
            if row < B and K > 1:
                logits[row] = logits[row].max() - np.linspace(0.0, gap, K)
    prior = rng.normal(0, 1, K) if learned else None
    dy = rng.normal(0, 1, (B, K))
    return _f(logits), (None if prior is None else _f(prior)), _f(dy), 0.37


PAIR_SHAPES = [(K, S, B, L) for L in (1, 63, 64, 65, 130) for S in (1, 3)
               for K, B in ((1, 1), (3, 7))] + [(3, 1, 1400, 130)]
SCALES = (-80.0, -30.0, 0.0, 30.0, 80.0)


def pair_inputs(K, S, B, L, regime="ordinary"):
    rng = np.random.default_rng(K * 1000 + S * 100 + B * 10 + L)
    arrays = dict(qm=rng.normal(0, 1, (K * B, L)), qs=rng.normal(0, 1.5, (K * B, L)),
                  Wpm=rng.normal(0, 1, (K, L)), bpm=rng.normal(0, 0.3, L),
                  Wps=rng.normal(0, 1, (K, L)), bps=rng.normal(0, 0.3, L),
                  eps=rng.normal(0, 1, (K, S, B, L)),
                  dz=rng.normal(0, 1, (K, S, B, L)), gklz=rng.normal(0, 1, (K, S, B)))
    if regime == "scales":
        # Pre-activations of both scales from SCALES, mixed within every row.
        # g (1 - v^2) / sp with v = (z - pm) / sp has to stay inside fp32 for
        # sp = sqrt(softplus(-80)) = 4e-18, so the inputs keep |v| moderate: the
        # posterior's scale at or below the prior's, its mean within a few
        # prior sigmas of the prior's; where the prior's scale is the smallest
        # the prior mean is exactly 0 (fl(pm + sp nu) would be pm otherwise).
        ip = rng.integers(0, len(SCALES), (K, L))
        iq = np.minimum(rng.integers(0, len(SCALES), (K, B, L)), ip[:, None, :])
        sc = np.asarray(SCALES)
        arrays["bps"] = np.zeros(L)
        arrays["Wps"] = sc[ip]
        arrays["qs"] = sc[iq].reshape(K * B, L)
        arrays["bpm"] = _f(arrays["bpm"])
        arrays["Wpm"] = np.where(ip == 0, -arrays["bpm"][None, :], _f(arrays["Wpm"]))
        pm = (_f(arrays["Wpm"]) + _f(arrays["bpm"])).astype(F32).astype(np.float64)
        sp = np.sqrt(np.maximum(sc[ip], 0) + np.log1p(np.exp(-np.abs(sc[ip]))))
        arrays["qm"] = (pm[:, None, :] + sp[:, None, :] * rng.normal(0, 1, (K, B, L))
                        ).reshape(K * B, L)
    return {k: _f(v) for k, v in arrays.items()}


# The clip (K = 4, B = 5, L = 6): every out-of-range element sits in cluster 3,
# whose prior is out of range too, so the rows (3, b) -- a quarter of them -- are
# the ones whose klz and gradients fp32 cannot hold.
CLIP_SHAPE = (4, 2, 5, 6)
CLIP_BAD_CLUSTER = 3
CLIP_ELEMENTS = {          # name -> [(k, b or None, l, value)]
    "qm": [(3, 0, 0, 2e38), (3, 1, 1, -2e38), (3, 2, 2, np.inf), (3, 3, 3, -np.inf)],
    "qs": [(3, 0, 4, 2e38), (3, 1, 5, -2e38), (3, 4, 0, np.inf), (3, 2, 1, -np.inf)],
    "Wpm": [(3, None, 0, 2e38), (3, None, 1, -np.inf)],
    "Wps": [(3, None, 2, np.inf), (3, None, 3, -2e38)],
}


def clip_inputs():
    K, S, B, L = CLIP_SHAPE
    arrays = {k: np.array(v) for k, v in pair_inputs(K, S, B, L).items()}
    for name, elements in CLIP_ELEMENTS.items():
        for k, b, l, value in elements:
            if b is None:
                arrays[name][k, l] = value
            else:
                arrays[name][k * B + b, l] = value
    return {k: _f(v) for k, v in arrays.items()}


ELBO_SHAPES = ([(K, 1, B) for K in (1, 7, 8, 9, 17) for B in (1, 255, 256, 257, 600)]
               + [(K, 2, B) for K in (3, 9) for B in (1, 255, 256, 257, 600)]
               + [(130, 1, 2100)])
ELBO_SHARES = [1.0, 1.0 / 3]
ELBO_WEIGHTS = [0.0, 0.6, 1.0]


def elbo_inputs(K, S, B):
    rng = np.random.default_rng(K * 7 + S * 3 + B)
    ll = rng.normal(-300, 30, (K, S, B))
    klz = rng.gamma(2.0, 2.0, (K, S, B))
    logits = rng.normal(0, 1.5, (B, K))
    y = np.exp(logits - logits.max(axis=1, keepdims=True))
    y /= y.sum(axis=1, keepdims=True)
    kl_y = rng.gamma(2.0, 0.2, B)
    return _f(ll), _f(klz), _f(y), _f(kl_y)


# The free-nats gate: (prior kind, side) -> logits [B, K] of q(y|x) and the prior
# logits (None: uniform).  "above": peaked posteriors, KL_y well over the
# threshold free_nats H[p]; "below": posteriors close to the prior.
GATE_K, GATE_B, GATE_FREE_NATS = 9, 37, 0.5
GATE_CUSTOM = tuple(np.arange(1, GATE_K + 1) / np.arange(1, GATE_K + 1).sum())
GATE_CASES = [(p, s) for p in ("uniform", "custom", "learned") for s in ("above", "below")]


def gate_inputs(prior_kind, side):
    rng = np.random.default_rng(11 + len(prior_kind) + (side == "above"))
    K, B = GATE_K, GATE_B
    if prior_kind == "uniform":
        prior = None
    elif prior_kind == "custom":       # (log of the given probabilities, as the plan holds them)
        prior = _f(np.log(np.asarray(GATE_CUSTOM)))
    else:
        prior = _f(rng.normal(0, 0.8, K))
    base = np.zeros(K) if prior is None else prior.astype(np.float64)
    logits = base + (4.0 if side == "above" else 0.3) * rng.normal(0, 1, (B, K))
    S = 2
    ll = rng.normal(-300, 30, (K, S, B))
    klz = rng.gamma(2.0, 2.0, (K, S, B))
    dy = rng.normal(0, 1, (B, K))
    return dict(logits=_f(logits), prior=prior, ll=_f(ll), klz=_f(klz), dy=_f(dy), S=S,
                learned=prior_kind == "learned")


GROUP_COL_SUM_CASES = ([(R, 65, 3, 65, 1.0) for R in (1, 15, 16, 17, 256, 257)]
                       + [(17, N, 1, N, 1.0) for N in (1, 63, 64, 130)]
                       + [(16385, 5, 3, 5, 1.0), (257, 70, 3, 63, 1.0),
                          (257, 64, 1, 64, 1.0 / 257)])
# (R, lda, G, N, scale): R = 16385 is past 64 chunks of 256 rows; lda > N; scale != 1


def group_inputs(*shape):
    rng = np.random.default_rng(sum(int(v) for v in shape))
    return _f(rng.normal(0.3, 1.0, shape))


# --------------------------------------------------------------------------
# the checks, written once: ``run`` is the GPU library (test_gpu_mixture_stage.py)
# or ``Fp32Evaluation`` below (test_mixture_oracle_host.py)
# --------------------------------------------------------------------------
class Fp32Evaluation:
    """The entries in plain NumPy fp32, in the kernels' order of operations."""

    def cat_fwd(self, logits, prior):
        return sim_categorical_fwd(logits, prior)

    def cat_bwd(self, y, dy, gate, c, prior):
        return sim_categorical_bwd(y, dy, gate, c, prior)

    def prior_bwd(self, y, prior, gate, c, off_scale, free_nats):
        return sim_prior_logits_bwd(y, prior, gate, c, off_scale, free_nats)

    def pair(self, arrays, K, S, B, L):
        return sim_pair(arrays, K, S, B, L)

    def prior_stats(self, Wpm, bpm, Wps, bps):
        return sim_prior_stats(Wpm, bpm, Wps, bps)

    def elbo_fwd(self, ll, klz, y, kl_y_cell, inv_gb, w, free_nats, share, prior, scalars=None):
        out = sim_elbo_fwd(ll, klz, y, kl_y_cell, inv_gb, w, free_nats, share, prior)
        full = np.zeros(8, dtype=F32) if scalars is None else scalars
        full[:5] = out["scalars"]
        if not np.isfinite(out["scalars"][0]):
            full[7] += 1
        out["scalars"] = full
        return out

    def elbo_bwd(self, ll, klz, y, w, inv_gb):
        return sim_elbo_bwd(ll, klz, y, w, inv_gb)

    def group_col_sum(self, a, R, G, N, scale):
        return sim_group_col_sum(a, R, G, N, scale)

    def sum_groups(self, a, w, G, R, N):
        return sim_sum_groups(a, w, G, R, N)

    def add_group_rows(self, a0, rows, relu):
        return sim_add_group_rows(a0, rows, relu)


def check_categorical(run, K, B, regime, learned, report=None):
    """Forward and both gate states of the backward, every element on its own
    bound (``categorical_fwd`` / ``categorical_bwd`` derive them)."""
    logits, prior, dy, c = categorical_inputs(K, B, regime, learned)
    tag = " [K {} B {} {} {}]".format(K, B, regime, "learned" if learned else "uniform")
    y, kl = run.cat_fwd(logits, prior)
    want, info = categorical_fwd(logits, prior)
    assert np.isfinite(y).all() and np.isfinite(kl).all(), "non-finite forward" + tag
    hold("y" + tag, y, want["y"], report=report)
    hold("kl_y_cell" + tag, kl, want["kl"], report=report)
    if regime in ("near-uniform", "equal") and not learned:
        # KL(q || uniform) >= 0: the fp32 value may be below 0 by its bound only
        assert (np.asarray(kl, dtype=np.float64) >= -want["kl"].bound).all(), tag
    if regime.startswith("spread") and K > 1:
        gone = want["y"].value < FLT_MIN / 4
        if K >= 63 and B > 1:       # (the gap rows do reach 0)
            assert gone.any(), tag
        # below a quarter of FLT_MIN a flushing exponential and a denormal one
        # both stay under the absolute bound 2 FLT_MIN; nothing turns up there
        assert (np.asarray(y, dtype=np.float64)[gone] <= 2 * FLT_MIN).all(), tag
    for gate in (1.0, 0.0):
        dl = run.cat_bwd(y, dy, gate, c, prior)
        hold("dlogits gate {:.0f}".format(gate) + tag, dl,
             categorical_bwd(y, dy, gate, c, prior), report=report)
    return info


def _pair_masks(info, K, B, L):
    """Rows [K, B] that hold no out-of-range element, of theirs or their prior's."""
    c = info["clipped"]
    bad = (c["qm"] | c["qs"] | c["pm"] | c["ps"]).any(axis=-1)
    return ~bad


def check_pair(run, K, S, B, L, regime="ordinary", report=None):
    """The pair's forward and backward, per element (``pair`` derives the bounds)."""
    arrays = clip_inputs() if regime == "clip" else pair_inputs(K, S, B, L, regime)
    tag = " [K {} S {} B {} L {} {}]".format(K, S, B, L, regime)
    got = run.pair(arrays, K, S, B, L)
    want, info = pair(arrays, K, S, B, L)
    rows = _pair_masks(info, K, B, L)                    # [K, B]
    if regime == "clip":
        # by construction: exactly the rows of CLIP_BAD_CLUSTER, a quarter of them
        expect = np.ones((K, B), dtype=bool)
        expect[CLIP_BAD_CLUSTER] = False
        assert (rows == expect).all() and (~rows).mean() <= 0.25
    else:
        assert rows.all()
    el = rows[:, :, None]
    # z and qvar are the values of the clamped inputs wherever those are finite
    finite_z = np.isfinite(want["z"].value) & np.isfinite(want["z"].bound)
    hold("z" + tag, got["z"], want["z"], mask=finite_z, report=report)
    hold("qvar" + tag, got["qvar"], want["qvar"], report=report)
    hold("klz" + tag, got["klz"], want["klz"], mask=rows[:, None, :], report=report)
    hold("dqm" + tag, got["dqm"], want["dqm"], mask=el, report=report)
    hold("dqs" + tag, got["dqs"], want["dqs"], mask=el, report=report)
    hold("dprior" + tag, got["dpr"], want["dpr"], mask=el, report=report)
    # the gradient of a clamped pre-activation is exactly 0
    c = info["clipped"]
    dqm = np.asarray(got["dqm"]).reshape(K, B, L)
    dqs = np.asarray(got["dqs"]).reshape(K, B, L)
    assert (dqm[c["qm"]] == 0).all() and (dqs[c["qs"]] == 0).all(), tag
    if regime == "clip":
        assert c["qm"].sum() == 4 and c["qs"].sum() == 4
    return info


def check_prior_stats(run, K, L, clip=False, report=None):
    arrays = clip_inputs() if clip else pair_inputs(K, 1, 1, L)
    args = [arrays[k] for k in ("Wpm", "bpm", "Wps", "bps")]
    means, variances = run.prior_stats(*args)
    want = prior_stats(*args)
    tag = " [K {} L {}{}]".format(K, L, " clip" if clip else "")
    hold("p_z_means" + tag, means, want["means"], report=report)
    hold("p_z_variances" + tag, variances, want["variances"], report=report)


def check_elbo(run, K, S, B, w, share, report=None):
    ll, klz, y, kl_y = elbo_inputs(K, S, B)
    inv_gb = share / B            # (a rank holding `share` of the global minibatch)
    tag = " [K {} S {} B {} w {} share {:.2f}]".format(K, S, B, w, share)
    got = run.elbo_fwd(ll, klz, y, kl_y, inv_gb, w, 0.0, share, None)
    want = elbo_fwd(ll, klz, y, kl_y, inv_gb, w, 0.0, share, None)
    hold("sums" + tag, got["sums"], want["sums"], report=report)
    hold("rec_cell" + tag, got["rec_cell"], want["rec_cell"], report=report)
    hold("scalars" + tag, got["scalars"][:5], want["scalars"], report=report)
    assert got["gate"] == 1.0 and got["scalars"][7] == 0.0, tag   # (free_nats = 0)
    gb = run.elbo_bwd(ll, klz, y, w, inv_gb)
    wb = elbo_bwd(ll, klz, y, w, inv_gb)
    for name in ("gw", "gklz", "dy"):
        hold(name + tag, gb[name], wb[name], report=report)


def check_gate(run, prior_kind, side, report=None):
    """The free-nats gate end to end: categorical forward -> mixture ELBO ->
    gate -> categorical backward and the prior logits' gradient, each stage
    against its oracle ON THE INPUTS IT WAS GIVEN (the stage before's fp32
    output), the gate decision against fp64 from the logits."""
    d = gate_inputs(prior_kind, side)
    K, B, S, prior = GATE_K, GATE_B, d["S"], d["prior"]
    w, share, fn = 0.6, 1.0, GATE_FREE_NATS
    inv_gb = 1.0 / B
    tag = " [{} prior, KL_y {} the threshold]".format(prior_kind, side)
    exact, _ = categorical_fwd(d["logits"], prior)
    y, kl = run.cat_fwd(d["logits"], prior)
    hold("kl_y_cell" + tag, kl, exact["kl"], report=report)
    got = run.elbo_fwd(d["ll"], d["klz"], y, kl, inv_gb, w, fn, share, prior)
    want = elbo_fwd(d["ll"], d["klz"], y, kl, inv_gb, w, fn, share, prior)
    # the decision as fp64 takes it from the logits, 1e-3 thr clear of the threshold
    ky64 = exact["kl"].value.mean()
    assert abs(ky64 - want["thr"]) >= 1e-3 * want["thr"] > want["margin_needed"], tag
    assert (ky64 > want["thr"]) == (side == "above"), tag
    assert want["gate"] == (1.0 if side == "above" else 0.0), tag
    assert float(got["gate"]) == want["gate"], "gate" + tag
    hold("scalars" + tag, got["scalars"][:5], want["scalars"], report=report)
    gate = want["gate"]
    dy = run.elbo_bwd(d["ll"], d["klz"], y, w, inv_gb)["dy"]
    hold("dy" + tag, dy, elbo_bwd(d["ll"], d["klz"], y, w, inv_gb)["dy"], report=report)
    dl = run.cat_bwd(y, dy, float(got["gate"]), w * inv_gb, prior)
    hold("dlogits" + tag, dl, categorical_bwd(y, dy, gate, w * inv_gb, prior), report=report)
    if d["learned"]:
        dp = run.prior_bwd(y, prior, float(got["gate"]), w * inv_gb, w * share, fn)
        hold("dprior" + tag, dp,
             prior_logits_bwd(y, prior, gate, w * inv_gb, w * share, fn), report=report)
    # free_nats = 0: the gate is 1 whatever KL_y is
    assert float(run.elbo_fwd(d["ll"], d["klz"], y, kl, inv_gb, w, 0.0, share,
                              prior)["gate"]) == 1.0, tag
    return want


def check_prior_bwd_shapes(run, K, B, report=None):
    """prior_logits_bwd on its own, both gate states, past one pass of 256 cells."""
    logits, prior, _, _ = categorical_inputs(K, B, "ordinary", True)
    y = np.asarray(categorical_fwd(logits, prior)[0]["y"].value, dtype=F32)
    for gate in (1.0, 0.0):
        dp = run.prior_bwd(y, prior, gate, 0.6 / B, 0.6, 0.5)
        hold("dprior gate {:.0f} [K {} B {}]".format(gate, K, B), dp,
             prior_logits_bwd(y, prior, gate, 0.6 / B, 0.6, 0.5), report=report)


def check_group_col_sum(run, R, lda, G, N, scale, report=None):
    a = group_inputs(G * R, lda)
    tag = " [R {} lda {} G {} N {}]".format(R, lda, G, N)
    hold("group_col_sum" + tag, run.group_col_sum(a, R, G, N, scale),
         group_col_sum(a, R, G, N, scale), report=report)


def check_sum_groups(run, G, R, N, weighted, report=None):
    a = group_inputs(G * R, N)
    w = np.abs(group_inputs(R, G)) if weighted else None
    tag = " [G {} R {} N {} {}]".format(G, R, N, "weighted" if weighted else "plain")
    hold("sum_groups" + tag, run.sum_groups(a, w, G, R, N), sum_groups(a, w, G, R, N),
         report=report)


def check_add_group_rows(run, K, B, N, relu, report=None):
    a0, rows = group_inputs(B, N), group_inputs(K, N + 0) - F32(0.3)
    tag = " [K {} B {} N {} relu {}]".format(K, B, N, relu)
    hold("add_group_rows" + tag, run.add_group_rows(a0, rows, relu),
         add_group_rows(a0, rows, relu), report=report)
