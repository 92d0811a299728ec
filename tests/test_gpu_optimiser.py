"""The optimiser against fp64: ``scvae_adam_clip_step`` element by element
(clip, ``grad_scale``, carried moments, the float4 body's grid stride and its
1-3 element tail), and ``Engine.adam_step`` over six steps against
``om.clip_and_adam`` iterated six times (``lr_t`` of step t, ``adam_t`` through
``state_dict`` / ``load_state_dict`` and through ``initialise``).

The formula (include/scvae_hip.h, _setup_optimiser, va:2736-2770):

    gc = clip(g * grad_scale, -1, 1)
    m' = beta1 * m + (1 - beta1) * gc
    v' = beta2 * v + (1 - beta2) * gc * gc
    theta' = theta - lr_t * m' / (sqrt(v') + epsilon)

Every bound below counts fp32 roundings; u = 2^-24 is half an ulp relative to
a value (the most one rounding moves it), and each expression is allowed TWICE
its count of roundings times u times the summed magnitudes of its terms.
``1 - beta`` is exact in fp32 for both betas (Sterbenz), and a contracted
multiply-add only removes roundings from the counts.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import models as om
from _parity import close_elementwise, close_per_tensor

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = -7777.25
PAD = 8
B1 = np.float32(om.ADAM_BETA1)
B2 = np.float32(om.ADAM_BETA2)
EPS = np.float32(om.ADAM_EPSILON)

# 2048 blocks x 256 threads x 4 floats, one more float4 for each thread of the
# first four blocks' worth (a second grid-stride trip), and a tail of three
BIG = 2048 * 256 * 4 + 4 * 256 + 3
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1025, BIG]
SCALES = [np.float32(1.0), np.float32(0.25), np.float32(1.0) / np.float32(3.0)]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buffer(values, device):
    """``values`` (fp32) followed by PAD canaries, 16-byte aligned."""
    host = np.full(values.size + PAD, CANARY, dtype=np.float32)
    host[:values.size] = values
    t = torch.from_numpy(host).to(device)
    assert t.data_ptr() % 16 == 0
    return t


def _gradient(rng, n, scale):
    """Ordinary values that cross the clip once scaled, and at every third
    place one of: 0, +-1e-12, +-0.3, +-1/scale with its two fp32 neighbours,
    +-50, +-3e38 (the rotation by ``n`` brings different ones to the small
    sizes and to the tail)."""
    edge = np.float32(1.0 / np.float64(scale))
    below, above = np.nextafter(edge, np.float32(0)), np.nextafter(
        edge, np.float32(np.inf))
    specials = np.array(
        [0.0, 1e-12, -1e-12, 0.3, -0.3, edge, -edge, below, -below, above,
         -above, 50.0, -50.0, 3e38, -3e38], dtype=np.float32)
    g = (rng.normal(0.0, 0.6, n) / np.float64(scale)).astype(np.float32)
    at = np.arange(0, n, 3)
    g[at] = specials[(at // 3 + n) % specials.size]
    return g


def _reference(theta, g, m, v, scale, lr_t):
    """The formula in fp64 on the fp32 values the device holds, and the
    bounds (see the module docstring for the rule)."""
    theta, g, m, v = (a.astype(np.float64) for a in (theta, g, m, v))
    b1, b2, eps = np.float64(B1), np.float64(B2), np.float64(EPS)
    c1, c2 = np.float64(np.float32(1) - B1), np.float64(np.float32(1) - B2)
    lr = np.float64(lr_t)
    gc = np.clip(g * np.float64(scale), -1.0, 1.0)
    # m': g*scale, beta1*m, (1-beta1)*gc, the sum: 4 roundings
    m_mag = np.abs(b1 * m) + np.abs(c1 * gc)
    m_new = b1 * m + c1 * gc
    m_tol = 2 * 4 * U * m_mag
    # v': g*scale enters twice, (1-beta2)*gc, *gc, beta2*v, the sum: 6
    # roundings (every term is positive: the magnitudes sum to v' itself)
    v_new = b2 * v + c2 * gc * gc
    v_tol = 2 * 6 * U * v_new
    # theta': with d = sqrt(v') + epsilon and the update q = lr_t * m' / d,
    #   m' carries its 4 roundings of m_mag                 -> 4 u lr_t m_mag / d
    #   sqrt halves the 6 of v' (3), rounds (1), + epsilon rounds (1): d by 5 u,
    #   lr_t * m' rounds (1), the division rounds (1)       -> 7 u |q|
    #   theta - q rounds once, by at most u (|theta| + |q|) -> u (|theta| + |q|)
    # 4 + 7 + 1 = 12 roundings; |q| <= lr_t m_mag / d, so all of them are
    # within 12 u (lr_t m_mag / d + |theta|), allowed twice
    d = np.sqrt(v_new) + eps
    theta_new = theta - lr * m_new / d
    theta_tol = 2 * 12 * U * (lr * m_mag / d + np.abs(theta))
    return (theta_new, m_new, v_new), (theta_tol, m_tol, v_tol)


def _within(got, want, tol, what):
    """``close_elementwise`` with a bound per element (``tol``)."""
    close_elementwise((got.astype(np.float64) - want) / np.where(tol > 0, tol, 1.0),
                      np.zeros_like(want), rtol=0.0, atol=1.0,
                      what=what + " (error in units of its bound)")
    exact = tol == 0
    assert np.array_equal(got.astype(np.float64)[exact], want[exact]), what


@pytest.mark.parametrize("carried", [False, True], ids=["from-zero", "carried"])
@pytest.mark.parametrize("scale", SCALES, ids=["scale-1", "scale-1/4", "scale-1/3"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_clip_step_elementwise(cuda_device, n, scale, carried):
    from scvae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n % 100003 + int(1000 * scale) + 7 * carried)
    theta = rng.normal(0.0, 0.5, n).astype(np.float32)
    g = _gradient(rng, n, scale)
    if carried:
        m = rng.normal(0.0, 0.1, n).astype(np.float32)
        v = rng.gamma(2.0, 0.01, n).astype(np.float32)
        zero = np.flatnonzero(g == 0)
        v[zero] = 0.0               # v exactly 0 under a zero gradient ...
        m[zero[::2]] = 0.0          # ... with and without a carried m
    else:
        m = np.zeros(n, dtype=np.float32)
        v = np.zeros(n, dtype=np.float32)
    lr_t = np.float32(1e-3 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
                      if carried else 3.1622776e-4)
    td, gd, md, vd = (_buffer(a, cuda_device) for a in (theta, g, m, v))
    _lib.check(lib.scvae_adam_clip_step(
        _ptr(td), _ptr(gd), _ptr(md), _ptr(vd), n, float(scale), float(lr_t),
        float(B1), float(B2), float(EPS), _stream()), "scvae_adam_clip_step")
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (td, md, vd)]
    for name, t in zip(("theta", "m", "v"), got):
        assert np.all(t[n:] == np.float32(CANARY)), name + ": canary"
    # the gradient is read only: its clipped value is never stored (the
    # data-parallel path reads the buffer after the update)
    assert np.array_equal(gd.cpu().numpy().view(np.uint32),
                          np.concatenate([g, np.full(PAD, CANARY, np.float32)])
                          .view(np.uint32)), "gradient buffer changed"
    want, tol = _reference(theta, g, m, v, scale, lr_t)
    for name, a, w, t in zip(("theta", "m", "v"), got, want, tol):
        assert np.isfinite(a[:n]).all(), name
        _within(a[:n], w, t, "{} n={} scale={}".format(name, n, scale))
    still = (g == 0) & (m == 0) & (v == 0)
    assert still.any() or n < 1023
    assert np.array_equal(got[0][:n][still].view(np.uint32),
                          theta[still].view(np.uint32)), "theta under g = m = v = 0"


def test_adam_clip_step_refuses_a_misaligned_pointer(cuda_device):
    """One float off a 16-byte boundary: the argument error, nothing launched
    (every buffer as it was), ``scvae_last_error`` names the condition."""
    from scvae_amd import _lib
    lib = _lib.load()
    n = 64
    rng = np.random.default_rng(0)
    host = [rng.normal(0, 1, n + PAD).astype(np.float32) for _ in range(4)]
    host[3] = np.abs(host[3])
    for which in range(4):
        dev = [torch.from_numpy(a).to(cuda_device) for a in host]
        ptrs = [t.data_ptr() for t in dev]
        assert all(p % 16 == 0 for p in ptrs)
        ptrs[which] += 4
        rc = lib.scvae_adam_clip_step(
            *[ctypes.c_void_p(p) for p in ptrs], n, 1.0, 1e-3, float(B1),
            float(B2), float(EPS), _stream())
        message = lib.scvae_last_error().decode("utf-8", "replace")
        torch.cuda.synchronize()
        assert rc == -1, (which, rc)
        assert "bad argument" in message and "% 16 == 0" in message, message
        for t, a in zip(dev, host):
            assert np.array_equal(t.cpu().numpy().view(np.uint32),
                                  a.view(np.uint32))


# ---- Engine.adam_step over six steps ------------------------------------------

F, L, H = 40, 3, (12,)
STEPS, LR = 6, 1e-3


def _engine(device):
    from scvae_amd.engine import Engine
    return Engine(F, L, H, "poisson", batch_norm=True, device=device, seed=3)


def _prescribed(eng):
    """|g| log-uniform in [1e-3, 5] with fixed signs; ``flip`` changes sign
    every step, ``zero`` is exactly 0 in every step (the alignment padding
    between the tensors of the flat buffer among it, as in a real step)."""
    n = eng.params.numel()
    padding = np.ones(n, dtype=bool)
    for offset, shape in eng.param_table.values():
        padding[offset:offset + int(np.prod(shape))] = False
    rng = np.random.default_rng(11)
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(5.0), n))
    g = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    idx = np.arange(n)
    zero = (idx % 7 == 3) | padding
    flip = (idx % 5 == 1) & ~zero
    g[zero] = 0.0
    return g, flip, zero


def _gradient_of_step(g, flip, t):
    out = g.copy()
    if t % 2 == 0:
        out[flip] = -out[flip]
    return out


def _named(flat, table):
    flat = torch.as_tensor(flat)
    return {k: flat[o:o + int(np.prod(s))].reshape(s).clone()
            for k, (o, s) in table.items()}


def _flat(named, table, n):
    out = torch.zeros(n, dtype=torch.float64)
    for k, (o, s) in table.items():
        out[o:o + int(np.prod(s))] = named[k].reshape(-1)
    return out


class _Oracle:
    """``om.clip_and_adam`` on the engine's fp32 start, the prescribed
    gradients pre-scaled in fp64 (the oracle has no ``grad_scale``)."""

    def __init__(self, eng, scale):
        self.table, self.n, self.scale = eng.param_table, eng.params.numel(), scale
        self.params = _named(eng.params.cpu().double(), self.table)
        self.state = om.adam_state(self.params)

    def step(self, g):
        grads = _named(torch.from_numpy(g.astype(np.float64) * self.scale),
                       self.table)
        self.params = om.clip_and_adam(self.params, grads, self.state, LR)

    def flat(self):
        return (_flat(self.params, self.table, self.n),
                _flat(self.state["m"], self.table, self.n),
                _flat(self.state["v"], self.table, self.n))


# The bound after t steps.  Every element's gradient keeps its magnitude (only
# signs change), scale 1 and 0.5 multiply exactly, and the moments start at
# zero, so with a = |clip(g * scale)|: |m_t| <= a and v_t <= a^2, both sums of
# terms no larger than that.  |g * scale| >= 5e-4 keeps sqrt(v) >= sqrt(1e-3)
# * 5e-4 = 1.6e-5 >> epsilon = 1e-8: nothing is ill-conditioned.
#
# The device's hyper-parameters are fp32, the oracle's fp64: fl(0.9) and
# fl(0.999) are within u/2 of theirs, but 1 - fl(beta), exact in fp32, is then
# off by E1 = 2.4e-7 (4 u) of 0.1 and by E2 = 1.29e-5 (216 u) of 0.001.  That
# is the number format's doing (tf.train.AdamOptimizer casts the same way), so
# it is part of the bound, computed here from the constants and not fitted.
#
#   m_t: a step multiplies the carried error by beta1 < 1 and adds at most
#     three roundings of magnitudes <= a (beta1 * m with beta1's own error,
#     (1 - beta1) * gc, the sum) and E1 * a:   |dm_t| <= t (3 u + E1) a
#   v_t: all terms positive, so errors stay relative: per step beta2 * v,
#     (1 - beta2) * gc, * gc and the sum (4 u), and E2 once in every term:
#                                               |dv_t| <= (4 t u + E2) v_t
#   q_t = lr_t m_t / (sqrt(v_t) + epsilon) = lr_t m_t / d_t: sqrt halves v's
#     error and rounds, + epsilon rounds: d_t by (2 t u + E2 / 2 + 2 u);
#     lr_t is cast to fp32, the product and the division round (3 u); m's
#     error is absolute.  With |q_t| <= lr_t a / d_t:
#       |dq_t| <= (lr_t a / d_t) ((2 t + 5) u + E2 / 2 + t (3 u + E1))
#   theta_t = theta_{t-1} - q_t rounds once, by at most u |theta_t|:
#       |dtheta_t| <= sum_{k <= t} (|dq_k| + u |theta_k|)
# Twice each, as everywhere in this file.
E1 = abs(np.float64(np.float32(1) - B1) - (1 - om.ADAM_BETA1)) / (1 - om.ADAM_BETA1)
E2 = abs(np.float64(np.float32(1) - B2) - (1 - om.ADAM_BETA2)) / (1 - om.ADAM_BETA2)
assert E1 < 5 * U and E2 < 220 * U


class _Bounds:
    def __init__(self, g, scale):
        self.a = np.minimum(np.abs(g.astype(np.float64) * scale), 1.0)
        self.theta = np.zeros_like(self.a)
        self.t = 0

    def step(self, theta, v):
        """After the oracle's step: its ``theta_t`` and ``v_t``."""
        self.t += 1
        t = self.t
        lr_t = (LR * np.sqrt(1.0 - om.ADAM_BETA2 ** t)
                / (1.0 - om.ADAM_BETA1 ** t))
        d = np.sqrt(v) + om.ADAM_EPSILON
        dq = (lr_t * self.a / d) * ((2 * t + 5) * U + E2 / 2 + t * (3 * U + E1))
        self.theta = self.theta + dq + U * np.abs(theta)
        self.m = t * (3 * U + E1) * self.a
        self.v = (4 * t * U + E2) * v

    def twice(self):
        return 2 * self.theta, 2 * self.m, 2 * self.v


def _tensor_rtol(tol, want, table):
    """The elementwise bounds as ONE relative bound for ``close_per_tensor``:
    the largest, over the tensors, of a tensor's largest elementwise bound
    against its largest magnitude."""
    worst = 0.0
    for offset, shape in table.values():
        n = int(np.prod(shape))
        scale = np.abs(want[offset:offset + n]).max()
        assert scale > 0
        worst = max(worst, tol[offset:offset + n].max() / scale)
    return worst


def _hold(eng, oracle, bounds, live, zero, theta0):
    torch.cuda.synchronize()
    t = bounds.t
    want = [a.numpy() for a in oracle.flat()]
    got = [a.cpu().double().numpy() for a in (eng.params, eng.adam_m, eng.adam_v)]
    for name, a, w, b in zip(("params", "adam_m", "adam_v"), got, want,
                             bounds.twice()):
        what = "step {} {}".format(t, name)
        rtol = _tensor_rtol(b, w, eng.param_table)
        assert rtol < 1e-3, (what, rtol)    # (sanity: the bounds stay tight)
        close_per_tensor(a, w, eng.param_table, rtol=rtol, atol=0.0, what=what)
        _within(a[live], w[live], b[live], what)
    assert np.array_equal(eng.params.cpu().numpy()[zero].view(np.uint32),
                          theta0[zero].view(np.uint32)), "theta of the zero subset"
    assert not got[1][zero].any() and not got[2][zero].any()


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_six_adam_steps_against_the_oracle(cuda_device, scale):
    eng = _engine(cuda_device)
    n = eng.params.numel()
    g, flip, zero = _prescribed(eng)
    live = ~zero
    assert (np.abs(g[live]) * scale >= 5e-4).all()
    assert (np.abs(g) * scale > 1).sum() > n // 20          # some are clipped
    assert flip.sum() > n // 10 and zero.sum() > n // 10
    theta0 = eng.params.cpu().numpy().copy()
    oracle = _Oracle(eng, scale)
    bounds = _Bounds(g, scale)
    twin = state = None
    for t in range(1, STEPS + 1):
        gt = _gradient_of_step(g, flip, t)
        eng.grads.copy_(torch.from_numpy(gt))
        eng.adam_step(LR, grad_scale=scale)
        oracle.step(gt)
        theta, _, v = oracle.flat()
        bounds.step(theta.numpy(), v.numpy())
        _hold(eng, oracle, bounds, live, zero, theta0)
        if twin is not None:
            twin.grads.copy_(torch.from_numpy(gt))
            twin.adam_step(LR, grad_scale=scale)
        if t == 3:
            # a checkpoint into a second engine (another seed: every buffer
            # and the step count must come from the state)
            state = eng.state_dict()
            from scvae_amd.engine import Engine
            twin = Engine(F, L, H, "poisson", batch_norm=True,
                          device=cuda_device, seed=99)
            twin.load_state_dict(state)
            assert twin.adam_t == 3
    assert eng.adam_t == STEPS and twin.adam_t == STEPS
    torch.cuda.synchronize()
    for a, b in ((eng.params, twin.params), (eng.adam_m, twin.adam_m),
                 (eng.adam_v, twin.adam_v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _hold(twin, oracle, bounds, live, zero, theta0)


def test_initialise_restarts_the_step_count(cuda_device):
    """``Engine.initialise`` zeroes the moments and ``adam_t``: the next update
    is step 1 again (``lr_t`` of t = 1), held to the oracle from a fresh
    state."""
    eng = _engine(cuda_device)
    g, flip, zero = _prescribed(eng)
    for t in range(1, 4):
        eng.grads.copy_(torch.from_numpy(_gradient_of_step(g, flip, t)))
        eng.adam_step(LR)
    assert eng.adam_t == 3
    eng.initialise(seed=3)
    assert eng.adam_t == 0
    assert not eng.adam_m.any().item() and not eng.adam_v.any().item()
    theta0 = eng.params.cpu().numpy().copy()
    oracle = _Oracle(eng, 1.0)
    bounds = _Bounds(g, 1.0)
    for t in range(1, 3):
        gt = _gradient_of_step(g, flip, t)
        eng.grads.copy_(torch.from_numpy(gt))
        eng.adam_step(LR)
        oracle.step(gt)
        theta, _, v = oracle.flat()
        bounds.step(theta.numpy(), v.numpy())
        _hold(eng, oracle, bounds, ~zero, zero, theta0)
    assert eng.adam_t == 2
