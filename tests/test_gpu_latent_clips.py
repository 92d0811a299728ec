"""The posterior's log-sigma clip, on purpose, on every chain.

``log_sigma = clamp(pre, -3, 3)`` with a zero gradient outside the interval
(oracle/models.py, ``vae_forward``; va:2346-2369) is written several times: in
the launch chain's ``gauss_latent_fwd_kernel`` / ``gauss_latent_bwd_kernel``
(elementwise.hip), in the mid chain (midchain.hip), in the tile chain's
resident launches and in the one-launch evaluation pass (tilechain.hip; the
tile chain's ordinary launches use the launch chain's kernels for this stage).
The step-level cases put unit 0 of the LOG_SIGMA head above
the interval and unit 1 below it for every cell, and units 2 and 3 across its
upper and lower end, with every pre-activation at least 1e-3 away from +-3:
two orders above the fp32 error of a value of size 3 behind two batch-norm
layers, so that no cell's gate can legitimately fall on either side.  The
stand-alone cases call ``scvae_gauss_latent_fwd`` directly.

The clip of the mean at +-FLOAT32_MAX_HALF needs activations of overflow
scale, which no step produces; its twin in the mixture's softplus-Gaussian
pair is held stand-alone, with +-2e38 and +-inf pre-activations and the zeroed
gradients, by ``test_pair_clip`` in tests/test_gpu_mixture_stage.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import models as om
from _parity import (LL_ATOL, LL_RTOL, close_elementwise, close_per_tensor,
                     close_scalar)

pytestmark = pytest.mark.gpu

F, H = 96, (20, 16)
NB = "negative binomial"
WARM_UP = 0.7
CLEAR = 1e-3            # every pre-activation at least this far from +-3
LS_W, LS_B = "POSTERIOR/LOG_SIGMA/DENSE/weights", "POSTERIOR/LOG_SIGMA/DENSE/biases"


def _counts(rng, cells, features):
    lam = rng.gamma(0.6, 3.0, size=(1, features))
    x = rng.poisson(lam, size=(cells, features)).astype(np.float64)
    x *= rng.random((cells, features)) > 0.6
    x[0, 0] += 40.0
    return torch.from_numpy(x)


def _f32(t):
    return t.float().double()


def _config(L, n_iw, n_mc, analytical):
    return om.ModelConfig(feature_size=F, latent_size=L, hidden_sizes=H,
                          likelihood=NB, n_iw=n_iw, n_mc=n_mc,
                          analytical_kl_term=analytical)


def _log_sigma_pre(cfg, params, moving, x, training):
    """The LOG_SIGMA head's pre-activations [B, L] BEFORE the clamp (the
    encoder of ``om.vae_forward``)."""
    h = _encoder(params, moving, x, training)
    return om.dense_layer(h, params, "POSTERIOR/LOG_SIGMA", False, training,
                          moving, None, activation=False)


def _encoder(params, moving, x, training, statistics=None):
    """The last encoder layer's activations (``om.vae_forward``'s encoder);
    ``statistics``: filled with the batch mean and variance of every layer."""
    h = x
    for i in range(len(H)):
        scope = "ENCODER/{}".format(i + 1)
        if statistics is not None:
            a = h @ params[scope + "/DENSE/weights"] + params[scope + "/DENSE/biases"]
            statistics[scope] = (a.mean(dim=0), a.var(dim=0, unbiased=False))
        h = om.dense_layer(h, params, scope, True, training, moving, None)
    return h


def _straddle(train, evaluation, target):
    """The bias that puts ``target`` into a gap of ``train + bias`` between its
    30th and 70th percentile (and between the 25th and 75th of ``evaluation +
    bias``), as far from every value of both as possible."""
    v = torch.sort(train).values
    n = v.numel()
    best, best_gap = None, -1.0
    for i in range(int(0.3 * n), int(0.7 * n)):
        bias = target - 0.5 * (v[i] + v[i + 1])
        if not 0.25 <= (evaluation + bias > target).double().mean() <= 0.75:
            continue
        gap = min((train + bias - target).abs().min().item(),
                  (evaluation + bias - target).abs().min().item())
        if gap > best_gap:
            best, best_gap = bias, gap
    return best


def _state(L, B, S):
    """Parameters, moving statistics, minibatch and noise on the host, as the
    fp32 values the device will hold: the usual small random parameters, and
    the LOG_SIGMA head's unit 0 near +6 and unit 1 near -6 for every cell,
    units 2 and 3 spread across +3 and -3, the other units well inside."""
    cfg = _config(L, 1, 1, True)
    shapes = om.vae_parameter_shapes(cfg)
    g = torch.Generator().manual_seed(1)
    params = om.init_parameters(shapes, 0)
    for name, p in params.items():
        if not name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
    rng = np.random.default_rng(1000 * B + S)
    x = _counts(rng, B, F)
    eps = _f32(torch.from_numpy(rng.standard_normal((S, B, L))))
    # moving statistics of a model that has seen such minibatches: the
    # encoder's within a few percent of this one's, the decoder's arbitrary
    moving = om.init_moving_statistics(shapes)
    for name, m in moving.items():
        if name.endswith("moving_mean"):
            m.copy_(torch.randn(m.shape, generator=g, dtype=torch.float64) * 0.2)
        else:
            m.copy_(torch.rand(m.shape, generator=g, dtype=torch.float64) + 0.5)
    statistics = {}
    _encoder(params, moving, x, True, statistics)
    for scope, (mean, var) in statistics.items():
        moving[scope + "/BATCH_NORM/moving_mean"] += mean
        moving[scope + "/BATCH_NORM/moving_variance"] *= var
        moving[scope + "/BATCH_NORM/moving_variance"] += 0.05
    W, b = params[LS_W], params[LS_B]
    W[:, :2] *= 0.25
    W[:, 2:4] *= 2.0
    W[:, 4:] *= 0.5
    b[0], b[1] = 6.0, -6.0
    params = {k: _f32(v) for k, v in params.items()}
    moving = {k: _f32(v) for k, v in moving.items()}
    h = [_encoder(params, moving, x, training) for training in (True, False)]
    for unit, target in ((2, 3.0), (3, -3.0)):
        w = params[LS_W][:, unit]
        params[LS_B][unit] = _f32(_straddle(h[0] @ w, h[1] @ w, target))
    return params, moving, x, eps


def _conditions(pre):
    """What the fixture must give (asserted on the oracle's fp64
    pre-activations, so that a change of the fixture cannot slide a value onto
    a boundary unnoticed): the failure text, or None."""
    away = (pre.abs() - 3.0).abs().min().item()
    if away < CLEAR:
        return "a pre-activation {:.2e} from a clip boundary".format(away)
    if not (pre[:, 0] > 3).all() or not (pre[:, 1] < -3).all():
        return "units 0 / 1 not clipped for every cell"
    for unit, side in ((2, pre[:, 2] > 3), (3, pre[:, 3] < -3)):
        share = side.double().mean().item()
        if not 0.2 <= share <= 0.8:
            return "unit {}: {:.2f} of the cells clipped".format(unit, share)
    return None


@functools.lru_cache(maxsize=None)
def _reference(L, B, n_iw, n_mc, analytical):
    """The fixture and the oracle's training and evaluation step on it (one
    per shape: the paths of a shape share it and leave it unchanged)."""
    S = n_iw * n_mc
    cfg = _config(L, n_iw, n_mc, analytical)
    params, moving, x, eps = _state(L, B, S)
    for training in (True, False):
        bad = _conditions(_log_sigma_pre(cfg, params, moving, x, training))
        assert bad is None, (bad, "training" if training else "evaluation")
    _, _, out, grads = om.vae_train_step(
        cfg, dict(params), moving, om.adam_state(params), x, x, eps, 1e-4,
        warm_up_weight=WARM_UP)
    ev = om.vae_forward(cfg, params, moving, x, x, eps, False)
    return cfg, params, moving, x, eps, out, grads, ev


def _bn_bias(name):
    return name.endswith("DENSE/biases") and (
        "ENCODER/" in name or "DECODER/" in name)


def _hold_outputs(tag, sc, ll, klz, qz, out):
    sc = sc.cpu().double()
    assert torch.isfinite(sc[:4]).all(), tag
    for i, n in enumerate(("lower_bound", "lower_bound_weighted",
                           "reconstruction_error", "kl_divergence")):
        close_scalar(sc[i], out[n], what="{} {}".format(tag, n))
    # (the bounds of test_gpu_chain_paths.py for the same outputs)
    close_elementwise(ll, out["log_p_x_given_z"].reshape(-1), rtol=LL_RTOL,
                      atol=LL_ATOL, what=tag + " per-cell log-likelihood")
    close_elementwise(klz, out["kl_divergence_neurons"], rtol=1e-4, atol=1e-6,
                      what=tag + " kl_neurons")
    close_elementwise(qz, out["q_z_mean"], rtol=1e-4, atol=1e-5,
                      what=tag + " q_z_mean")


# (L, B, path).  B = 29 runs the mid chain (midchain.hip's copy of the clamp).
# B = 192 runs the tile chain, whose latent stage is the launch chain's kernel
# unless the pass is recorded into resident launches ("resident":
# ``set_tile_resident``), which run tilechain.hip's own copy.  "launch": both
# chains switched off, which leaves the kernels of elementwise.hip.  L = 70
# makes gauss_latent_fwd_kernel reduce across two waves.  The evaluation step of
# every B = 192 case with one sample per cell runs eval_mlp_kernel
# (tilechain.hip), a fourth, forward-only copy.
SHAPES = [(6, 29, "mid"), (6, 29, "launch"), (6, 192, "tile"),
          (6, 192, "resident"), (6, 192, "launch"), (70, 29, "launch")]


@pytest.mark.parametrize("analytical", [True, False], ids=["analytic-kl", "mc-kl"])
@pytest.mark.parametrize("n_iw,n_mc", [(1, 1), (2, 2)])
@pytest.mark.parametrize("L,B,path", SHAPES)
def test_step_with_clipped_log_sigma(cuda_device, L, B, path, n_iw, n_mc,
                                     analytical):
    from scvae_amd.engine import Engine
    S = n_iw * n_mc
    cfg, params, moving, x, eps, out, grads, ev = _reference(
        L, B, n_iw, n_mc, analytical)
    eng = Engine(F, L, H, NB, batch_norm=True, device=cuda_device, seed=0,
                 analytical_kl_term=analytical)
    assert list(eng.param_table) == list(params)
    eng.load_parameters(params, moving)
    if path == "launch":
        eng.set_mid_chain(False)
        eng.set_tile_chain(False)
    if path == "resident":
        eng.set_tile_resident(True)
    eng.reserve(B, S)
    # the Monte-Carlo KL has no chain kernels: every such step is a launch-chain
    # step, whatever its shape
    taken = path if analytical else "launch"
    assert eng.uses_mid_chain(B, S) == (taken == "mid")
    assert eng.uses_mid_chain(B, S, training=False) == (taken == "mid")
    assert eng.uses_tile_chain(B, S) == (taken in ("tile", "resident"))
    assert eng.uses_tile_resident(B, S) == (taken == "resident")
    for name, p in eng.named_parameters().items():
        assert torch.equal(p.cpu().double(), params[name]), name

    xd, ed = x.float().to(cuda_device), eps.float().to(cuda_device)
    moving0 = eng.moving.clone()
    ll = torch.zeros(S * B, device=cuda_device)
    klz = torch.zeros(L, device=cuda_device)
    qz = torch.zeros(B, L, device=cuda_device)
    outs = {"log_p_x_given_z": ll, "kl_neurons": klz, "q_z_mean": qz}
    sc = eng.step(xd, xd, eps=ed, training=True, n_iw=n_iw, n_mc=n_mc,
                  warm_up_weight=WARM_UP, outputs=outs).clone()
    torch.cuda.synchronize()
    _hold_outputs("train", sc, ll, klz, qz, out)

    got = {k: v.cpu().double() for k, v in eng.named_gradients().items()}
    table = {k: v for k, v in eng.param_table.items() if not _bn_bias(k)}
    want_flat = torch.zeros(eng.grads.numel(), dtype=torch.float64)
    for name, (offset, shape) in table.items():
        want_flat[offset:offset + grads[name].numel()] = grads[name].reshape(-1)
    # 2e-4 of each tensor's own largest magnitude: test_gpu_chain_paths.py's
    # bound for the gradients of these paths
    close_per_tensor(eng.grads, want_flat, table, rtol=2e-4, atol=0.0,
                     what="grad")
    for name in eng.param_table:
        if _bn_bias(name):      # (cancelled by the batch norm: exactly zero)
            assert got[name].abs().max().item() == 0.0, name
    # clipped for every cell: the clamp passes no gradient, exactly
    for unit in (0, 1):
        assert (grads[LS_B][unit] == 0.0) and (grads[LS_W][:, unit] == 0.0).all()
        assert got[LS_B][unit].item() == 0.0, "LOG_SIGMA bias {}".format(unit)
        assert (got[LS_W][:, unit] == 0.0).all(), "LOG_SIGMA column {}".format(unit)
    # clipped for some cells: bias and weight column of the unit, element by
    # element.  Each is a sum over the SAME unclipped cells of d log_sigma times
    # an activation of order one, so its rounding error scales with the
    # column's magnitude (a single element may cancel): 2e-4, the bound above,
    # of the column's own largest element instead of the tensor's, whose scale
    # the never-clipped units set
    for unit in (2, 3):
        want = torch.cat([grads[LS_B][unit:unit + 1], grads[LS_W][:, unit]])
        have = torch.cat([got[LS_B][unit:unit + 1], got[LS_W][:, unit]])
        assert want.abs().max() > 0
        close_elementwise(have, want, rtol=0.0,
                          atol=2e-4 * want.abs().max().item(),
                          what="LOG_SIGMA unit {}".format(unit))

    eng.moving.copy_(moving0)
    ll.zero_()
    klz.zero_()
    qz.zero_()
    sc = eng.step(xd, xd, eps=ed, training=False, n_iw=n_iw, n_mc=n_mc,
                  outputs=outs).clone()
    torch.cuda.synchronize()
    _hold_outputs("evaluation", sc, ll, klz, qz, ev)


# ---- scvae_gauss_latent_fwd on its own --------------------------------------------

# sigma = __expf(clamp(ls)): the fast exponential's error on [-3, 3] is not
# derivable from the code, so these two bounds are MEASURED: the largest
# elementwise error of all the cases below on an MI355X (gfx950) against fp64,
#   z       relative to |mu| + sigma |eps|          observed 2.68e-7
#   kl_elem relative to (mu^2 + sigma^2 + 1)/2 + |ls| (the magnitudes of the
#           KL term's own terms; the term itself cancels to 0 at the prior)
#                                                   observed 5.76e-7
# (kl_cell, relative to the row's summed magnitudes: 3.1e-7; the unit-variance
# posterior, which has no exponential: 6.0e-8, 5.1e-8 and 9.5e-8), times a
# margin of 4 for draws not seen.  An error above 1e-5 would be a defect of
# the kernel, never a bound to adopt.
Z_OBSERVED, KL_OBSERVED, MARGIN = 2.7e-7, 5.8e-7, 4.0
# kl_cell: the row sum of kl_elem over L <= 1000 in fp32: a butterfly over 64
# lanes (6 roundings) and up to 16 waves in sequence (16): 22 u of the summed
# magnitudes on top of the elements' own bound
ROW_SUM_ROUNDINGS = 22
U = 2.0 ** -24


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("mode", ["sampled", "unit-variance", "deterministic"])
@pytest.mark.parametrize("cells", [1, 37])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("L", [1, 6, 64, 65, 130, 1000])
def test_gauss_latent_fwd_against_fp64(cuda_device, L, S, cells, mode):
    from scvae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(L * 100 + S * 10 + cells)
    mu = rng.normal(0.0, 1.5, (cells, L)).astype(np.float32)
    ls = rng.normal(0.0, 1.5, (cells, L))
    ls = np.clip(ls, -3.0 + CLEAR, 3.0 - CLEAR)
    # a fixed third outside [-3, 3], alternately above and below, clear of it
    flat = ls.reshape(-1)
    third = np.arange(0, flat.size, 3)
    flat[third] = (3.0 + CLEAR + np.abs(rng.normal(0.0, 2.0, third.size))) * (
        1 - 2 * (third // 3 % 2))
    ls = ls.astype(np.float32)
    assert np.abs(np.abs(ls.astype(np.float64)) - 3.0).min() >= CLEAR * 0.99
    eps = rng.standard_normal((S, cells, L)).astype(np.float32)
    deterministic = mode == "deterministic"
    unit = mode == "unit-variance"

    dev = cuda_device
    mud = torch.from_numpy(mu).to(dev)
    lsd = None if unit else torch.from_numpy(ls).to(dev)
    epsd = None if deterministic else torch.from_numpy(eps).to(dev)
    rows = 1 if deterministic else S
    z = torch.full((rows, cells, L), float("nan"), device=dev)
    kl_elem = torch.full((cells, L), float("nan"), device=dev)
    kl_cell = torch.full((cells,), float("nan"), device=dev)
    _lib.check(lib.scvae_gauss_latent_fwd(
        _p(mud), _p(lsd), _p(epsd), _p(z), _p(kl_elem), _p(kl_cell), S, cells,
        L, 1 if deterministic else 0,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
        "scvae_gauss_latent_fwd")
    torch.cuda.synchronize()

    # oracle/models.py, vae_forward: the clamps, sigma, z, the analytic KL
    m64 = np.clip(mu.astype(np.float64), -om.FLOAT32_MAX_HALF, om.FLOAT32_MAX_HALF)
    l64 = np.zeros_like(m64) if unit else np.clip(ls.astype(np.float64), -3.0, 3.0)
    sigma = np.exp(l64)
    e64 = np.zeros((1, cells, L)) if deterministic else eps.astype(np.float64)
    want_z = m64[None] + sigma[None] * e64
    want_kl = 0.5 * (m64 * m64 + sigma * sigma - 1.0) - l64
    z_mag = np.abs(m64)[None] + sigma[None] * np.abs(e64)
    kl_mag = 0.5 * (m64 * m64 + sigma * sigma + 1.0) + np.abs(l64)

    got_z = z.cpu().double().numpy()
    got_kl = kl_elem.cpu().double().numpy()
    got_cell = kl_cell.cpu().double().numpy()
    assert np.isfinite(got_z).all() and np.isfinite(got_kl).all()
    z_err = (np.abs(got_z - want_z) / z_mag).max()
    kl_err = (np.abs(got_kl - want_kl) / kl_mag).max()
    cell_err = (np.abs(got_cell - want_kl.sum(axis=1)) / kl_mag.sum(axis=1)).max()
    print("gauss_latent_fwd L={} S={} cells={} {}: z {:.3e} kl_elem {:.3e} "
          "kl_cell {:.3e}".format(L, S, cells, mode, z_err, kl_err, cell_err))
    assert max(z_err, kl_err, cell_err) <= 1e-5, "a finding, not a bound"
    z_tol, kl_tol = MARGIN * Z_OBSERVED, MARGIN * KL_OBSERVED
    _scaled = lambda got, want, mag, tol, what: close_elementwise(  # noqa: E731
        (got - want) / mag, np.zeros_like(want), rtol=0.0, atol=tol, what=what)
    _scaled(got_z, want_z, z_mag, z_tol, "z")
    _scaled(got_kl, want_kl, kl_mag, kl_tol, "kl_elem")
    _scaled(got_cell, want_kl.sum(axis=1), kl_mag.sum(axis=1),
            kl_tol + ROW_SUM_ROUNDINGS * U, "kl_cell")
