"""The hidden-layer chains of a step against the fp64 oracle, per tensor.

A step runs its hidden layers, posterior heads and latent stage on one of
three paths, picked by the plan from the step's shape:

    mid chain     two cooperative launches, 16 workgroups, a grid barrier per
                  layer (midchain.hip): VAE, B*S <= 128, widths and L <= 128
    tile chain    64-row tiles, one launch per layer and direction
                  (tilechain.hip): training, B*S > 128, widths and L <= 128;
                  GMVAE with whole tiles per pass; opt-in: one resident
                  launch per direction
    launch chain  gemm.hip / elementwise.hip: everything else

Every case asserts which path it took (``Engine.uses_mid_chain`` /
``uses_tile_chain`` / ``uses_tile_resident``), holds the step to the oracle
(``oracle/models.py``: va:2219-2770, gm:2788-3470) with the bounds of
test_gpu_baseline_configs.py -- each gradient and each moving statistic on its
own, relative to its own magnitude -- and then runs the same inputs on the
launch chain: the chain's error against fp64 may not exceed twice the launch
chain's plus a floor (``_differential``).  The shapes sit on the chains' index
edges: partial 8-column strips, odd k-split lengths, idle workgroups at the
barriers, ragged 64-row tails, encoder rows B against decoder rows B*S, the
row / width / depth limits on both sides.
"""
import numpy as np
import pytest
import torch

from oracle import models as om
from _parity import (LL_ATOL, LL_RTOL, close_elementwise, close_maxnorm,
                     close_scalar)

pytestmark = pytest.mark.gpu

WARM_UP = 0.7
NB, ZINB = "negative binomial", "zero-inflated negative binomial"
P, ZIP = "poisson", "zero-inflated poisson"

# The differential bound: err(chain) <= FACTOR * err(launch) + FLOOR * scale,
# errors being max |device - fp64| of one tensor and scale its max |fp64|.
# Both paths run the same fp32 input-layer product and likelihood heads -- the
# larger share of either error -- and differ only in the order of the fp32
# sums over <= 128 widths and the minibatch rows in between, which moves a
# result by a few fp32 ulps (2^-24 ~ 6e-8) of the tensor's scale, far below
# FLOOR = 4e-6 (64 ulps).  The launch chain's own error, 1e-7..1e-5 of the
# scale at these shapes, is the error fp32 makes here; FACTOR = 2 lets the
# chain make it in another order.  The decoder gradient's fp32 atomics (the
# plan's default) vary the last bits of both from run to run, also within the
# floor.  An index or weighting defect in a strip, tile or tail shows as an
# error the launch chain does not make, from about 1e-5 of the scale upwards.
FACTOR, FLOOR = 2.0, 4e-6


def _counts(rng, cells, features):
    lam = rng.gamma(0.6, 3.0, size=(1, features))
    x = rng.poisson(lam, size=(cells, features)).astype(np.float64)
    x *= rng.random((cells, features)) > 0.6
    x[0, 0] += 40.0
    return torch.from_numpy(x)


def _perturb(engine, seed):
    """Biases / beta away from zero, moving statistics away from (0, 1), as
    test_gpu_baseline_configs.py does."""
    g = torch.Generator().manual_seed(seed)
    for name, p in engine.named_parameters().items():
        if not name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    for name, m in engine.named_moving_statistics().items():
        if name.endswith("moving_mean"):
            m.copy_(torch.randn(m.shape, generator=g) * 0.2)
        else:
            m.copy_(torch.rand(m.shape, generator=g) + 0.5)


def _host(named):
    return {k: v.detach().cpu().double() for k, v in named.items()}


def _bn_bias(name):
    return name.endswith("DENSE/biases") and (
        "ENCODER/" in name or "DECODER/" in name or "LAYER_" in name)


def _grad_kind(name, shape):
    """The weights of a batch-normalised unit with ONE input (the first
    decoder layer at L = 1) are scale-invariant but for the batch norm's
    epsilon (1e-3): their gradient is that epsilon's term alone, a difference
    of terms ~1e2 larger, so it carries ~1e2 x fp32's relative rounding on any
    path.  It is held to the launch chain's error (``_differential``) rather
    than to 2e-4 of its own magnitude."""
    if _bn_bias(name):
        return "bn_bias"
    if (name.endswith("DENSE/weights") and len(shape) == 2 and shape[0] == 1
            and ("ENCODER/" in name or "DECODER/" in name)):
        return "grad_eps"
    return "grad"


# ---- one quantity = (device tensor, fp64 tensor, kind) ----------------------

def _check(name, got, want, kind):
    if kind == "scalar":
        close_scalar(got, want, what=name)
    elif kind == "ll":
        close_elementwise(got, want, rtol=LL_RTOL, atol=LL_ATOL, what=name)
    elif kind == "kl":
        close_elementwise(got, want, rtol=1e-4, atol=1e-6, what=name)
    elif kind == "qz":
        close_elementwise(got, want, rtol=1e-4, atol=1e-5, what=name)
    elif kind == "bn_bias":
        assert got.abs().max().item() == 0.0, name
    elif kind == "grad_eps":
        pass                            # (the differential only: _grad_kind)
    elif kind.startswith("grad"):       # "grad" or "grad:<rtol>"
        rtol = float(kind[5:]) if ":" in kind else 2e-4
        close_maxnorm(got, want, rtol=rtol, what=name)
    elif kind.startswith("moving"):
        rtol = float(kind[7:]) if ":" in kind else 1e-5
        close_elementwise(got, want, rtol=rtol, atol=1e-7, what=name)
    else:
        raise ValueError(kind)


def _hold_to_oracle(quantities):
    for name, (got, want, kind) in quantities.items():
        _check(name, got, want, kind)


def _error(got, want):
    got = torch.as_tensor(got, dtype=torch.float64).reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    return ((got - want).abs().max().item(), want.abs().max().item())


def _differential(chain, launch, label):
    """Per tensor: the chain's error against fp64 within FACTOR x the launch
    chain's + FLOOR x the tensor's scale.  Returns the worst use of the bound."""
    assert list(chain) == list(launch)
    worst, where = 0.0, None
    for name, (got, want, kind) in chain.items():
        if kind == "bn_bias":           # (exactly zero on both paths)
            continue
        err_chain, scale = _error(got, want)
        err_launch, _ = _error(launch[name][0], want)
        bound = FACTOR * err_launch + FLOOR * scale
        assert err_chain <= bound, (
            "{} {}: chain error {:.3e}, launch chain {:.3e}, scale {:.3e}"
            .format(label, name, err_chain, err_launch, scale))
        if bound > 0 and err_chain / bound > worst:
            worst, where = err_chain / bound, name
    print("{}: worst {:.2f} of the differential bound ({})".format(
        label, worst, where))
    return worst


# ---- VAE ----------------------------------------------------------------------

def _vae_engine(dev, F, L, H, likelihood, seed):
    from scvae_amd.engine import Engine
    eng = Engine(F, L, H, likelihood, batch_norm=True, device=dev, seed=seed)
    _perturb(eng, seed + 1)
    return eng


def _vae_quantities(eng, dev, cfg, params, moving, x, eps, n_iw, n_mc,
                    evaluate, oracle=None):
    """Run the training step (and with ``evaluate`` an evaluation step with
    the drawn z and one with the deterministic z, at the moving statistics the
    training step started from) and pair every output with the oracle's."""
    B, L = x.shape[0], cfg.latent_size
    S = n_iw * n_mc
    xd = x.float().to(dev)
    ed = eps.float().to(dev)
    if oracle is None:
        oracle = {}
        _, new_moving, out, grads = om.vae_train_step(
            cfg, dict(params), moving, om.adam_state(params), x, x, eps,
            1e-4, warm_up_weight=WARM_UP)
        oracle["train"] = (out, grads, new_moving)
        if evaluate:
            oracle["eval"] = om.vae_forward(cfg, params, moving, x, x, eps,
                                            False)
            oracle["det"] = om.vae_forward(cfg, params, moving, x, x, None,
                                           False, deterministic_z=True)
    moving0 = eng.moving.clone()
    ll = torch.zeros(S * B, device=dev)
    klz = torch.zeros(L, device=dev)
    qz = torch.zeros(B, L, device=dev)
    outs = {"log_p_x_given_z": ll, "kl_neurons": klz, "q_z_mean": qz}
    sc = eng.step(xd, xd, eps=ed, training=True, n_iw=n_iw, n_mc=n_mc,
                  warm_up_weight=WARM_UP, outputs=outs).clone()
    torch.cuda.synchronize()
    out, grads, new_moving = oracle["train"]
    q = {}
    names = ("lower_bound", "lower_bound_weighted", "reconstruction_error",
             "kl_divergence")
    sc = sc.cpu().double()
    assert torch.isfinite(sc[:4]).all()
    for i, n in enumerate(names):
        q["train " + n] = (sc[i], out[n], "scalar")
    q["train log_p_x_given_z"] = (ll.cpu().double(),
                                  out["log_p_x_given_z"].reshape(-1), "ll")
    q["train kl_neurons"] = (klz.cpu().double(), out["kl_divergence_neurons"],
                             "kl")
    q["train q_z_mean"] = (qz.cpu().double(), out["q_z_mean"], "qz")
    for name, g in _host(eng.named_gradients()).items():
        q["grad " + name] = (g, grads[name], _grad_kind(name, g.shape))
    for name, m in _host(eng.named_moving_statistics()).items():
        q["moving " + name] = (m, new_moving[name], "moving")
    if not evaluate:
        return q, oracle
    for tag, det in (("eval", False), ("det", True)):
        eng.moving.copy_(moving0)
        rows = B if det else S * B
        ll = torch.zeros(rows, device=dev)
        klz.zero_()
        qz.zero_()
        outs = {"log_p_x_given_z": ll, "kl_neurons": klz, "q_z_mean": qz}
        if det:
            sc = eng.step(xd, xd, training=False, deterministic_z=True,
                          outputs=outs).clone()
        else:
            sc = eng.step(xd, xd, eps=ed, training=False, n_iw=n_iw,
                          n_mc=n_mc, outputs=outs).clone()
        torch.cuda.synchronize()
        out = oracle[tag]
        sc = sc.cpu().double()
        for i, n in enumerate(names):
            q[tag + " " + n] = (sc[i], out[n], "scalar")
        q[tag + " log_p_x_given_z"] = (
            ll.cpu().double(), out["log_p_x_given_z"].reshape(-1), "ll")
        q[tag + " kl_neurons"] = (klz.cpu().double(),
                                  out["kl_divergence_neurons"], "kl")
        q[tag + " q_z_mean"] = (qz.cpu().double(), out["q_z_mean"], "qz")
    return q, oracle


def _vae_case(dev, F, L, H, likelihood, B, n_iw=1, n_mc=1, path="mid",
              resident=False, resident_taken=None, seed=0):
    """``path``: "mid", "tile" or "launch" -- the path the plan must take;
    "mid" and "tile" are then compared with the launch chain as well.
    ``resident``: the tile chain's resident launches switched on;
    ``resident_taken``: whether the step must take them (default: as on)."""
    if resident_taken is None:
        resident_taken = resident
    S = n_iw * n_mc
    H = tuple(H)
    rng = np.random.default_rng(seed + 1000 * B + S)
    x = _counts(rng, B, F)
    eps = torch.from_numpy(rng.standard_normal((S, B, L)))
    cfg = om.ModelConfig(feature_size=F, latent_size=L, hidden_sizes=H,
                         likelihood=likelihood, n_iw=n_iw, n_mc=n_mc)
    evaluate = path == "mid"

    eng = _vae_engine(dev, F, L, H, likelihood, seed)
    if resident:
        eng.set_tile_resident(True)
    eng.reserve(B, S)
    params, moving = _host(eng.named_parameters()), _host(
        eng.named_moving_statistics())
    assert list(params) == list(om.vae_parameter_shapes(cfg))
    assert eng.uses_mid_chain(B, S) == (path == "mid")
    assert eng.uses_mid_chain(B, S, training=False) == (path == "mid")
    assert eng.uses_tile_chain(B, S) == (path == "tile")
    assert eng.uses_tile_resident(B, S) == (path == "tile" and resident_taken)
    if evaluate:
        assert eng.uses_mid_chain(B, 1, training=False)   # (deterministic z)
    chain, oracle = _vae_quantities(eng, dev, cfg, params, moving, x, eps,
                                    n_iw, n_mc, evaluate)
    _hold_to_oracle(chain)
    if path == "launch":
        return None
    del eng

    ref = _vae_engine(dev, F, L, H, likelihood, seed)
    if path == "mid":
        ref.set_mid_chain(False)
    else:
        ref.set_tile_chain(False)
    ref.reserve(B, S)
    for name, p in _host(ref.named_parameters()).items():
        assert torch.equal(p, params[name]), name      # (the same state)
    assert not ref.uses_mid_chain(B, S) and not ref.uses_tile_chain(B, S)
    assert not ref.uses_mid_chain(B, S, training=False)
    launch, _ = _vae_quantities(ref, dev, cfg, params, moving, x, eps,
                                n_iw, n_mc, evaluate, oracle)
    _hold_to_oracle(launch)
    return _differential(chain, launch, "{} B={} S={} H={} L={} {}".format(
        path + (" resident" if resident else ""), B, S, H, L, likelihood))


# (F, L, H, likelihood, B, n_iw, n_mc)
MID_CASES = {
    # `scvae train` with no options: cfg1's 100 genes, H = [100], L = 2, Poisson
    "reference-default": (100, 2, (100,), P, 100, 1, 1),
    # B*S = 128 exactly, three ways, and the smallest minibatch
    "rows-128x1": (200, 10, (64, 32), NB, 128, 1, 1),
    "rows-32x2x2": (200, 6, (50,), ZINB, 32, 2, 2),
    "rows-64x2": (200, 9, (40, 40), ZIP, 64, 2, 1),
    "rows-2": (150, 3, (16,), P, 2, 1, 1),
    # strip edges: width 1 and 8 leave fifteen workgroups idle at the barriers,
    # odd widths an odd k-split, 127 / 128 a partial and a full last strip
    "width-1-L1": (120, 1, (1,), NB, 40, 1, 1),
    "width-7-9-L9": (120, 9, (7, 9), ZINB, 40, 1, 1),
    "width-8-L128": (120, 128, (8,), ZIP, 30, 1, 1),
    "width-127-128": (120, 9, (127, 128), P, 50, 1, 1),
    "width-128-L128": (120, 128, (128,), NB, 128, 1, 1),
    # depth: one hidden layer, and MAX_HIDDEN = 8 (the most barriers)
    "depth-1": (150, 4, (32,), ZIP, 64, 1, 1),
    "depth-8": (150, 5, (9, 16, 33, 8, 128, 7, 64, 20), NB, 48, 1, 1),
}


@pytest.mark.parametrize("case", list(MID_CASES))
def test_mid_chain_against_the_oracle(cuda_device, case):
    F, L, H, likelihood, B, n_iw, n_mc = MID_CASES[case]
    _vae_case(cuda_device, F, L, H, likelihood, B, n_iw, n_mc, path="mid")


PAST_MID_CASES = {
    # one row past the mid chain: the tile chain
    "rows-129x1": (200, 10, (64, 32), NB, 129, 1, 1, "tile"),
    "rows-43x3": (200, 6, (50,), ZIP, 43, 3, 1, "tile"),
    # one column past it: the launch chain, training and evaluation
    "width-129": (200, 10, (129,), P, 64, 1, 1, "launch"),
    "L-129": (200, 129, (32, 16), ZINB, 64, 1, 1, "launch"),
}


@pytest.mark.parametrize("case", list(PAST_MID_CASES))
def test_just_past_the_mid_chain(cuda_device, case):
    F, L, H, likelihood, B, n_iw, n_mc, path = PAST_MID_CASES[case]
    _vae_case(cuda_device, F, L, H, likelihood, B, n_iw, n_mc, path=path)


TILE_CASES = {
    # R = B*S with R mod 64 = 0, 1, 63
    "R192": (300, 25, (100, 100), NB, 192, 1, 1),
    "R129-width-128-L128": (300, 128, (128,), ZINB, 129, 1, 1),
    "R191-three-odd": (300, 7, (33, 17, 9), ZIP, 191, 1, 1),
    # 50 encoder rows (less than one tile), 150 decoder rows
    "B50-iw3": (300, 10, (64, 32), P, 50, 3, 1),
    "R256-iw2-width-128": (200, 128, (128, 128), NB, 128, 2, 1),
    "R333-mc3": (250, 9, (127,), P, 111, 1, 3),
}


@pytest.mark.parametrize("case", list(TILE_CASES))
def test_tile_chain_against_the_oracle(cuda_device, case):
    F, L, H, likelihood, B, n_iw, n_mc = TILE_CASES[case]
    _vae_case(cuda_device, F, L, H, likelihood, B, n_iw, n_mc, path="tile")


def test_resident_tile_chain_three_layers(cuda_device):
    """Three layers per side: the deepest pass the resident launch takes."""
    _vae_case(cuda_device, 300, 8, (40, 30, 20), NB, 300, path="tile",
              resident=True)


def test_resident_tile_chain_refuses_four_layers(cuda_device):
    """Four layers per side: more tile stages than the resident launch holds;
    the step runs one launch per layer."""
    _vae_case(cuda_device, 300, 8, (20, 20, 20, 20), ZINB, 300, path="tile",
              resident=True, resident_taken=False)


def test_resident_tile_chain_at_its_tile_limit(cuda_device):
    """Both sides of ``tiles <= capacity / 2``: the largest minibatch the
    resident launch takes, found by bisecting the query, and one row more."""
    from scvae_amd.engine import Engine
    F, L, H = 24, 4, (16, 12)
    eng = Engine(F, L, H, ZIP, device=cuda_device)
    eng.set_tile_resident(True)
    eng.reserve(256, 1)
    lo, hi = 129, 1 << 22
    assert eng.uses_tile_resident(lo) and not eng.uses_tile_resident(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if eng.uses_tile_resident(mid):
            lo = mid
        else:
            hi = mid
    assert lo % 64 == 0 and lo >= 64 * 64, lo   # (whole tiles, half the CUs or more)
    del eng
    _vae_case(cuda_device, F, L, H, ZIP, lo, path="tile", resident=True)
    _vae_case(cuda_device, F, L, H, NB, lo + 1, path="tile", resident=True,
              resident_taken=False)


# ---- GMVAE ----------------------------------------------------------------------

def _gmvae_quantities(eng, dev, cfg, x, eps, oracle=None):
    B, L, K, F = x.shape[0], cfg.latent_size, cfg.n_clusters, cfg.feature_size
    if oracle is None:
        params, moving = _host(eng.named_parameters()), _host(
            eng.named_moving_statistics())
        assert list(params) == list(om.gmvae_parameter_shapes(cfg))
        _, new_moving, out, grads = om.gmvae_train_step(
            cfg, dict(params), moving, om.adam_state(params), x, x, eps,
            1e-4, warm_up_weight=WARM_UP)
        oracle = (out, grads, new_moving)
    out, grads, new_moving = oracle
    xd = x.float().to(dev)
    ll = torch.zeros(K * B, device=dev)
    logits = torch.zeros(B, K, device=dev)
    zmean = torch.zeros(B, L, device=dev)
    sc = eng.step(xd, xd, eps=eps.float().to(dev), training=True,
                  warm_up_weight=WARM_UP,
                  outputs={"log_p_x_given_z": ll, "q_y_logits": logits,
                           "q_z_mean": zmean}).clone()
    torch.cuda.synchronize()
    sc = sc.cpu().double()
    assert torch.isfinite(sc[:5]).all()
    q = {}
    for i, n in enumerate(("lower_bound", "lower_bound_weighted",
                           "reconstruction_error", "kl_divergence_z")):
        q[n] = (sc[i], out[n], "scalar")
    q["log_p_x_given_z"] = (ll.cpu().double(),
                            out["log_p_x_given_z"].reshape(-1), "ll")
    q["q_y_logits"] = (logits.cpu().double(), out["q_y_logits"], "qz")
    q["z_mean"] = (zmean.cpu().double(), out["z_mean"], "qz")
    # (bounds of test_gpu_baseline_configs.py's GMVAE step, for its reasons)
    close_scalar(sc[4], out["kl_divergence_y"], rtol=2e-4, atol=1e-6,
                 what="kl_divergence_y")
    for name, g in _host(eng.named_gradients()).items():
        want = grads[name]
        if _bn_bias(name):
            q["grad " + name] = (g, want, "bn_bias")
            continue
        if name == "Z/Q/ENCODER/LAYER_1/DENSE/weights":
            # the one-hot rows W[F+k] are cancelled by the per-pass batch norm
            assert g[F:].abs().max().item() < 1e-5
            g, want = g[:F], want[:F]
        q["grad " + name] = (g, want, "grad:{}".format(
            2e-3 if name.startswith("Y/") else 5e-4))
    for name, m in _host(eng.named_moving_statistics()).items():
        q["moving " + name] = (m, new_moving[name], "moving:2e-5")
    return q, oracle


@pytest.mark.parametrize("B,L,H,likelihood,path", [
    (128, 128, (64,), NB, "tile"),           # whole tiles: the K passes as tile groups
    (192, 9, (33, 17), ZINB, "tile"),
    (100, 12, (40, 40), P, "launch"),        # not a multiple of 64
    (32, 6, (24,), ZIP, "launch"),           # mid-chain-sized: no mid chain for a GMVAE
])
def test_gmvae_chain_paths_against_the_oracle(cuda_device, B, L, H, likelihood,
                                              path):
    from scvae_amd.engine import Engine
    F, K = 160, 3
    rng = np.random.default_rng(B + L)
    x = _counts(rng, B, F)
    eps = torch.from_numpy(rng.standard_normal((K, 1, B, L)))
    cfg = om.ModelConfig(feature_size=F, latent_size=L, hidden_sizes=H,
                         likelihood=likelihood, n_clusters=K)

    def engine():
        eng = Engine(F, L, H, likelihood, batch_norm=True, model_type="GMVAE",
                     n_clusters=K, device=cuda_device, seed=0)
        _perturb(eng, 2)
        eng.reserve(B, 1)
        assert not eng.uses_mid_chain(B) and not eng.uses_mid_chain(
            B, training=False)
        return eng

    eng = engine()
    assert eng.uses_tile_chain(B) == (path == "tile")
    chain, oracle = _gmvae_quantities(eng, cuda_device, cfg, x, eps)
    _hold_to_oracle(chain)
    if path != "tile":
        return
    del eng
    ref = engine()
    ref.set_tile_chain(False)
    assert not ref.uses_tile_chain(B)
    launch, _ = _gmvae_quantities(ref, cuda_device, cfg, x, eps, oracle)
    _hold_to_oracle(launch)
    _differential(chain, launch, "GMVAE tile B={} H={} L={} {}".format(
        B, H, L, likelihood))


# ---- one epoch of `scvae train` at cfg1's defaults --------------------------------

def test_default_training_epoch_matches_oracle(tmp_path, cuda_device):
    """``VariationalAutoencoder.train`` with every model default (cfg1: L = 2,
    H = [100], Poisson, B = 100, learning rate 1e-4) over 250 cells x 100
    genes: two full minibatches and a 50-cell tail, all on the mid chain,
    against the oracle driven with the same permutation and the same Philox
    noise; then the epoch-end ELBO of the training set.  Three Adam steps:
    further in, the evaluation-mode ELBO amplifies 1e-6 differences in the
    moving statistics (test_gpu_models.py)."""
    from scvae_amd.data import DataSet
    from scvae_amd.minibatch import philox_normal
    from scvae_amd.models import VariationalAutoencoder
    from scvae_amd.models.utilities import load_learning_curves
    n, F = 250, 100
    rng = np.random.default_rng(5)
    values = _counts(rng, n, F).numpy().astype(np.float32)
    data = DataSet("cfg1", values=values, labels=None,
                   example_names=np.arange(n).astype(str),
                   feature_names=np.arange(F).astype(str), kind="training")
    model = VariationalAutoencoder(feature_size=F,
                                   log_directory=str(tmp_path),
                                   device=cuda_device)
    eng = model.engine
    L, B, lr = eng.latent_size, 100, 1e-4
    assert (L, eng.hidden_sizes, eng.likelihood) == (2, [100], P)
    params, moving = _host(eng.named_parameters()), _host(
        eng.named_moving_statistics())

    def philox(rows, cols, row_offset, stream_id):
        out = torch.empty(rows, cols, device=cuda_device)
        philox_normal(out, row_offset, model.noise_seed, stream_id)
        return out.cpu().double()

    np.random.seed(11)
    model.train(data, None, number_of_epochs=1, minibatch_size=B,
                learning_rate=lr)
    assert eng.uses_mid_chain(B) and eng.uses_mid_chain(n % B)

    cfg = om.ModelConfig(feature_size=F, latent_size=L, hidden_sizes=(100,),
                         likelihood=P)
    x = torch.from_numpy(values.astype(np.float64))
    np.random.seed(11)
    perm = np.random.permutation(n)
    state = om.adam_state(params)
    for step, i in enumerate(range(0, n, B)):
        idx = perm[i:i + B]
        eps = philox(len(idx), L, 0, step).unsqueeze(0)
        params, moving, _, _ = om.vae_train_step(
            cfg, params, moving, state, x[idx], x[idx], eps, lr)
    assert step == 2
    for name, p in _host(eng.named_parameters()).items():
        if _bn_bias(name):
            continue
        err = (p - params[name]).abs().max().item()
        assert err <= 3e-4 * params[name].abs().max().item() + 1e-7, name
    # epoch-end ELBO of the training set, at the engine's own state
    params, moving = _host(eng.named_parameters()), _host(
        eng.named_moving_statistics())
    total = 0.0
    for i in range(0, n, B):
        rows = slice(i, min(i + B, n))
        eps = philox(rows.stop - rows.start, L, i,
                     (1 << 40) + 1 * (1 << 20)).unsqueeze(0)
        total += float(om.vae_forward(cfg, params, moving, x[rows], x[rows],
                                      eps, False)["lower_bound"])
    expected = total / (n / B)
    got = load_learning_curves(model)["training"]["lower_bound"][0]
    assert abs(got - expected) <= 1e-4 * abs(expected)
