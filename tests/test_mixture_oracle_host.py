"""tests/_mixture_oracle.py on the host: its fp64 restatements pinned to
``oracle/models.py`` (``gmvae_forward`` and its autograd on a tiny model: the
uniform, custom and learned priors, free nats on both sides of the threshold),
and the plain NumPy fp32 evaluation of every entry taken through the SAME
asserts, on the SAME inputs, as tests/test_gpu_mixture_stage.py: a correct fp32
implementation of the kernels' formulation meets every derived bound."""
import math

import numpy as np
import pytest
import torch

from oracle import models as om

import _mixture_oracle as mo

RUN = mo.Fp32Evaluation()


@pytest.fixture
def exact_inputs():
    mo.ROUND_INPUTS = False
    yield
    mo.ROUND_INPUTS = True


def _tiny(prior_kind, free_nats):
    K, L, F, H, B, S = 3, 3, 12, (5,), 6, 2
    method = {"uniform": "uniform", "custom": "custom", "learned": "learn"}[prior_kind]
    cfg = om.ModelConfig(
        feature_size=F, latent_size=L, hidden_sizes=H, likelihood="poisson",
        minibatch_normalisation=False, n_clusters=K, n_iw=S, n_mc=1,
        free_nats_proportion=free_nats, prior_probabilities_method=method,
        prior_probabilities=(0.2, 0.3, 0.5) if method == "custom" else ())
    params = om.init_parameters(om.gmvae_parameter_shapes(cfg), seed=3)
    g = torch.Generator().manual_seed(5)
    for name, p in params.items():
        if not name.endswith("weights"):
            params[name] = 0.4 * torch.randn(p.shape, generator=g, dtype=torch.float64)
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.poisson(1.5, (B, F)).astype(np.float64))
    eps = torch.from_numpy(rng.standard_normal((K, S, B, L)))
    return cfg, params, x, eps


def _prior_logits(cfg, params):
    if cfg.prior_probabilities_method == "uniform":
        return None
    if cfg.prior_probabilities_method == "learn":
        return params["Y/P/LOGITS"].numpy()
    return np.log(np.asarray(cfg.prior_probabilities))


@pytest.mark.parametrize("side", ["above", "below"])
@pytest.mark.parametrize("prior_kind", ["uniform", "custom", "learned"])
def test_restatement_matches_the_model_oracle(exact_inputs, prior_kind, side):
    """Stage by stage through the helpers = om.gmvae_forward, values and
    gradients, to fp64 rounding."""
    w_up = 0.6
    cfg, params, x, eps = _tiny(prior_kind, 0.0)
    probe = om.gmvae_forward(cfg, params, {}, x, x, eps, True, w_up)
    prior = _prior_logits(cfg, params)
    H_p = (math.log(cfg.n_clusters) if prior is None
           else float(-(torch.softmax(torch.from_numpy(prior), 0)
                        * torch.log_softmax(torch.from_numpy(prior), 0)).sum()))
    # a threshold 30 % to either side of this model's KL_y
    free_nats = float(probe["kl_divergence_y"]) / H_p * (0.7 if side == "above" else 1.3)
    cfg, params, x, eps = _tiny(prior_kind, free_nats)
    out, grads = om.gradients(
        lambda p: om.gmvae_forward(cfg, p, {}, x, x, eps, True, w_up), params)
    K, L, S, B = cfg.n_clusters, cfg.latent_size, cfg.n_iw, x.shape[0]
    Hs = list(cfg.hidden_sizes)

    def close(got, want, what):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.abs(got - want).max() <= 1e-11 * (1.0 + np.abs(want).max()), what

    logits = out["q_y_logits"].numpy()
    cat, _ = mo.categorical_fwd(logits, prior)
    close(cat["y"].value, out["y"], "y")
    close(cat["kl"].value.mean(), out["kl_divergence_y"], "kl_divergence_y")
    qm, qs = [], []
    for k in range(K):      # (as gmvae_forward builds q(z|x,y=k))
        h = om._layers(x, params, "Z/Q/ENCODER", Hs, False, True, {}, {}, extra_row=k)
        qm.append(om.dense_layer(h, params, "Z/Q/SOFTPLUS_GAUSSIAN/MEAN", False, True, {},
                                 None, activation=False))
        qs.append(om.dense_layer(h, params, "Z/Q/SOFTPLUS_GAUSSIAN/SOFTPLUS_SCALE", False,
                                 True, {}, None, activation=False))
    inv_gb = 1.0 / B
    ll = out["log_p_x_given_z"].numpy()
    y = cat["y"].value
    arrays = dict(
        qm=torch.cat(qm).numpy(), qs=torch.cat(qs).numpy(),
        Wpm=params["Z/P/SOFTPLUS_GAUSSIAN/MEAN/DENSE/weights"].numpy(),
        bpm=params["Z/P/SOFTPLUS_GAUSSIAN/MEAN/DENSE/biases"].numpy(),
        Wps=params["Z/P/SOFTPLUS_GAUSSIAN/SOFTPLUS_SCALE/DENSE/weights"].numpy(),
        bps=params["Z/P/SOFTPLUS_GAUSSIAN/SOFTPLUS_SCALE/DENSE/biases"].numpy(),
        eps=eps.numpy(), dz=np.zeros((K, S, B, L)), gklz=np.zeros((K, S, B)))
    klz = mo.pair(arrays, K, S, B, L)[0]["klz"].value
    e = mo.elbo_fwd(ll, klz, y, cat["kl"].value, inv_gb, w_up, free_nats, 1.0, prior)
    for i, name in enumerate(("lower_bound", "lower_bound_weighted", "reconstruction_error",
                              "kl_divergence_z", "kl_divergence_y")):
        close(e["scalars"].value[i], out[name], name)
    close(e["rec_cell"].value, out["reconstruction_cell"], "reconstruction_cell")
    assert e["gate"] == (1.0 if side == "above" else 0.0)
    assert (float(out["kl_divergence_y"]) > e["thr"]) == (side == "above")
    stats = mo.prior_stats(arrays["Wpm"], arrays["bpm"], arrays["Wps"], arrays["bps"])
    close(stats["means"].value, out["p_z_means"], "p_z_means")
    close(stats["variances"].value, out["p_z_variances"], "p_z_variances")
    # backward: d(-lower_bound_weighted) / d ...
    b = mo.elbo_bwd(ll, klz, y, w_up, inv_gb)
    dl = mo.categorical_bwd(y, b["dy"].value, e["gate"], w_up * inv_gb, prior).value
    close(dl.sum(axis=0), grads["Y/CATEGORICAL/LOGITS/DENSE/biases"], "sum_b dlogits")
    arrays["gklz"] = b["gklz"].value
    dpr = mo.pair(arrays, K, S, B, L)[0]["dpr"].value.sum(axis=1)
    close(dpr[:, :L], grads["Z/P/SOFTPLUS_GAUSSIAN/MEAN/DENSE/weights"], "d prior means")
    close(dpr[:, L:], grads["Z/P/SOFTPLUS_GAUSSIAN/SOFTPLUS_SCALE/DENSE/weights"],
          "d prior scales")
    if prior_kind == "learned":
        dp = mo.prior_logits_bwd(y, prior, e["gate"], w_up * inv_gb, w_up, free_nats).value
        close(dp, grads["Y/P/LOGITS"], "d prior logits")


@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("gate", [1.0, 0.0])
def test_categorical_backward_closed_form_is_autograd(exact_inputs, learned, gate):
    logits, prior, dy, c = mo.categorical_inputs(65, 5, "ordinary", learned)
    lt = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    log_y = torch.log_softmax(lt, dim=-1)
    yt = torch.exp(log_y)
    if learned:
        log_p = torch.log_softmax(torch.from_numpy(prior.astype(np.float64)), dim=-1)
        kl = (yt * (log_y - log_p)).sum()
    else:
        kl = (yt * log_y).sum()
    ((yt * torch.from_numpy(dy.astype(np.float64))).sum() + c * gate * kl).backward()
    got = mo.categorical_bwd(yt.detach().numpy(), dy, gate, c, prior).value
    assert np.abs(got - lt.grad.numpy()).max() <= 1e-13


# ---- the fp32 evaluation through the GPU test's asserts, on its inputs ----
@pytest.mark.parametrize("learned", [False, True], ids=["uniform", "learned"])
@pytest.mark.parametrize("K", mo.CAT_K)
def test_fp32_categorical_shapes(K, learned):
    for B in mo.CAT_B:
        mo.check_categorical(RUN, K, B, "ordinary", learned)


@pytest.mark.parametrize("learned", [False, True], ids=["uniform", "learned"])
@pytest.mark.parametrize("regime", mo.CAT_REGIMES[1:])
def test_fp32_categorical_regimes(regime, learned):
    for K, B in ((2, 5), (65, 5), (200, 3)):
        mo.check_categorical(RUN, K, B, regime, learned)


def test_fp32_pair_shapes():
    for K, S, B, L in mo.PAIR_SHAPES:
        mo.check_pair(RUN, K, S, B, L)


@pytest.mark.parametrize("regime", ["scales", "clip"])
def test_fp32_pair_regimes(regime):
    if regime == "clip":
        mo.check_pair(RUN, *mo.CLIP_SHAPE, regime="clip")
        mo.check_prior_stats(RUN, mo.CLIP_SHAPE[0], mo.CLIP_SHAPE[3], clip=True)
    else:
        for K, S, B, L in ((3, 3, 7, 65), (3, 1, 7, 130)):
            info = mo.check_pair(RUN, K, S, B, L, regime="scales")
            assert info["inv_sg"].max() > 1e17      # (the -g / sg term does dominate)
    mo.check_prior_stats(RUN, 7, 37)


def test_fp32_elbo():
    for K, S, B in mo.ELBO_SHAPES:
        for w in mo.ELBO_WEIGHTS:
            for share in mo.ELBO_SHARES:
                mo.check_elbo(RUN, K, S, B, w, share)


@pytest.mark.parametrize("prior_kind,side", mo.GATE_CASES)
def test_fp32_gate_and_its_margins(prior_kind, side):
    """Also what the GPU test relies on: fp64 KL_y at least 1e-3 thr from thr,
    and that margin above anything fp32 may lose (asserted in check_gate)."""
    mo.check_gate(RUN, prior_kind, side)


def test_fp32_prior_logits_bwd_and_group_ops():
    for K, B in ((1, 1), (9, 255), (65, 257), (200, 600)):
        mo.check_prior_bwd_shapes(RUN, K, B)
    for case in mo.GROUP_COL_SUM_CASES:
        mo.check_group_col_sum(RUN, *case)
    for weighted in (False, True):
        mo.check_sum_groups(RUN, 3, 7, 65, weighted)
        mo.check_sum_groups(RUN, 3, 4100, 130, weighted)
    for relu in (0, 1):
        mo.check_add_group_rows(RUN, 3, 7, 65, relu)
        mo.check_add_group_rows(RUN, 3, 1400, 130, relu)
