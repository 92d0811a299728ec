"""GPU parity: GMVAE steps with the "full-covariance gaussian mixture" latent
distribution (latent_mode bit 3) through ``Engine.step`` + ``adam_step``
against the fp64 restatement in ``_fullcov_oracle`` -- modelled on
``test_gpu_gmvae_step.py``: same setup, same tolerances, the same treatment of
Adam near a zero gradient -- and the model class on top of it."""
import os

import numpy as np
import pytest
import torch

from oracle import models as om

import _fullcov_oracle as fo
from _parity import LL_ATOL, LL_RTOL, close_elementwise

pytestmark = pytest.mark.gpu

NAME = "full-covariance gaussian mixture"
F_, L_, K_, H_ = 157, 6, 4, (24, 16)
SEED = 0x1234ABCD5678


def _close(a, b, rtol=1e-4, what=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "{}: max err {:.3e} of scale {:.3e}".format(
        what, err, scale)


def _setup(device, likelihood, B, bn, S=1, free_nats=0.0, seed=0, keeps=None):
    from scvae_amd.engine import Engine
    eng = Engine(F_, L_, H_, likelihood, batch_norm=bn, model_type="GMVAE",
                 n_clusters=K_, free_nats_proportion=free_nats, device=device,
                 seed=seed, latent_distribution=NAME,
                 dropout_keep_probabilities=keeps)
    g = torch.Generator().manual_seed(seed + 1)
    for name, p in eng.named_parameters().items():
        if not name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    cfg = om.ModelConfig(feature_size=F_, latent_size=L_, hidden_sizes=H_,
                         likelihood=likelihood, minibatch_normalisation=bn,
                         n_clusters=K_, n_iw=S, n_mc=1,
                         free_nats_proportion=free_nats)
    params = {k: v.detach().cpu().double()
              for k, v in eng.named_parameters().items()}
    assert {k: tuple(v.shape) for k, v in params.items()} == dict(
        fo.parameter_shapes(cfg))
    assert list(params) == list(fo.parameter_shapes(cfg))
    moving = {k: v.detach().cpu().double()
              for k, v in eng.named_moving_statistics().items()}
    rng = np.random.default_rng(seed)
    lam = rng.gamma(0.5, 3.0, size=(1, F_))
    x = rng.poisson(lam, size=(B, F_)).astype(np.float64)
    x *= rng.random((B, F_)) > 0.6
    x = torch.from_numpy(x)
    eps = torch.from_numpy(rng.standard_normal((K_, S, B, L_)))
    return eng, cfg, params, moving, x, eps


def _outputs(device, B, S):
    return {"log_p_x_given_z": torch.zeros(K_ * S * B, device=device),
            "q_y_logits": torch.zeros(B, K_, device=device),
            "q_z_mean": torch.zeros(B, L_, device=device),
            "cluster_stats": torch.zeros(4, K_, L_, device=device),
            "cluster_covariances": torch.zeros(2, K_, L_, L_, device=device)}


def _check_outputs(sc, outs, out):
    _close(sc[0], out["lower_bound"], what="lower_bound")
    _close(sc[1], out["lower_bound_weighted"], what="lower_bound_weighted")
    _close(sc[2], out["reconstruction_error"], what="reconstruction_error")
    _close(sc[3], out["kl_divergence_z"], what="kl_divergence_z")
    _close(sc[4], out["kl_divergence_y"], rtol=2e-4, what="kl_divergence_y")
    close_elementwise(outs["log_p_x_given_z"],
                      out["log_p_x_given_z"].reshape(-1), rtol=LL_RTOL,
                      atol=LL_ATOL, what="per-cell ll")
    _close(outs["q_y_logits"].cpu(), out["q_y_logits"], what="q_y_logits")
    _close(outs["q_z_mean"].cpu(), out["z_mean"], what="z_mean")
    cstats = outs["cluster_stats"].cpu()
    for i, key in enumerate(("p_z_means", "p_z_variances", "q_z_means",
                             "q_z_variances")):
        _close(cstats[i], out[key], what=key)
    ccov = outs["cluster_covariances"].cpu()
    _close(ccov[0], out["p_z_covariances"], what="p_z_covariances")
    _close(ccov[1], out["q_z_covariances"], what="q_z_covariances")


def _check_gradients(eng, grads, bn, rtol=3e-4, dropped_input=False):
    for name, g in eng.named_gradients().items():
        if bn and name.endswith("DENSE/biases") and "LAYER_" in name:
            assert g.abs().max().item() < 1e-5, name
            continue
        got, want = g.cpu(), grads[name]
        if (bn and name == "Z/Q/ENCODER/LAYER_1/DENSE/weights"
                and not dropped_input):
            got, want = got[:F_], want[:F_]   # one-hot rows: cancelled by BN
        _close(got, want, rtol=rtol, what="grad " + name)


def _train_case(device, likelihood, bn, S, free_nats, B):
    eng, cfg, params, moving, x, eps = _setup(device, likelihood, B, bn, S,
                                              free_nats)
    xd = x.float().to(device)
    epsd = eps.float().to(device)
    outs = _outputs(device, B, S)
    sc = eng.step(xd, xd, eps=epsd, training=True, n_iw=S, n_mc=1,
                  warm_up_weight=0.6, outputs=outs).cpu().numpy()
    eng.adam_step(1e-3)
    torch.cuda.synchronize()
    # B = 64 with batch norm: whole tiles per pass, the hidden layers take the
    # tile chain and the heads of this mode the GEMM launches
    assert eng.uses_tile_chain(B, S) == (bn and B % 64 == 0)

    state = om.adam_state(params)
    new_params, new_moving, out, grads = fo.train_step(
        cfg, dict(params), moving, state, x, x, eps, 1e-3, warm_up_weight=0.6)
    _check_outputs(sc, outs, out)
    _check_gradients(eng, grads, bn)
    # Adam near a zero gradient: see test_gpu_gmvae_step.py
    eps_hat = om.ADAM_EPSILON / np.sqrt(1.0 - om.ADAM_BETA2)
    own = om.clip_and_adam(
        dict(params),
        {k: g.cpu().double() for k, g in eng.named_gradients().items()},
        om.adam_state(params), 1e-3)
    for name, p in eng.named_parameters().items():
        if bn and name.endswith("DENSE/biases") and "LAYER_" in name:
            continue
        near = grads[name].abs() <= 100 * eps_hat
        got, want = p.cpu(), torch.where(near, own[name], new_params[name])
        if bn and name == "Z/Q/ENCODER/LAYER_1/DENSE/weights":
            assert eng.gradient(name)[F_:].abs().max().item() < 1e-5
            got, want = got[:F_], want[:F_]
        _close(got, want, rtol=3e-4, what="param " + name)
    for name, m in eng.named_moving_statistics().items():
        _close(m.cpu(), new_moving[name], rtol=2e-5, what="moving " + name)
    return eng, cfg, x, eps


@pytest.mark.parametrize("likelihood,bn,S", [
    ("negative binomial", True, 1),
    ("zero-inflated negative binomial", True, 2),
    ("poisson", False, 1),
])
@pytest.mark.parametrize("B", [29, 64])   # the launch chain, the tile chain
def test_train_step_matches_oracle(cuda_device, likelihood, bn, S, B):
    _train_case(cuda_device, likelihood, bn, S, 0.0, B)


def test_train_step_with_free_nats(cuda_device):
    _train_case(cuda_device, "negative binomial", True, 1, 0.8, 29)


@pytest.mark.parametrize("B", [29, 64])
def test_evaluation_step_matches_oracle(cuda_device, B):
    S = 2
    eng, cfg, params, moving, x, eps = _setup(
        cuda_device, "negative binomial", B, True, S)
    xd = x.float().to(cuda_device)
    outs = _outputs(cuda_device, B, S)
    sc = eng.step(xd, xd, eps=eps.float().to(cuda_device), training=False,
                  n_iw=S, n_mc=1, outputs=outs).cpu().numpy()
    torch.cuda.synchronize()
    out = fo.forward(cfg, params, moving, x, x, eps, False)
    _check_outputs(sc, outs, out)


def test_workspace_guard_runs_clean(cuda_device, monkeypatch):
    """Every workspace buffer followed by a guard region that the step checks:
    the buffers resized for the triangle (qs, dqs, dprior, the covariance
    scratch) are not overrun.  The switch is read once per process, so the
    step runs in a fresh one."""
    import subprocess
    import sys
    monkeypatch.setenv("SCVAE_WS_GUARD", "1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys; sys.path[:0] = [{root!r}, {tests!r}]\n"
        "import torch\n"
        "import test_gpu_fullcov_step as t\n"
        "for B, S in ((29, 2), (64, 1)):\n"
        "    t._train_case(torch.device('cuda:0'), 'negative binomial', True,"
        " S, 0.0, B)\n"
        "print('guarded steps ok')\n").format(
            root=root, tests=os.path.join(root, "tests"))
    done = subprocess.run([sys.executable, "-c", script], capture_output=True,
                          text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "guarded steps ok" in done.stdout


def test_head_dropout_matches_oracle(cuda_device):
    """dropout_keep h and y on the four new heads: sites 16, 17 (Z/Q
    locations, scales: [K B, H_last] masks) and 24, 25 (Z/P: the one-hot's one
    non-zero input of each pass), the masks read back through
    ``scvae_dropout_apply`` and handed to the oracle."""
    B, S = 27, 1
    keeps = (0.8, 0.0, 0.0, 0.6)
    eng, cfg, params, moving, x, eps = _setup(
        cuda_device, "negative binomial", B, True, S, keeps=keeps)
    kh, ky = keeps[0], keeps[3]
    masks = {}

    def add(scope, site, rows, width, keep, passes=0):
        m = eng.dropout_mask(site, max(passes, 1) * rows, width, keep, SEED)
        masks[scope] = (m.view(passes, rows, width) if passes
                        else m).cpu().double()
    width = F_
    for i, h in enumerate(H_):
        if i > 0:
            add("Y/CATEGORICAL/ENCODER/LAYER_{}".format(i + 1), 64 + i, B,
                width, kh)
            add("Z/Q/ENCODER/LAYER_{}".format(i + 1), i, B, width, kh,
                passes=K_)
        width = h
    add("Y/CATEGORICAL/LOGITS", 80, B, width, kh)
    add("Z/Q/MULTIVARIATE_GAUSSIAN/LOCATIONS", 16, B, width, kh, passes=K_)
    add("Z/Q/MULTIVARIATE_GAUSSIAN/SCALES", 17, B, width, kh, passes=K_)
    add("Z/P/MULTIVARIATE_GAUSSIAN/LOCATIONS", 24, K_, K_, ky)
    add("Z/P/MULTIVARIATE_GAUSSIAN/SCALES", 25, K_, K_, ky)
    width = L_
    for i, h in enumerate(H_[::-1]):
        if i > 0:
            add("X/DECODER/LAYER_{}".format(i + 1), 32 + i, S * B, width, kh,
                passes=K_)
        width = h
    for j, head in enumerate(cfg.heads):
        add("X/DISTRIBUTION/" + head.upper(), 48 + j, S * B, width, kh,
            passes=K_)
    # both kinds of prior mask occur: a dropped and a kept pass
    diagonal = torch.diagonal(masks["Z/P/MULTIVARIATE_GAUSSIAN/SCALES"])
    assert (diagonal == 0).any() and (diagonal > 0).any()

    xd = x.float().to(cuda_device)
    outs = {"log_p_x_given_z": torch.zeros(K_ * S * B, device=cuda_device)}
    sc = eng.step(xd, xd, eps=eps.float().to(cuda_device), training=True,
                  n_iw=S, n_mc=1, warm_up_weight=0.7, dropout_seed=SEED,
                  outputs=outs).cpu().numpy()
    torch.cuda.synchronize()
    new_moving = {}
    out, grads = om.gradients(
        lambda p: fo.forward(cfg, p, moving, x, x, eps, True, 0.7, new_moving,
                             dropout=masks), params)
    _close(sc[0], out["lower_bound"], what="lower_bound")
    _close(sc[1], out["lower_bound_weighted"], what="lower_bound_weighted")
    _close(sc[3], out["kl_divergence_z"], what="kl_divergence_z")
    _close(sc[4], out["kl_divergence_y"], rtol=2e-4, what="kl_divergence_y")
    close_elementwise(outs["log_p_x_given_z"],
                      out["log_p_x_given_z"].reshape(-1), rtol=LL_RTOL,
                      atol=LL_ATOL, what="per-cell ll")
    _check_gradients(eng, grads, True)


# ------------------------------- model class --------------------------------

def _data(n=200, F=157, seed=3):
    from scvae_amd.data import DataSet
    rng = np.random.default_rng(seed)
    centres = rng.gamma(1.0, 2.0, size=(3, F))
    lab = rng.integers(0, 3, size=n)
    x = rng.poisson(centres[lab]).astype(np.float32)
    x *= rng.random((n, F)) > 0.5
    return DataSet("toy", values=x,
                   labels=np.array(["c%d" % k for k in lab]),
                   example_names=np.arange(n).astype(str),
                   feature_names=np.arange(F).astype(str), kind="training")


def _new_model(directory):
    from scvae_amd.models import GaussianMixtureVariationalAutoencoder
    return GaussianMixtureVariationalAutoencoder(
        feature_size=F_, latent_size=L_, hidden_sizes=list(H_),
        reconstruction_distribution="negative binomial",
        latent_distribution=NAME, number_of_latent_clusters=K_,
        log_directory=str(directory))


def _evaluated_scalars(model):
    from scvae_amd.models import utilities as mu
    records = mu._read_scalars(
        os.path.join(model.log_directory(), "evaluation"))
    return records[-1]["scalars"]


def test_model_trains_evaluates_samples_and_reloads(tmp_path, cuda_device):
    from scvae_amd.models.utilities import load_centroids
    data = _data()
    state = np.random.get_state()
    np.random.seed(20261018)
    try:
        model = _new_model(tmp_path / "a")
        assert model.train(data, None, number_of_epochs=2, minibatch_size=32,
                           learning_rate=1e-2) == 0
    finally:
        np.random.set_state(state)
    model.evaluate(data, minibatch_size=32, output_versions="latent")
    scalars = _evaluated_scalars(model)
    assert np.isfinite(scalars["losses/lower_bound"])

    centroids = model._centroids(model._prior_summary())
    covariances = centroids["prior"]["covariance_matrices"]
    assert covariances.shape == (K_, L_, L_)
    assert np.allclose(covariances, covariances.transpose(0, 2, 1),
                       rtol=1e-12, atol=0)
    assert (np.linalg.eigvalsh(covariances) > 0).all()
    off_diagonal = covariances[:, ~np.eye(L_, dtype=bool)]
    assert (np.abs(off_diagonal) > 1e-3).all()
    # the store the analyses read: per epoch, the logged P P^T entries
    logged = load_centroids(model, "training")["prior"]["covariance_matrices"]
    assert logged.shape == (2, K_, L_, L_)
    assert np.allclose(logged[-1], covariances, rtol=1e-5, atol=1e-7)
    for side in ("prior", "posterior"):
        tag = "{}/cluster_1/covariance/dimension_2_0".format(side)
        assert np.isfinite(scalars[tag]) and scalars[tag] != 0
    assert np.isclose(scalars["prior/cluster_1/covariance/dimension_2_0"],
                      covariances[1, 2, 0], rtol=1e-5)
    assert np.isclose(scalars["prior/cluster_1/variance/dimension_2"],
                      covariances[1, 2, 2], rtol=1e-5)

    sampled = model.sample(sample_size=5)
    members = sampled if isinstance(sampled, (list, tuple)) else [sampled]
    found = 0
    for member in members:
        sets = member.values() if isinstance(member, dict) else [member]
        for data_set in sets:
            assert np.isfinite(np.asarray(data_set.values)).all()
            found += 1
    assert found

    # checkpoints save and reload by parameter name
    # (the noise of an evaluation pass is keyed by the number of passes the
    #  model object has run, so the round trip compares fresh objects: each
    #  loads the checkpoint and draws its first pass's noise)
    trained = model.engine.params.clone()
    elbos = []
    for _ in range(2):
        again = _new_model(tmp_path / "a")
        again.evaluate(data, minibatch_size=32, output_versions="latent")
        assert torch.equal(again.engine.params, trained)
        elbos.append(_evaluated_scalars(again)["losses/lower_bound"])
    assert np.isfinite(elbos[0]) and elbos[0] == elbos[1]
    # the part of the bound that no noise enters agrees with the trained object
    assert (_evaluated_scalars(again)["losses/kl_divergence_y"]
            == scalars["losses/kl_divergence_y"])


def test_deterministic_runs_are_bit_identical(tmp_path, cuda_device):
    data = _data()
    params = []
    for run in ("first", "second"):
        state = np.random.get_state()
        np.random.seed(7)
        try:
            model = _new_model(tmp_path / run)
            assert model.train(data, None, number_of_epochs=2,
                               minibatch_size=32, learning_rate=1e-2,
                               deterministic=True) == 0
        finally:
            np.random.set_state(state)
        params.append(model.engine.params.clone())
    assert torch.equal(params[0], params[1])
    assert torch.isfinite(params[0]).all()
