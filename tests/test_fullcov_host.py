"""Host side of the "full-covariance gaussian mixture" latent distribution
(du:75-93, 347-349): triangle layout, the fp64 restatement against
``torch.distributions.MultivariateNormal``, registry / constructor / names and
the C-ABI plan layout.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import models as om

import _fullcov_oracle as fo

NAME = "full-covariance gaussian mixture"


def test_fill_triangular_order():
    """tfp's documented example pins the order."""
    from scvae_amd.distributions.utilities import fill_triangular
    x = torch.arange(1.0, 7.0, dtype=torch.float64)
    want = torch.tensor([[4.0, 0, 0], [6, 5, 0], [3, 2, 1]],
                        dtype=torch.float64)
    assert torch.equal(fo.fill_triangular(x), want)
    assert torch.equal(fill_triangular(x), want)
    # batched, and the degenerate triangle
    xb = torch.stack([x, 2 * x])
    assert torch.equal(fill_triangular(xb), torch.stack([want, 2 * want]))
    assert torch.equal(fill_triangular(torch.tensor([3.0])),
                       torch.tensor([[3.0]]))
    with pytest.raises(ValueError):
        fill_triangular(torch.zeros(5))


@pytest.mark.parametrize("L", [1, 6, 25])
def test_oracle_log_probabilities_match_torch(L):
    """The restatement's log q - log p against torch's MultivariateNormal
    (an independent implementation) in fp64."""
    g = torch.Generator().manual_seed(L)
    T, B, S = L * (L + 1) // 2, 5, 2
    qloc = torch.randn(B, L, generator=g, dtype=torch.float64)
    qpre = 0.3 * torch.randn(B, T, generator=g, dtype=torch.float64)
    ploc = torch.randn(L, generator=g, dtype=torch.float64)
    ppre = 0.3 * torch.randn(T, generator=g, dtype=torch.float64)
    eps = torch.randn(S, B, L, generator=g, dtype=torch.float64)
    z, klz, A, P = fo.latent_pair(qloc, qpre, ploc, ppre, eps)
    q = torch.distributions.MultivariateNormal(qloc, scale_tril=A)
    p = torch.distributions.MultivariateNormal(ploc, scale_tril=P)
    want = q.log_prob(z) - p.log_prob(z)
    assert torch.allclose(klz, want, rtol=1e-12, atol=1e-12)
    # log q at the sample is -|eps|^2 / 2 - sum log A_ii - c
    log_q = (-0.5 * (eps ** 2).sum(-1)
             - torch.log(torch.diagonal(A, dim1=-2, dim2=-1)).sum(-1)
             - L * om.HALF_LOG_2PI)
    assert torch.allclose(q.log_prob(z), log_q, rtol=1e-12, atol=1e-12)


def test_registry_entries():
    from scvae_amd.distributions import utilities as du
    entry = du.DISTRIBUTIONS["multivariate gaussian"]
    assert list(entry["parameters"]) == ["locations", "scales"]
    assert entry["parameters"]["scales"]["size function"](25) == 325
    assert "size function" not in entry["parameters"]["locations"]
    assert du.GAUSSIAN_MIXTURE_DISTRIBUTIONS[NAME] == {
        "z prior": "multivariate gaussian",
        "z posterior": "multivariate gaussian"}
    assert NAME not in du.UNSUPPORTED_DISTRIBUTIONS
    assert "multivariate gaussian" not in du.UNSUPPORTED_DISTRIBUTIONS
    assert du.parse_distribution("full_covariance_gaussian_mixture",
                                 "GMVAE") == NAME
    with pytest.raises(ValueError):
        du.parse_distribution(NAME, "VAE")
    d = entry["class"]({"locations": torch.zeros(2, dtype=torch.float64),
                        "scales": torch.tensor([1.0, 2.0, 3.0],
                                               dtype=torch.float64)})
    # scale_tril = [[3, 0], [2, 1]]
    assert torch.equal(d.covariance(), torch.tensor(
        [[9.0, 6.0], [6.0, 5.0]], dtype=torch.float64))


def _model(**kwargs):
    from scvae_amd.models import GaussianMixtureVariationalAutoencoder
    arguments = dict(feature_size=157, latent_size=6, hidden_sizes=[24, 16],
                     reconstruction_distribution="negative binomial",
                     latent_distribution=NAME, number_of_latent_clusters=4)
    arguments.update(kwargs)
    return GaussianMixtureVariationalAutoencoder(**arguments)


def test_constructor_parameter_names_shapes_and_order():
    model = _model()
    table = model._parameter_shapes()
    names = [name for name, _ in table]
    shapes = dict(table)
    L, K, T = 6, 4, 21
    scope = "MULTIVARIATE_GAUSSIAN"
    heads = [("Z/Q/{}/LOCATIONS".format(scope), (16, L)),
             ("Z/Q/{}/SCALES".format(scope), (16, T)),
             ("Z/P/{}/LOCATIONS".format(scope), (K, L)),
             ("Z/P/{}/SCALES".format(scope), (K, T))]
    first = names.index(heads[0][0] + "/DENSE/weights")
    want = []
    for head, shape in heads:
        want += [head + "/DENSE/weights", head + "/DENSE/biases"]
        assert shapes[head + "/DENSE/weights"] == shape
        assert shapes[head + "/DENSE/biases"] == (shape[1],)
    assert names[first:first + 8] == want
    # the slots of MEAN / SOFTPLUS_SCALE, everything around them unchanged
    cfg = om.ModelConfig(feature_size=157, latent_size=L,
                         hidden_sizes=(24, 16),
                         likelihood="negative binomial", n_clusters=K)
    assert table == list(fo.parameter_shapes(cfg).items())
    assert names[first - 1].startswith("Z/Q/ENCODER/LAYER_2/")
    assert names[first + 8] == "X/DECODER/LAYER_1/DENSE/weights"


@pytest.mark.parametrize("bn", [True, False])
def test_c_abi_plan_layout_matches_the_model(bn):
    from scvae_amd import _lib
    lib = _lib.load()
    model = _model(minibatch_normalisation=bn)
    cfg = _lib.ModelConfig()
    cfg.model_type = _lib.MODEL_GMVAE
    cfg.feature_size, cfg.latent_size, cfg.n_hidden = 157, 6, 2
    cfg.hidden[0], cfg.hidden[1] = 24, 16
    cfg.likelihood = _lib.NB
    cfg.batch_norm = 1 if bn else 0
    cfg.n_clusters = 4
    cfg.kl_weight = 1.0
    cfg.latent_mode = 8
    handle = ctypes.c_void_p()
    assert lib.scvae_plan_create(ctypes.byref(cfg), ctypes.byref(handle)) == 0
    try:
        name = ctypes.create_string_buffer(_lib.NAME_MAX)
        off, rows, cols = (ctypes.c_int64(), ctypes.c_int64(),
                           ctypes.c_int64())
        table = []
        for i in range(lib.scvae_plan_param_count(handle)):
            assert lib.scvae_plan_param_info(
                handle, i, name, ctypes.byref(off), ctypes.byref(rows),
                ctypes.byref(cols)) == 0
            table.append((name.value.decode(),
                          (rows.value, cols.value) if cols.value
                          else (rows.value,)))
        assert table == model._parameter_shapes()
    finally:
        lib.scvae_plan_destroy(handle)


def test_model_name_and_description():
    model = _model()
    assert model.latent_distribution_name == NAME
    assert not model.analytical_kl_term
    assert model.name == (
        "GMVAE/full_covariance_gaussian_mixture-c_4/"
        "negative_binomial-l_6-h_24_16-mc_1-iw_1-bn")
    description = model.description
    assert "latent distribution: " + NAME in description
    assert "latent clusters: 4" in description
    # the diagonal mixture keeps its names
    assert "/gaussian_mixture-c_4/" in _model(
        latent_distribution="gaussian mixture").name


def test_latent_size_limit():
    _model(latent_size=64)
    with pytest.raises(ValueError, match="at most 64"):
        _model(latent_size=65)


def test_plan_create_rejects_the_mode_where_it_does_not_apply():
    from scvae_amd import _lib
    lib = _lib.load()

    def create(model_type, latent_mode, latent_size=6):
        cfg = _lib.ModelConfig()
        cfg.model_type = model_type
        cfg.feature_size, cfg.latent_size, cfg.n_hidden = 30, latent_size, 1
        cfg.hidden[0] = 16
        cfg.n_clusters = 3 if model_type == _lib.MODEL_GMVAE else 1
        cfg.kl_weight = 1.0
        cfg.latent_mode = latent_mode
        handle = ctypes.c_void_p()
        rc = lib.scvae_plan_create(ctypes.byref(cfg), ctypes.byref(handle))
        if rc == 0:
            lib.scvae_plan_destroy(handle)
        return rc, lib.scvae_last_error().decode()

    assert create(_lib.MODEL_GMVAE, 8)[0] == 0
    assert create(_lib.MODEL_GMVAE, 8, 64)[0] == 0
    rc, message = create(_lib.MODEL_VAE, 8)
    assert rc == -1 and "GMVAE" in message
    rc, message = create(_lib.MODEL_GMVAE, 12)
    assert rc == -1 and "exclude" in message
    rc, message = create(_lib.MODEL_GMVAE, 8, 65)
    assert rc == -1 and "64" in message


def test_step_args_mirror_carries_the_covariance_output():
    from scvae_amd import _lib
    names = [name for name, _ in _lib.StepArgs._fields_]
    # next to the other cluster statistics
    assert names[names.index("cluster_stats") + 1] == "cluster_covariances"
    for symbol in ("scvae_mvn_tril_logprob_pair_fwd",
                   "scvae_mvn_tril_logprob_pair_bwd"):
        assert symbol in _lib.SIGNATURES
        assert hasattr(_lib.load(), symbol)
