"""fp64 restatement of a GMVAE step with the "full-covariance gaussian mixture"
latent distribution (TEST INFRASTRUCTURE, beside the tests because ``oracle/``
is frozen).

``oracle.models.gmvae_forward`` with the z block replaced: q(z|x,y=k) and
p(z|y=k) are ``MultivariateNormalTriL(loc, fill_triangular(scales))``
(scvae/distributions/utilities.py:75-93; gm:2936-3048, 2879-2893, 3270-3292)
with ``scales = max(softplus(pre), FLT_MIN)`` on every one of the
``L (L + 1) / 2`` entries and unclipped locations.  Everything else -- q(y|x),
the hidden stacks, the decoder, the loss -- is the oracle's own code.
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import models as om

FLOAT32_TINY = float(np.finfo(np.float32).tiny)
SCOPE = "MULTIVARIATE_GAUSSIAN"


def fill_triangular(x):
    """tfp.distributions.fill_triangular on the last axis, restated from its
    documentation: y = concat(x[L:], reverse(x)), reshape [L, L], keep the
    lower triangle.  [1..6] -> [[4,0,0],[6,5,0],[3,2,1]]."""
    T = x.shape[-1]
    L = int((math.sqrt(8 * T + 1) - 1) / 2)
    assert L * (L + 1) // 2 == T
    y = torch.cat([x[..., L:], torch.flip(x, dims=(-1,))], dim=-1)
    return torch.tril(y.reshape(x.shape[:-1] + (L, L)))


def scale_tril(pre):
    """gm:2976-2980 on du:82-87: clip(softplus(pre), 0 + tiny, inf - tiny)."""
    return fill_triangular(torch.clamp(F.softplus(pre), min=FLOAT32_TINY))


def tril_log_prob(z, loc, tril):
    """log N(z; loc, tril tril^T) without the constant's sign games:
    -|u|^2 / 2 - sum_i log tril_ii - L log(2 pi) / 2, u = tril^-1 (z - loc).
    z: [..., L]; loc, tril broadcast against it."""
    r = (z - loc).unsqueeze(-1)
    tril_b = tril.expand(r.shape[:-2] + tril.shape[-2:])
    u = torch.linalg.solve_triangular(tril_b, r, upper=False).squeeze(-1)
    log_det = torch.log(torch.diagonal(tril, dim1=-2, dim2=-1)).sum(dim=-1)
    L = z.shape[-1]
    return (-0.5 * (u * u).sum(dim=-1) - log_det
            - L * om.HALF_LOG_2PI)


def latent_pair(qloc, qpre, ploc, ppre, eps):
    """The stand-alone pair (one cluster k): qloc [B, L], qpre [B, T], ploc
    [L], ppre [T], eps [S, B, L] -> z [S, B, L], klz [S, B], A [B, L, L],
    P [L, L]; dtype-generic (fp64 for parity, fp32 for the tests' bound)."""
    A = scale_tril(qpre)
    P = scale_tril(ppre)
    z = qloc.unsqueeze(0) + torch.einsum("bij,sbj->sbi", A, eps)
    # log q at its own sample: A^-1 (z - loc) IS eps.  (Solving for it again
    # is the same number on paper and loses everything once an A_ii sits at
    # the FLT_MIN clip: the rounding of z - loc is divided by 1e-38.)
    log_q = (-0.5 * (eps * eps).sum(dim=-1)
             - torch.log(torch.diagonal(A, dim1=-2, dim2=-1)).sum(dim=-1)
             - eps.shape[-1] * om.HALF_LOG_2PI)
    klz = log_q - tril_log_prob(z, ploc, P)
    return z, klz, A, P


def parameter_shapes(cfg):
    """``om.gmvae_parameter_shapes`` with the z heads of the full-covariance
    mixture: same slots, scope MULTIVARIATE_GAUSSIAN, LOCATIONS [., L] and
    SCALES [., L (L + 1) / 2]."""
    L = cfg.latent_size
    T = L * (L + 1) // 2
    shapes = OrderedDict()
    for name, shape in om.gmvae_parameter_shapes(cfg).items():
        if "/SOFTPLUS_GAUSSIAN/" in name:
            name = name.replace("SOFTPLUS_GAUSSIAN", SCOPE)
            if "/SOFTPLUS_SCALE/" in name:
                name = name.replace("SOFTPLUS_SCALE", "SCALES")
                shape = shape[:-1] + (T,)
            else:
                name = name.replace("/MEAN/", "/LOCATIONS/")
        shapes[name] = shape
    return shapes


def forward(cfg, params, moving, x, t, eps, training, warm_up_weight=1.0,
            new_moving=None, dropout=None):
    """``eps``: [K, S, B, L].  Keys of ``om.gmvae_forward`` plus
    ``p_z_covariances`` / ``q_z_covariances`` [K, L, L]."""
    bn = cfg.minibatch_normalisation
    H = list(cfg.hidden_sizes)
    K, L = cfg.n_clusters, cfg.latent_size
    B = x.shape[0]
    S = cfg.n_iw * cfg.n_mc
    assert cfg.prior_probabilities_method == "uniform"

    if not training:
        dropout = None
    hy = om._layers(x, params, "Y/CATEGORICAL/ENCODER", H, bn, training,
                    moving, new_moving, dropout=dropout)
    logits = om.dense_layer(hy, params, "Y/CATEGORICAL/LOGITS", False,
                            training, moving, None, activation=False,
                            dropout=dropout)
    log_y = torch.log_softmax(logits, dim=-1)
    y = torch.exp(log_y)
    entropy = -(y * log_y).sum(dim=-1)
    p_y_entropy = math.log(K)
    kl_y_cell = p_y_entropy - entropy

    q_loc_scope = "Z/Q/" + SCOPE + "/LOCATIONS"
    q_scale_scope = "Z/Q/" + SCOPE + "/SCALES"
    p_loc_scope = "Z/P/" + SCOPE + "/LOCATIONS"
    p_scale_scope = "Z/P/" + SCOPE + "/SCALES"
    Wpl = params[p_loc_scope + "/DENSE/weights"]
    bpl = params[p_loc_scope + "/DENSE/biases"]
    Wps = params[p_scale_scope + "/DENSE/weights"]
    bps = params[p_scale_scope + "/DENSE/biases"]

    t_tiled = t.repeat(S, 1)
    kl_z_cell = 0.0
    rec_cell = 0.0
    z_mean = 0.0
    log_p_all = []
    p_z_means, p_z_variances, q_z_means, q_z_variances = [], [], [], []
    p_z_covariances, q_z_covariances = [], []
    for k in range(K):
        dk = None
        if dropout is not None:
            dk = {scope: m[k] for scope, m in dropout.items()
                  if scope.startswith(("Z/", "X/"))}
        h = om._layers(x, params, "Z/Q/ENCODER", H, bn, training, moving,
                       new_moving, extra_row=k, dropout=dk)
        q_loc = om.dense_layer(h, params, q_loc_scope, False, training,
                               moving, None, activation=False, dropout=dk)
        q_pre = om.dense_layer(h, params, q_scale_scope, False, training,
                               moving, None, activation=False, dropout=dk)
        one_hot_l = torch.zeros(K, dtype=Wpl.dtype)
        one_hot_l[k] = 1.0
        one_hot_s = one_hot_l
        if dk and p_loc_scope in dk:
            one_hot_l = one_hot_l * dk[p_loc_scope]
            one_hot_s = one_hot_s * dk[p_scale_scope]
        p_loc = one_hot_l @ Wpl + bpl
        p_pre = one_hot_s @ Wps + bps
        z, klz, A, P = latent_pair(q_loc, q_pre, p_loc, p_pre, eps[k])

        d = z.reshape(S * B, L)
        d = om._layers(d, params, "X/DECODER", H[::-1], bn, training, moving,
                       new_moving, dropout=dk)
        log_prob, _ = om._decoder_distribution(
            cfg, d, params, "X/DISTRIBUTION/", training, moving, dk, None)
        log_p = log_prob(t_tiled).sum(dim=-1).reshape(S, B)
        log_p_all.append(log_p)

        yk = y[:, k]
        kl_z_cell = kl_z_cell + klz.mean(dim=0) * yk
        rec_cell = rec_cell + log_p.mean(dim=0) * yk
        z_mean = z_mean + q_loc * yk.unsqueeze(-1)

        p_cov = P @ P.T
        q_cov = A @ A.transpose(-1, -2)
        p_z_means.append(p_loc)
        # gm:2881-2882: the square of the batch mean of the stddev
        p_z_variances.append(torch.sqrt(torch.diagonal(p_cov)) ** 2)
        q_z_means.append(q_loc.mean(dim=0))
        q_z_variances.append(
            torch.diagonal(q_cov, dim1=-2, dim2=-1).mean(dim=0))
        p_z_covariances.append(p_cov)
        q_z_covariances.append(q_cov.mean(dim=0))

    kl_z = kl_z_cell.mean()
    kl_y = kl_y_cell.mean()
    rec = rec_cell.mean()
    if cfg.free_nats_proportion:
        thr = cfg.free_nats_proportion * p_y_entropy
        kl_y_mod = torch.where(kl_y > thr, kl_y,
                               torch.as_tensor(thr, dtype=kl_y.dtype))
    else:
        kl_y_mod = kl_y
    w = warm_up_weight * cfg.kl_weight
    return {
        "reconstruction_error": rec,
        "kl_divergence_z": kl_z,
        "kl_divergence_y": kl_y,
        "kl_divergence": kl_z + kl_y,
        "lower_bound": rec - (kl_z + kl_y),
        "lower_bound_weighted": rec - w * (kl_z + kl_y_mod),
        "log_p_x_given_z": torch.stack(log_p_all),
        "reconstruction_cell": rec_cell,
        "q_y_logits": logits,
        "q_y_probabilities": y.mean(dim=0),
        "y": y,
        "z_mean": z_mean,
        "p_z_means": torch.stack(p_z_means),
        "p_z_variances": torch.stack(p_z_variances),
        "q_z_means": torch.stack(q_z_means),
        "q_z_variances": torch.stack(q_z_variances),
        "p_z_covariances": torch.stack(p_z_covariances),
        "q_z_covariances": torch.stack(q_z_covariances),
    }


def train_step(cfg, params, moving, state, x, t, eps, learning_rate,
               warm_up_weight=1.0, dropout=None):
    new_moving = {}
    out, grads = om.gradients(
        lambda p: forward(cfg, p, moving, x, t, eps, True, warm_up_weight,
                          new_moving, dropout), params)
    params = om.clip_and_adam(params, grads, state, learning_rate)
    moving = OrderedDict((k, new_moving.get(k, v)) for k, v in moving.items())
    return params, moving, out, grads
