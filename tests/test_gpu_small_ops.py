"""The small ops of the graph through their stand-alone C-ABI entries
(include/scvae_hip.h, "the small ops of the graph") against
the oracle's fp64 restatement (``oracle/models.py``: ``dense_layer``'s batch
norm, ``_normal_log_prob``, the KL_y block, ``log_reduce_exp_mean``;
``oracle/likelihoods.py``: ``mean_variance``) with autograd for the backward
entries.  Reference: mu:60-76, 129-137; du:52-73; gm:2936-3048, 3242-3261,
3272-3292; va:2665-2734."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import likelihoods as lk
from oracle import models as om
from _parity import close_elementwise, close_maxnorm, close_scalar
import _mixture_oracle as mo

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(device)


def _close(got, want, rtol, what):
    got = got.detach().cpu().double().numpy()
    want = np.asarray(want.detach().numpy() if hasattr(want, "detach") else want,
                      dtype=np.float64)
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max() / scale
    assert np.isfinite(got).all() and err <= rtol, (what, err)


@pytest.mark.parametrize("rows,N", [(100, 100), (4096, 100), (37, 7), (1000, 128)])
@pytest.mark.parametrize("relu", [0, 1])
def test_batch_norm_stats_apply_and_backward(cuda_device, rows, N, relu):
    from scvae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(rows + N + relu)
    a = rng.normal(0.3, 2.0, (rows, N))
    beta = rng.normal(0, 0.5, N)
    dh = rng.normal(0, 1, (rows, N))
    ad, bd, dhd = _dev(a, cuda_device), _dev(beta, cuda_device), _dev(dh, cuda_device)
    ws = torch.empty(int(lib.scvae_bn_workspace_floats(N)) + 2 * N, device=cuda_device)
    mean = torch.empty(N, device=cuda_device)
    var = torch.empty(N, device=cuda_device)
    h = torch.empty(rows, N, device=cuda_device)
    da = torch.empty(rows, N, device=cuda_device)
    dbeta = torch.empty(N, device=cuda_device)
    _lib.check(lib.scvae_bn_stats(_p(ad), N, rows, N, _p(mean), _p(var), _p(ws), _stream()),
               "bn_stats")
    _lib.check(lib.scvae_bn_apply_relu_fwd(_p(ad), N, _p(mean), _p(var), _p(bd), _p(h), N,
                                           rows, N, relu, _stream()), "bn_apply_fwd")
    _lib.check(lib.scvae_bn_apply_relu_bwd(_p(dhd), N, _p(h), N, _p(ad), N, _p(mean), _p(var),
                                           rows, N, relu, _p(da), N, _p(dbeta), _p(ws),
                                           _stream()), "bn_apply_bwd")
    torch.cuda.synchronize()
    # oracle: dense_layer with an identity affine map (mu:53-76)
    at = torch.from_numpy(a).requires_grad_(True)
    bt = torch.from_numpy(beta).requires_grad_(True)
    params = {"S/DENSE/weights": torch.eye(N, dtype=torch.float64),
              "S/DENSE/biases": torch.zeros(N, dtype=torch.float64),
              "S/BATCH_NORM/beta": bt}
    moving = {"S/BATCH_NORM/moving_mean": torch.zeros(N, dtype=torch.float64),
              "S/BATCH_NORM/moving_variance": torch.ones(N, dtype=torch.float64)}
    out = om.dense_layer(at, params, "S", True, True, moving, None, activation=bool(relu))
    (out * torch.from_numpy(dh)).sum().backward()
    _close(mean, at.detach().mean(dim=0), 1e-5, "mean")
    _close(var, at.detach().var(dim=0, unbiased=False), 1e-5, "var")
    _close(h, out, 2e-6, "h")
    # (a unit within rounding of the ReLU kink may fall on the other side in fp32)
    before = om.dense_layer(at.detach(), {k: v.detach() for k, v in params.items()}, "S",
                            True, True, moving, None, activation=False)
    live = before.abs() > 1e-5
    assert live.double().mean() > 0.99
    _close(da * live.to(cuda_device), at.grad * live, 5e-4 if relu else 2e-5, "da")
    _close(dbeta, bt.grad, 5e-4 if relu else 2e-5, "dbeta")


# The longest chain of fp32 roundings a value passes through in the chunked
# sums of scvae_bn_stats for up to 5000 rows (elementwise.hip: at most 5 + 16
# additions within a chunk, a division, 4 + 16 across the chunks, a division: 43)
BN_SUM_ROUNDINGS = 48
U32 = 2.0 ** -24


@pytest.mark.parametrize("rows", [37, 4096, 5000])
def test_batch_norm_stats_under_cancellation(cuda_device, rows):
    """Columns whose mean dwarfs their spread, constant columns and a single
    spike, against the fp64 statistics of the fp32-ROUNDED inputs (fp32 holds
    1e4 to 1e-3: the unrounded oracle would be a different column).

    With u = 2^-24, k = BN_SUM_ROUNDINGS and A = mean |x| of a column:
      mean: a sum of terms of magnitude A through at most k roundings:
            |d mean| <= k u A =: D  (a few ulps of the mean where A = |mean|)
      var:  the kernel centres every chunk on its own mean and merges with
            M2 + n (mean_c - mean)^2.  A chunk mean off by d_c leaves
            sum (x - mean_c - d_c)^2 = M2_c + n d_c^2 (the cross term vanishes)
            and moves the merge term by 2 n d_c (mean_c - mean) + n d_c^2; the
            global mean's own error D adds as much again.  Over the chunks,
            with mean_c |mean_c - mean| <= sigma:
            |d var| <= 2 D sigma + 4 D^2 + k u var
            (the last term: the roundings of the sums of squares, all positive).
    Nothing in it grows with mean^2.  A one-pass E[x^2] - E[x]^2 loses
    mean^2 u ~ 6 on the first column and 0.5 on the second, against bounds of
    about 0.05 and 1e-3."""
    from scvae_amd import _lib
    lib = _lib.load()
    N = 7
    rng = np.random.default_rng(rows)
    a = np.zeros((rows, N))
    a[:, 0] = rng.normal(1e4, 1.0, rows)
    a[:, 1] = rng.normal(-3e3, 0.05, rows)
    a[:, 2] = 2.5        # (every partial sum and the quotient exact: var == 0)
    a[:, 3] = 0.0
    a[:, 4] = rng.normal(0.0, 1.0, rows)
    a[rows // 3, 5] = 1000.0
    a[:, 6] = rng.normal(0.3, 2.0, rows)
    a32 = a.astype(np.float32)
    beta = rng.normal(0, 0.5, N).astype(np.float32)
    ad = torch.from_numpy(a32).to(cuda_device)
    bd = torch.from_numpy(beta).to(cuda_device)
    ws = torch.empty(int(lib.scvae_bn_workspace_floats(N)), device=cuda_device)
    mean = torch.empty(N, device=cuda_device)
    var = torch.empty(N, device=cuda_device)
    h = torch.empty(rows, N, device=cuda_device)
    _lib.check(lib.scvae_bn_stats(_p(ad), N, rows, N, _p(mean), _p(var), _p(ws), _stream()),
               "bn_stats")
    _lib.check(lib.scvae_bn_apply_relu_fwd(_p(ad), N, _p(mean), _p(var), _p(bd), _p(h), N,
                                           rows, N, 0, _stream()), "bn_apply_fwd")
    torch.cuda.synchronize()
    x = a32.astype(np.float64)
    want_mean, want_var = x.mean(axis=0), x.var(axis=0)
    D = BN_SUM_ROUNDINGS * U32 * np.abs(x).mean(axis=0)
    var_tol = 2 * D * np.sqrt(want_var) + 4 * D * D + BN_SUM_ROUNDINGS * U32 * want_var
    got_mean, got_var = mean.cpu().double().numpy(), var.cpu().double().numpy()
    print("bn_stats rows={}: mean err / bound {}, var err / bound {}".format(
        rows, np.abs(got_mean - want_mean) / np.maximum(D, 1e-300),
        np.abs(got_var - want_var) / np.maximum(var_tol, 1e-300)))
    for c in range(N):
        close_scalar(got_mean[c], want_mean[c], rtol=0.0, atol=D[c],
                     what="mean of column {}".format(c))
        close_scalar(got_var[c], want_var[c], rtol=0.0, atol=var_tol[c],
                     what="variance of column {}".format(c))
    assert (got_var >= 0).all()
    # the constant columns: mean exact, variance exactly 0, the output beta
    assert got_mean[2] == 2.5 and got_mean[3] == 0.0
    assert got_var[2] == 0.0 and got_var[3] == 0.0
    hh = h.cpu().numpy()
    assert (hh[:, 2] == beta[2]).all() and (hh[:, 3] == beta[3]).all()
    # the normalisation on the statistics THE DEVICE holds: a - mean (1
    # rounding), var + 1e-3 (1, halved by the root), the reciprocal root (the
    # hardware's v_rsq_f32: 1 ulp = 2 u), the multiply-add (1): 5 u of
    # |a - mean| / sqrt(var + 1e-3) + |beta|, allowed twice
    istd = 1.0 / np.sqrt(got_var + np.float64(np.float32(om.BN_EPSILON)))
    want_h = (x - got_mean) * istd + beta.astype(np.float64)
    mag = np.abs(x - got_mean) * istd + np.abs(beta.astype(np.float64))
    close_elementwise((hh.astype(np.float64) - want_h) / np.maximum(mag, 1e-300),
                      np.zeros_like(want_h), rtol=0.0, atol=2 * 5 * U32,
                      what="h relative to its terms")


@pytest.mark.parametrize("K,S,B,L", [(3, 1, 48, 5), (20, 2, 64, 100), (2, 3, 7, 130)])
def test_softplus_gaussian_logprob_pair(cuda_device, K, S, B, L):
    from scvae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(K * 100 + L)
    arrays = dict(qm=rng.normal(0, 1, (K * B, L)), qs=rng.normal(0, 1.5, (K * B, L)),
                  Wpm=rng.normal(0, 1, (K, L)), bpm=rng.normal(0, 0.3, L),
                  Wps=rng.normal(0, 1, (K, L)), bps=rng.normal(0, 0.3, L),
                  eps=rng.normal(0, 1, (K, S, B, L)),
                  dz=rng.normal(0, 1, (K, S, B, L)), gklz=rng.normal(0, 1, (K, S, B)))
    d = {k: _dev(v, cuda_device) for k, v in arrays.items()}
    z = torch.empty(K, S, B, L, device=cuda_device)
    klz = torch.empty(K, S, B, device=cuda_device)
    qvar = torch.empty(K * B, L, device=cuda_device)
    _lib.check(lib.scvae_softplus_gaussian_logprob_pair_fwd(
        _p(d["qm"]), _p(d["qs"]), _p(d["Wpm"]), _p(d["bpm"]), _p(d["Wps"]), _p(d["bps"]),
        _p(d["eps"]), _p(z), _p(klz), _p(qvar), K, S, B, L, _stream()), "pair_fwd")
    dqm = torch.empty(K * B, L, device=cuda_device)
    dqs = torch.empty(K * B, L, device=cuda_device)
    dpr = torch.empty(K * B, 2 * L, device=cuda_device)
    _lib.check(lib.scvae_softplus_gaussian_logprob_pair_bwd(
        _p(d["qm"]), _p(d["qs"]), _p(d["Wpm"]), _p(d["bpm"]), _p(d["Wps"]), _p(d["bps"]),
        _p(d["eps"]), _p(d["dz"]), _p(d["gklz"]), _p(dqm), _p(dqs), _p(dpr), K, S, B, L,
        _stream()), "pair_bwd")
    torch.cuda.synchronize()
    t = {k: torch.from_numpy(v).requires_grad_(k in ("qm", "qs", "Wpm", "Wps", "bpm", "bps"))
         for k, v in arrays.items()}
    # du:52-73: sigma = sqrt(softplus(s)); gm:3272-3292: sum_L log q(z) - log p(z)
    sigma = torch.sqrt(torch.nn.functional.softplus(t["qs"])).reshape(K, 1, B, L)
    mean = t["qm"].reshape(K, 1, B, L)
    zz = mean + sigma * t["eps"]
    pm = (t["Wpm"] + t["bpm"]).reshape(K, 1, 1, L)
    ps = torch.sqrt(torch.nn.functional.softplus(t["Wps"] + t["bps"])).reshape(K, 1, 1, L)
    want_kl = (om._normal_log_prob(zz, mean, sigma)
               - om._normal_log_prob(zz, pm, ps)).sum(dim=-1)
    ((zz * t["dz"]).sum() + (want_kl * t["gklz"]).sum()).backward()
    # every element against fp64 on the fp32 inputs the device holds, each on the
    # bound mo.pair derives from its own terms (dprior per cell, not summed)
    held, _ = mo.pair({k: v.astype(np.float32) for k, v in arrays.items()}, K, S, B, L)
    for name, got in (("z", z), ("klz", klz), ("qvar", qvar), ("dqm", dqm), ("dqs", dqs),
                      ("dpr", dpr)):
        mo.hold("{} [K {} S {} B {} L {}]".format(name, K, S, B, L), got, held[name])
    # (and the per-tensor bounds these cases had before)
    _close(z, zz, 1e-6, "z")
    _close(klz, want_kl, 2e-5, "klz")
    _close(qvar, (sigma ** 2).reshape(K * B, L), 1e-6, "qvar")
    _close(dqm, t["qm"].grad, 5e-5, "dqm")
    _close(dqs, t["qs"].grad, 5e-5, "dqs")
    per = dpr.reshape(K, B, 2 * L).sum(dim=1)        # summed over the cells: the Z/P rows
    _close(per[:, :L], t["Wpm"].grad, 1e-4, "d prior mean rows")
    _close(per[:, L:], t["Wps"].grad, 1e-4, "d prior scale rows")


@pytest.mark.parametrize("B,K", [(100, 20), (7, 3), (513, 64)])
@pytest.mark.parametrize("prior", ["uniform", "learned"])
def test_categorical_entropy_kl(cuda_device, B, K, prior):
    from scvae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(B + K)
    logits = rng.normal(0, 2, (B, K))
    dy = rng.normal(0, 1, (B, K))
    pl = rng.normal(0, 1, K) if prior == "learned" else None
    ld, dyd = _dev(logits, cuda_device), _dev(dy, cuda_device)
    pld = _dev(pl, cuda_device) if pl is not None else None
    y = torch.empty(B, K, device=cuda_device)
    kl = torch.empty(B, device=cuda_device)
    _lib.check(lib.scvae_categorical_entropy_kl_fwd(_p(ld), _p(y), _p(kl), B, K, _p(pld),
                                                    _stream()), "cat_fwd")
    c = 0.37
    gate = torch.ones(1, device=cuda_device)
    dl = torch.empty(B, K, device=cuda_device)
    _lib.check(lib.scvae_categorical_entropy_kl_bwd(_p(y), _p(dyd), _p(gate), c, _p(dl), B, K,
                                                    _p(pld), _stream()), "cat_bwd")
    gate0 = torch.zeros(1, device=cuda_device)
    dl0 = torch.empty(B, K, device=cuda_device)
    _lib.check(lib.scvae_categorical_entropy_kl_bwd(_p(y), _p(dyd), _p(gate0), c, _p(dl0), B, K,
                                                    _p(pld), _stream()), "cat_bwd")
    torch.cuda.synchronize()
    lt = torch.from_numpy(logits).requires_grad_(True)
    log_y = torch.log_softmax(lt, dim=-1)
    yt = torch.exp(log_y)
    if pl is None:       # gm:3242-3254: log K - H[q(y|x)]
        want_kl = math.log(K) + (yt * log_y).sum(dim=-1)
    else:                # gm:3256-3258: kl(q_y || p_y)
        log_p = torch.log_softmax(torch.from_numpy(pl), dim=-1)
        want_kl = (yt * (log_y - log_p)).sum(dim=-1)
    # every element against fp64 on the fp32 inputs the device holds, on the bounds
    # mo.categorical_fwd / mo.categorical_bwd derive (the backward on the device's y)
    l32, d32 = logits.astype(np.float32), dy.astype(np.float32)
    p32 = None if pl is None else pl.astype(np.float32)
    held, _ = mo.categorical_fwd(l32, p32)
    tag = " [B {} K {} {}]".format(B, K, prior)
    mo.hold("y" + tag, y, held["y"])
    mo.hold("kl_y_cell" + tag, kl, held["kl"])
    y_dev = y.cpu().numpy()
    mo.hold("dlogits gate 1" + tag, dl, mo.categorical_bwd(y_dev, d32, 1.0, c, p32))
    mo.hold("dlogits gate 0" + tag, dl0, mo.categorical_bwd(y_dev, d32, 0.0, c, p32))
    # (and the per-tensor bounds these cases had before)
    _close(y, yt, 1e-6, "y")
    _close(kl, want_kl, 2e-5, "kl_y")
    ((yt * torch.from_numpy(dy)).sum() + c * want_kl.sum()).backward()
    _close(dl, lt.grad, 5e-5, "dlogits (gate on)")
    lt2 = torch.from_numpy(logits).requires_grad_(True)
    (torch.softmax(lt2, dim=-1) * torch.from_numpy(dy)).sum().backward()
    _close(dl0, lt2.grad, 5e-5, "dlogits (gate off)")


def _iw_inputs(n_iw, n_mc, B, per_sample, spread=None):
    rng = np.random.default_rng(n_iw * 10 + n_mc + B)
    ll = rng.normal(-300, 30, (n_iw, n_mc, B))
    if spread is not None:      # importance samples nats apart
        ll = ll + np.asarray(spread, dtype=np.float64).reshape(n_iw, 1, 1)
    kl = rng.gamma(2.0, 2.0, (n_iw, n_mc, B) if per_sample else (B,))
    # (as the fp32 values the device holds)
    return (ll.astype(np.float32).astype(np.float64),
            kl.astype(np.float32).astype(np.float64))


def _iw_oracle(ll, kl, per_sample, w):
    """va:2717-2734 with mu:129-137 (log_reduce_exp_mean over the importance
    samples): the four means and d(-lower_bound_weighted) / d ll."""
    B = ll.shape[-1]
    lt = torch.from_numpy(ll).requires_grad_(True)
    kt = torch.from_numpy(kl)
    kk = kt if per_sample else kt.reshape(1, 1, B)
    lb = om.log_reduce_exp_mean(lt - kk, 0).mean()
    lbw = om.log_reduce_exp_mean(lt - w * kk, 0).mean()
    (-lbw).backward()
    return lb.item(), lbw.item(), ll.mean(), kl.mean(), lt.grad


def _iw_run(device, ll, kl, per_sample, w, row_scale, with_gw, scalars=None):
    from scvae_amd import _lib
    lib = _lib.load()
    n_iw, n_mc, B = ll.shape
    lld, kld = _dev(ll, device), _dev(kl, device)
    if scalars is None:
        scalars = torch.zeros(8, device=device)
    gw = torch.full((n_iw * n_mc * B,), float("nan"), device=device) if with_gw else None
    _lib.check(lib.scvae_iw_logmeanexp(_p(lld), _p(kld), per_sample, n_iw, n_mc, B, w,
                                       row_scale, _p(scalars), _p(gw), _stream()),
               "iw_logmeanexp")
    torch.cuda.synchronize()
    return scalars, gw


@pytest.mark.parametrize("n_iw,n_mc,B,per_sample", [
    (1, 1, 100, 0), (5, 1, 64, 0), (3, 2, 50, 1), (4, 3, 1000, 0), (2, 1, 4096, 1)])
def test_iw_logmeanexp(cuda_device, n_iw, n_mc, B, per_sample):
    from scvae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n_iw * 10 + n_mc + B)
    S = n_iw * n_mc
    ll = rng.normal(-300, 30, (n_iw, n_mc, B))
    kl = rng.gamma(2.0, 2.0, (n_iw, n_mc, B) if per_sample else (B,))
    w = 0.6
    lld, kld = _dev(ll, cuda_device), _dev(kl, cuda_device)
    scalars = torch.zeros(8, device=cuda_device)
    gw = torch.empty(S * B, device=cuda_device)
    _lib.check(lib.scvae_iw_logmeanexp(_p(lld), _p(kld), per_sample, n_iw, n_mc, B, w,
                                       1.0 / (n_mc * B), _p(scalars), _p(gw), _stream()),
               "iw_logmeanexp")
    torch.cuda.synchronize()
    lt = torch.from_numpy(ll).requires_grad_(True)
    kt = torch.from_numpy(kl)
    kk = kt if per_sample else kt.reshape(1, 1, B)
    # va:2717-2734 with mu:129-137 (log_reduce_exp_mean over the importance samples)
    lb = om.log_reduce_exp_mean(lt - kk, 0).mean()
    lbw = om.log_reduce_exp_mean(lt - w * kk, 0).mean()
    (-lbw).backward()
    s = scalars.cpu().double().numpy()
    assert abs(s[0] - lb.item()) <= 2e-6 * abs(lb.item())
    assert abs(s[1] - lbw.item()) <= 2e-6 * abs(lbw.item())
    assert abs(s[2] - ll.mean()) <= 2e-6 * abs(ll.mean())
    assert abs(s[3] - kl.mean()) <= 1e-5 * abs(kl.mean())
    _close(gw.reshape(n_iw, n_mc, B), lt.grad, 2e-5, "gw")


def _iw_hold_scalars(scalars, want, share, what):
    """The bounds of ``test_iw_logmeanexp``: 2e-6 relative, 1e-5 for the KL
    mean; a rank holding 1 / ``share`` of the global minibatch emits that share
    of the means."""
    s = scalars.cpu().double().numpy()
    assert np.isfinite(s[:4]).all(), what
    for i, (name, rtol) in enumerate((("lower_bound", 2e-6), ("lower_bound_weighted", 2e-6),
                                      ("reconstruction_error", 2e-6),
                                      ("kl_divergence", 1e-5))):
        close_scalar(s[i], want[i] / share, rtol=rtol, what="{} {}".format(what, name))
    assert s[7] == 0.0, what


# (n_iw, n_mc, B, per_sample, with a gw buffer).  Without one and with n_iw = 1
# and the analytic KL the kernel takes the training step's path: eight loads in
# flight per thread, 8192 pairs per trip -- (1, 3, 4096) and (1, 2, 4500) make a
# second trip with a partly clamped tail, and B < pairs keeps the KL sum to the
# first B pairs.  The others run the general loop: B = 1, 1024 mod B != 0, more
# pairs than threads, with and without the gradient.
IW_CASES = [
    (1, 1, 1, 0, False), (1, 1, 100, 0, False), (1, 3, 4096, 0, False),
    (1, 2, 4500, 0, False), (3, 2, 1500, 0, False), (3, 2, 1500, 1, False),
    (3, 2, 1500, 0, True), (3, 2, 1500, 1, True), (2, 1, 1, 0, True),
    (2, 1, 1, 1, True), (4, 1, 700, 0, True)]


@pytest.mark.parametrize("share", [1, 3], ids=["whole", "third"])
@pytest.mark.parametrize("w", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("n_iw,n_mc,B,per_sample,with_gw", IW_CASES)
def test_iw_logmeanexp_paths(cuda_device, n_iw, n_mc, B, per_sample, with_gw, w, share):
    ll, kl = _iw_inputs(n_iw, n_mc, B, per_sample)
    row_scale = 1.0 / (n_mc * share * B)
    scalars, gw = _iw_run(cuda_device, ll, kl, per_sample, w, row_scale, with_gw)
    want = _iw_oracle(ll, kl, per_sample, w)
    _iw_hold_scalars(scalars, want, share, "iw {} mc {} B {}".format(n_iw, n_mc, B))
    if with_gw:     # (test_iw_logmeanexp's bound)
        close_maxnorm(gw.reshape(n_iw, n_mc, B), want[4] / share, rtol=2e-5, what="gw")


@pytest.mark.parametrize("w", [0.0, 0.6, 1.0])
def test_iw_logmeanexp_samples_far_apart(cuda_device, w):
    """Importance samples 50 to 1000 nats apart: the winner takes the weight.
    Every weight is compared on its own.  With a = ll - w kl (of size up to
    1300, where an fp32 ulp is 1.2e-4) and weight_r = exp(a_r - max a) / sum:
    a_r carries two roundings of |w kl| + |a_r|, and so does the winner's,
    which the sum inherits; the argument a_r - max a rounds once and the fast
    exponential scales its argument by log2(e) in fp32 (2 more of |arg|); the
    exponential itself, the sum, the division and the scale about 6 more:
      |d weight_r| / weight_r <= u (2 (|a_r| + |w kl|) + 2 (|a_max| + |w kl|)
                                    + 3 |a_r - a_max| + 6),  allowed twice,
    plus one fp32 ulp of the winner's weight (row_scale, at most) as the
    absolute term: 0 is a correct fp32 answer for e^-400."""
    n_iw, n_mc, B = 5, 1, 64
    ll, kl = _iw_inputs(n_iw, n_mc, B, 0, spread=[0, -50, -200, -400, -1000])
    row_scale = 1.0 / (n_mc * B)
    scalars, gw = _iw_run(cuda_device, ll, kl, 0, w, row_scale, True)
    want = _iw_oracle(ll, kl, 0, w)
    _iw_hold_scalars(scalars, want, 1, "far apart")
    g = want[4].numpy()
    assert (np.abs(g).argmax(axis=0) == 0).mean() > 0.5      # (sample 0 mostly wins)
    wkl = np.abs(w * kl).reshape(1, 1, B)
    a = ll - w * kl.reshape(1, 1, B)
    top = a.max(axis=0, keepdims=True)
    rel = 2 * U32 * (2 * (np.abs(a) + wkl) + 2 * (np.abs(top) + wkl)
                     + 3 * np.abs(a - top) + 6)
    got = gw.reshape(n_iw, n_mc, B).cpu().double().numpy()
    assert np.isfinite(got).all()
    excess = np.abs(got - g) - (rel * np.abs(g) + row_scale * 2.0 ** -23)
    assert excess.max() <= 0, (np.unravel_index(excess.argmax(), excess.shape),
                               excess.max())


@pytest.mark.parametrize("with_gw", [False, True], ids=["step-path", "general-path"])
def test_iw_logmeanexp_counts_non_finite_bounds(cuda_device, with_gw):
    """scalars[7] counts the calls since the caller zeroed it whose bound was
    not finite (plain float arithmetic on a -inf log-likelihood)."""
    ll, kl = _iw_inputs(1, 2, 300, 0)
    bad = ll.copy()
    bad[0, 1, 17] = -np.inf
    scalars = torch.zeros(8, device=cuda_device)
    want = _iw_oracle(ll, kl, 0, 0.6)
    for values, count in ((ll, 0.0), (bad, 1.0), (bad, 2.0), (ll, 2.0)):
        _iw_run(cuda_device, values, kl, 0, 0.6, 1.0 / 600, with_gw, scalars)
        s = scalars.cpu().double().numpy()
        assert s[7] == count, (s[7], count)
        if values is ll:
            close_scalar(s[0], want[0], rtol=2e-6, what="lower_bound")
        else:
            assert not np.isfinite(s[0])


@pytest.mark.parametrize("likelihood", ["poisson", "negative binomial",
                                        "zero-inflated negative binomial"])
@pytest.mark.parametrize("S,B,F", [(1, 50, 300), (4, 20, 1000)])
def test_pxmean_stats(cuda_device, likelihood, S, B, F):
    from scvae_amd import _lib
    lib = _lib.load()
    kind, heads = _lib.LIKELIHOOD_KINDS[likelihood]
    rng = np.random.default_rng(S + B + F + kind)
    pre = [rng.normal(0, 1.5, (S * B, F)) for _ in heads]
    pred = [_dev(v, cuda_device) for v in pre]
    arr = (ctypes.c_void_p * len(pred))(*[t.data_ptr() for t in pred])
    weight = rng.random(B)
    wd = _dev(weight, cuda_device)
    outs = [torch.zeros(B, F, device=cuda_device) for _ in range(3)]
    _lib.check(lib.scvae_pxmean_stats(kind, arr, S, B, F, None, 0, 0, _p(outs[0]), _p(outs[1]),
                                      _p(outs[2]), _stream()), "pxmean_stats")
    acc = [torch.ones(B, F, device=cuda_device) for _ in range(3)]
    _lib.check(lib.scvae_pxmean_stats(kind, arr, S, B, F, _p(wd), 1, 1, _p(acc[0]), _p(acc[1]),
                                      _p(acc[2]), _stream()), "pxmean_stats (mixture)")
    torch.cuda.synchronize()
    mean, var = lk.mean_variance(likelihood, tuple(torch.from_numpy(v) for v in pre))
    mean, var = mean.reshape(S, B, F), var.reshape(S, B, F)
    # va:2665-2713: mean over the samples, mean of the variances, variance of the means
    _close(outs[0], mean.mean(dim=0), 2e-5, "p_x_mean")
    _close(outs[1], var.mean(dim=0), 2e-5, "mean of var")
    if S > 1:
        _close(outs[2], ((mean - mean.mean(dim=0)) ** 2).mean(dim=0), 2e-4, "var of mean")
    else:   # one sample: zero up to the rounding of (m - 1.0 * m)
        assert (outs[2].cpu().double() <= 1e-12 * (mean[0] ** 2 + 1e-30)).all()
    # gm:3311-3386: the cluster's share y_k times the statistics, the variance taken about the
    # ALREADY WEIGHTED mean (gm:3357-3368, reproduced), accumulated over the clusters
    wt = torch.from_numpy(weight).reshape(B, 1)
    pm = mean.mean(dim=0) * wt
    _close(acc[0], 1.0 + pm, 2e-5, "weighted p_x_mean")
    _close(acc[1], 1.0 + var.mean(dim=0) * wt, 2e-5, "weighted mean of var")
    _close(acc[2], 1.0 + ((mean - pm) ** 2).mean(dim=0) * wt, 2e-4, "weighted var of mean")
