"""The GMVAE mixture stage (scvae_amd/csrc/gmvae_kernels.hip) through its
stand-alone C-ABI entries, held to fp64 ELEMENT BY ELEMENT at the shapes where
the kernels branch and in the regimes where the formulation is ill-conditioned.

Every comparison is ``|got - want| <= bound(element)`` (``_mixture_oracle.hold``)
with ``want`` and ``bound`` from tests/_mixture_oracle.py, where each bound is
derived in the docstring of its oracle from the roundings the kernel performs
(u = 2^-24, the intrinsics at the accuracy common.hpp states, the u max|logit|
term of lse carried into every log-probability, the total allowed twice).  The
``check_*`` functions there hold the asserts; tests/test_mixture_oracle_host.py
takes a NumPy fp32 evaluation of the same formulation through the same
functions on the same inputs.  Each test prints err / bound per output.

  categorical:  one wave per cell strided over K -- K = 65, 129, 200 make a second,
                third and fourth pass; four cells share a block, B % 4 != 0 leaves
                idle waves; near-uniform q (KL_y a difference of two log K), peaked
                q with y through the subnormal range to 0
  pair:         ceil(L/64) waves summed through LDS once per sample; scales from
                e^-40 to 9; the clip at +-FLOAT32_MAX / 2; K B L > 2048 * 256
  mixture ELBO: the eight-pass unroll with its clamped tail (S = 1) and the
                plain loop (S > 1); B past one pass of 256 threads; B K > 1024 * 256;
                the free-nats gate on both sides, per prior kind; the sticky counter
  group ops:    R past 64 chunks of 256 rows, lda > N, past 2048 * 256 elements
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import models as om
from _parity import ELBO_RTOL, close_elementwise, close_per_tensor, close_scalar

import _mixture_oracle as mo

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Device:
    """The entries on the GPU: NumPy fp32 in, NumPy fp32 out."""

    def __init__(self, device):
        from scvae_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.device = device
        self._inputs = []

    def up(self, a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        # (kept until ``down``: a tensor dropped right after its pointer is taken goes
        # back to the allocator, and the next input lands on the same memory)
        self._inputs.append(t)
        return t

    def out(self, *shape):
        # (NaN-filled: an element the kernel leaves unwritten fails its bound)
        return torch.full(shape, float("nan"), device=self.device)

    def call(self, name, *args):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        try:
            self._lib.check(getattr(self.lib, name)(*args, stream), name)
        except Exception as e:      # (nothing more runs on a device that reported an error)
            pytest.exit("{}: {}".format(name, e), returncode=3)

    def down(self, *ts):
        try:
            torch.cuda.synchronize()
            r = [t.cpu().numpy() for t in ts]
        except RuntimeError as e:
            pytest.exit("device error: {}".format(e), returncode=3)
        self._inputs.clear()
        return r[0] if len(r) == 1 else r

    def cat_fwd(self, logits, prior):
        B, K = logits.shape
        y, kl = self.out(B, K), self.out(B)
        self.call("scvae_categorical_entropy_kl_fwd", _p(self.up(logits)), _p(y), _p(kl), B, K,
                  _p(self.up(prior)))
        return self.down(y, kl)

    def cat_bwd(self, y, dy, gate, c, prior):
        B, K = y.shape
        dl = self.out(B, K)
        self.call("scvae_categorical_entropy_kl_bwd", _p(self.up(y)), _p(self.up(dy)),
                  _p(self.up(np.array([gate]))), c, _p(dl), B, K, _p(self.up(prior)))
        return self.down(dl)

    def prior_bwd(self, y, prior, gate, c, off_scale, free_nats):
        B, K = y.shape
        dp = self.out(K)
        self.call("scvae_prior_logits_bwd", _p(self.up(y)), _p(self.up(prior)),
                  _p(self.up(np.array([gate]))), c, off_scale, free_nats, B, K, _p(dp))
        return self.down(dp)

    def pair(self, arrays, K, S, B, L):
        d = {k: self.up(v) for k, v in arrays.items()}
        z, klz, qvar = self.out(K, S, B, L), self.out(K, S, B), self.out(K, B, L)
        ins = [_p(d[k]) for k in ("qm", "qs", "Wpm", "bpm", "Wps", "bps", "eps")]
        self.call("scvae_softplus_gaussian_logprob_pair_fwd", *ins, _p(z), _p(klz), _p(qvar),
                  K, S, B, L)
        dqm, dqs, dpr = self.out(K, B, L), self.out(K, B, L), self.out(K, B, 2 * L)
        self.call("scvae_softplus_gaussian_logprob_pair_bwd", *ins, _p(d["dz"]), _p(d["gklz"]),
                  _p(dqm), _p(dqs), _p(dpr), K, S, B, L)
        return dict(zip(("z", "klz", "qvar", "dqm", "dqs", "dpr"),
                        self.down(z, klz, qvar, dqm, dqs, dpr)))

    def prior_stats(self, Wpm, bpm, Wps, bps):
        K, L = Wpm.shape
        means, variances = self.out(K, L), self.out(K, L)
        self.call("scvae_prior_stats", _p(self.up(Wpm)), _p(self.up(bpm)), _p(self.up(Wps)),
                  _p(self.up(bps)), K, L, _p(means), _p(variances))
        return self.down(means, variances)

    def elbo_fwd(self, ll, klz, y, kl_y_cell, inv_gb, w, free_nats, share, prior, scalars=None):
        K, S, B = ll.shape
        sums, gate, rec_cell = self.out(3), self.out(1), self.out(B)
        sc = torch.zeros(8, device=self.device) if scalars is None else self.up(scalars)
        self.call("scvae_mixture_elbo_fwd", _p(self.up(ll)), _p(self.up(klz)), _p(self.up(y)),
                  _p(self.up(kl_y_cell)), K, S, B, inv_gb, w, free_nats, share,
                  _p(self.up(prior)), _p(sums), _p(sc), _p(gate), _p(rec_cell))
        sums, sc, gate, rec_cell = self.down(sums, sc, gate, rec_cell)
        return dict(sums=sums, scalars=sc, gate=gate[0], rec_cell=rec_cell)

    def elbo_bwd(self, ll, klz, y, w, inv_gb):
        K, S, B = ll.shape
        gw, gklz, dy = self.out(K, S, B), self.out(K, S, B), self.out(B, K)
        self.call("scvae_mixture_elbo_bwd", _p(self.up(ll)), _p(self.up(klz)), _p(self.up(y)),
                  K, S, B, w, inv_gb, _p(gw), _p(gklz), _p(dy))
        return dict(zip(("gw", "gklz", "dy"), self.down(gw, gklz, dy)))

    def group_col_sum(self, a, R, G, N, scale):
        lda = a.shape[1]
        floats = int(self.lib.scvae_group_col_sum_workspace_floats(G, N))
        assert floats >= 64 * G * N      # (at most 64 row chunks of partial sums)
        ws, out = self.out(floats), self.out(G, N)
        self.call("scvae_group_col_sum", _p(self.up(a)), lda, R, G, N, scale, _p(out), _p(ws))
        return self.down(out)

    def sum_groups(self, a, w, G, R, N):
        out = self.out(R, N)
        self.call("scvae_sum_groups", _p(self.up(a)), _p(self.up(w)), G, G, R, N, _p(out))
        return self.down(out)

    def add_group_rows(self, a0, rows, relu):
        (B, N), K = a0.shape, rows.shape[0]
        out = self.out(K, B, N)
        self.call("scvae_add_group_rows", _p(self.up(a0)), _p(self.up(rows)), _p(out), K, B, N,
                  relu)
        return self.down(out)


@pytest.fixture
def run(cuda_device):
    return Device(cuda_device)


# ---- categorical q(y|x): bounds in mo.categorical_fwd / mo.categorical_bwd ----
@pytest.mark.parametrize("learned", [False, True], ids=["uniform", "learned"])
@pytest.mark.parametrize("K", mo.CAT_K)
def test_categorical_shapes(run, K, learned):
    """K through one to four strided passes, B through whole and partly idle
    blocks of four waves; forward, and the backward with the gate on and off."""
    for B in mo.CAT_B:
        mo.check_categorical(run, K, B, "ordinary", learned)


@pytest.mark.parametrize("learned", [False, True], ids=["uniform", "learned"])
@pytest.mark.parametrize("regime", mo.CAT_REGIMES[1:])
def test_categorical_regimes(run, regime, learned):
    """near-uniform / equal: KL_y = log K - H[q] is of size 1e-9..0 and a
    difference of two log K; held to the bound of its terms and >= -bound.
    spread-20 / spread-60: logits that far apart, row 0 down to 95 and row 1 to
    120 nats below its maximum: every output finite, y to p R_p + FLT_MIN (the
    exponential returns 0 below FLT_MIN, so the bound there is absolute),
    dlogits to its bound in both gate states."""
    for K, B in ((2, 5), (65, 5), (200, 3)):
        mo.check_categorical(run, K, B, regime, learned)


# ---- the softplus-Gaussian pair: bounds in mo.pair ----
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
def test_pair_shapes(run, L):
    for K, S, B, LL in mo.PAIR_SHAPES:
        if LL == L and B <= 7:
            mo.check_pair(run, K, S, B, L)


def test_pair_backward_grid_stride(run):
    """K B L = 546000 > 2048 * 256: the backward's grid-stride loop wraps."""
    K, S, B, L = mo.PAIR_SHAPES[-1]
    assert K * B * L > 2048 * 256
    mo.check_pair(run, K, S, B, L)


def test_pair_scales_far_from_one(run):
    """Scale pre-activations from {-80, -30, 0, 30, 80} mixed within a row:
    -log sg + log sp and g / sg are large terms of opposite sign.  klz against
    c u sum |terms|; dqm, dqs and both halves of dprior per element against
    their own term sums (1 / sg reaches 2e17: a max-norm bound hides every
    other element of dqs)."""
    for K, S, B, L in ((3, 3, 7, 65), (3, 1, 7, 130)):
        info = mo.check_pair(run, K, S, B, L, regime="scales")
        assert info["inv_sg"].max() > 1e17


def test_pair_clip(run):
    """mo.CLIP_ELEMENTS puts +-2e38 and +-inf into qm, qs, Wpm + bpm, Wps + bps
    of cluster 3 (K = 4): z, qvar and prior_stats are the values of the clamped
    inputs, dqm / dqs exactly 0 at the out-of-range elements, and the rows of
    clusters 0..2 keep their ordinary bounds on every output.  klz and the other
    gradients of the rows (3, b) -- a quarter of the rows, by construction --
    are not asserted: fp32 overflows there where fp64 does not."""
    mo.check_pair(run, *mo.CLIP_SHAPE, regime="clip")
    mo.check_prior_stats(run, mo.CLIP_SHAPE[0], mo.CLIP_SHAPE[3], clip=True)
    mo.check_prior_stats(run, 7, 37)      # (K L = 259: past one block, not a multiple)


# ---- the mixture ELBO: bounds in mo.elbo_fwd / mo.elbo_bwd ----
@pytest.mark.parametrize("K,S", [(1, 1), (7, 1), (8, 1), (9, 1), (17, 1), (3, 2), (9, 2)])
def test_mixture_elbo_shapes(run, K, S):
    for KK, SS, B in mo.ELBO_SHAPES:
        if (KK, SS) == (K, S):
            for w in mo.ELBO_WEIGHTS:
                for share in mo.ELBO_SHARES:
                    mo.check_elbo(run, K, S, B, w, share)


def test_mixture_elbo_backward_grid_stride(run):
    K, S, B = mo.ELBO_SHAPES[-1]
    assert B * K > 1024 * 256
    mo.check_elbo(run, K, S, B, 0.6, 1.0)


@pytest.mark.parametrize("prior_kind,side", mo.GATE_CASES)
def test_free_nats_gate(run, prior_kind, side):
    """gate[0], scalars[1] (through scalars), dlogits and dprior in both
    branches, for every kind of prior; with free_nats = 0 the gate is 1.  The
    fp64 KL_y is at least 1e-3 thr from thr (asserted here and on the host)."""
    mo.check_gate(run, prior_kind, side)


def test_prior_logits_gradient_shapes(run):
    for K, B in ((1, 1), (9, 255), (65, 257), (200, 600)):
        mo.check_prior_bwd_shapes(run, K, B)


def test_mixture_elbo_counts_non_finite_bounds(run):
    """scalars[7] counts the calls since the caller zeroed it whose bound was not
    finite; a finite call leaves the count alone."""
    K, S, B = 9, 1, 300
    ll, klz, y, kl_y = mo.elbo_inputs(K, S, B)
    bad = ll.copy()
    bad[4, 0, 17] = -np.inf
    want = mo.elbo_fwd(ll, klz, y, kl_y, 1.0 / B, 0.6, 0.0, 1.0, None)
    scalars = np.zeros(8, dtype=np.float32)
    for values, count in ((ll, 0.0), (bad, 1.0), (bad, 2.0), (ll, 2.0)):
        scalars = run.elbo_fwd(values, klz, y, kl_y, 1.0 / B, 0.6, 0.0, 1.0, None,
                               scalars)["scalars"]
        assert scalars[7] == count, (scalars[7], count)
        if values is ll:
            mo.hold("scalars", scalars[:5], want["scalars"])
        else:
            assert not np.isfinite(scalars[0])


# ---- the group reductions: bounds in mo.group_col_sum / sum_groups / add_group_rows ----
@pytest.mark.parametrize("R,lda,G,N,scale", mo.GROUP_COL_SUM_CASES)
def test_group_col_sum(run, R, lda, G, N, scale):
    mo.check_group_col_sum(run, R, lda, G, N, scale)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_sum_groups(run, weighted):
    mo.check_sum_groups(run, 3, 7, 65, weighted)
    mo.check_sum_groups(run, 3, 4100, 130, weighted)      # R N = 533000 > 2048 * 256


@pytest.mark.parametrize("relu", [0, 1])
def test_add_group_rows(run, relu):
    mo.check_add_group_rows(run, 3, 7, 65, relu)
    mo.check_add_group_rows(run, 3, 1400, 130, relu)      # K B N = 546000 > 2048 * 256


# ---- two whole steps: the entries as the plan wires them, K and L past one wave ----
@pytest.mark.parametrize("method,free_nats", [("uniform", 0.0), ("learn", 0.95)],
                         ids=["uniform", "learned-gate-off"])
def test_gmvae_step_past_one_wave(cuda_device, method, free_nats):
    """A training step at K = 70, L = 70, B = 5 against om.gmvae_train_step.
    Gradients and moving statistics per tensor against their own largest
    magnitude at the rtol of test_gpu_gmvae_step.py (3e-4, 2e-5), the scalars at
    ELBO_RTOL; the biases batch norm cancels and the one-hot rows as there."""
    from scvae_amd.engine import Engine
    F, L, H, B, K = 40, 70, (12,), 5, 70
    eng = Engine(F, L, H, "negative binomial", batch_norm=True, model_type="GMVAE",
                 n_clusters=K, free_nats_proportion=free_nats, device=cuda_device, seed=0,
                 prior_probabilities_method=method)
    g = torch.Generator().manual_seed(1)
    for name, p in eng.named_parameters().items():
        if not name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    cfg = om.ModelConfig(feature_size=F, latent_size=L, hidden_sizes=H,
                         likelihood="negative binomial", n_clusters=K,
                         free_nats_proportion=free_nats, prior_probabilities_method=method)
    params = {k: v.detach().cpu().double() for k, v in eng.named_parameters().items()}
    assert list(params) == list(om.gmvae_parameter_shapes(cfg))
    moving = {k: v.detach().cpu().double() for k, v in eng.named_moving_statistics().items()}
    rng = np.random.default_rng(0)
    x = rng.poisson(rng.gamma(0.5, 3.0, size=(1, F)), size=(B, F)).astype(np.float64)
    x = torch.from_numpy(x * (rng.random((B, F)) > 0.6))
    eps = torch.from_numpy(rng.standard_normal((K, 1, B, L)))
    xd, epsd = x.float().to(cuda_device), eps.float().to(cuda_device)
    logits = torch.zeros(B, K, device=cuda_device)
    zmean = torch.zeros(B, L, device=cuda_device)
    cstats = torch.zeros(4, K, L, device=cuda_device)
    sc = eng.step(xd, xd, eps=epsd, training=True, n_iw=1, n_mc=1, warm_up_weight=0.6,
                  outputs={"q_y_logits": logits, "q_z_mean": zmean,
                           "cluster_stats": cstats}).cpu().numpy()
    torch.cuda.synchronize()
    new_moving = {}
    out, grads = om.gradients(
        lambda p: om.gmvae_forward(cfg, p, moving, x, x, eps, True, 0.6, new_moving), params)
    if free_nats:       # (the branch this case is for)
        assert float(out["kl_divergence_y"]) < free_nats * np.log(K)
    for i, name in enumerate(("lower_bound", "lower_bound_weighted", "reconstruction_error",
                              "kl_divergence_z", "kl_divergence_y")):
        close_scalar(sc[i], out[name], rtol=ELBO_RTOL, what=name)
    # outputs element by element: a logit / a mean of order 1 after a few dozen
    # fp32 products (1e-5 relative), 1e-6 absolute for the elements near 0
    close_elementwise(logits, out["q_y_logits"], rtol=1e-5, atol=1e-6, what="q_y_logits")
    close_elementwise(zmean, out["z_mean"], rtol=1e-5, atol=1e-6, what="q_z_mean")
    for i, name in enumerate(("p_z_means", "p_z_variances", "q_z_means", "q_z_variances")):
        close_elementwise(cstats[i], out[name], rtol=1e-5, atol=1e-6, what=name)
    table = {}
    for name, (offset, shape) in eng.param_table.items():
        if name.endswith("DENSE/biases") and "LAYER_" in name:
            assert eng.gradient(name).abs().max().item() < 1e-5, name
            continue
        if name == "Z/Q/ENCODER/LAYER_1/DENSE/weights":
            assert eng.gradient(name)[F:].abs().max().item() < 1e-5
            shape = (F, shape[1])
        table[name] = (offset, shape)
    want = np.zeros(eng.grads.numel())
    for name, (offset, shape) in eng.param_table.items():
        want[offset:offset + grads[name].numel()] = grads[name].reshape(-1).numpy()
    close_per_tensor(eng.grads, want, table, rtol=3e-4, what="grad")
    want_m = np.zeros(eng.moving.numel())
    for name, (offset, shape) in eng.moving_table.items():
        want_m[offset:offset + new_moving[name].numel()] = new_moving[name].reshape(-1).numpy()
    close_per_tensor(eng.moving, want_m, eng.moving_table, rtol=2e-5, what="moving")
