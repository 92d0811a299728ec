"""GPU parity: the stand-alone "multivariate gaussian" latent pair
(``scvae_mvn_tril_logprob_pair_fwd`` / ``_bwd``, csrc/mvn_tril.hip) against
fp64, tensor by tensor in max-norm relative error.

Bound: an fp32 torch-CPU evaluation of the same formulas on the same inputs has
error e32 against fp64; the kernel may have 8 e32 + 1e-7 (a different summation
order, the device's ``__logf`` / ``__expf``).
"""
import ctypes

import numpy as np
import pytest
import torch

import _fullcov_oracle as fo

pytestmark = pytest.mark.gpu

FLOAT32_TINY = float(np.finfo(np.float32).tiny)
SHAPES = [(1, 1, 1, 1),      # the degenerate triangle
          (3, 2, 37, 6),     # several clusters and samples; B divides nothing
          (2, 1, 37, 25),    # the workload's L, no power of two
          (1, 2, 5, 64)]     # a full wave


def _inputs(K, S, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    T = L * (L + 1) // 2

    def n(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=g,
                                    dtype=torch.float64)).float().double()
    return {
        "qloc": n(K, B, L), "qpre": n(K, B, T, scale=0.3),
        "Wpl": n(K, L), "bpl": n(L, scale=0.1),
        "Wps": n(K, T, scale=0.3), "bps": n(T, scale=0.1),
        "eps": n(K, S, B, L), "dz": n(K, S, B, L, scale=0.1),
        "gklz": n(K, S, B, scale=0.05),
    }


def _reference(inputs, dtype):
    """Every checked tensor from the restated formulas in ``dtype``; the
    gradients by autograd of sum(dz z) + sum(gklz klz)."""
    t = {k: v.to(dtype) for k, v in inputs.items()}
    leaves = {k: t[k].clone().requires_grad_(True)
              for k in ("qloc", "qpre", "Wpl", "bpl", "Wps", "bps")}
    K = t["qloc"].shape[0]
    zs, klzs, qvar, qcov = [], [], [], []
    for k in range(K):
        ploc = leaves["Wpl"][k] + leaves["bpl"]
        ppre = leaves["Wps"][k] + leaves["bps"]
        z, klz, A, P = fo.latent_pair(leaves["qloc"][k], leaves["qpre"][k],
                                      ploc, ppre, t["eps"][k])
        zs.append(z)
        klzs.append(klz)
        cov = A @ A.transpose(-1, -2)
        qcov.append(cov)
        qvar.append(torch.diagonal(cov, dim1=-2, dim2=-1))
    z, klz = torch.stack(zs), torch.stack(klzs)
    loss = (t["dz"] * z).sum() + (t["gklz"] * klz).sum()
    grads = torch.autograd.grad(loss, list(leaves.values()))
    out = {"z": z, "klz": klz, "qvar": torch.stack(qvar),
           "qcov": torch.stack(qcov)}
    for name, g in zip(leaves, grads):
        out["d" + name] = g
    return {k: v.detach().double() for k, v in out.items()}


def _device(inputs, device):
    from scvae_amd import _lib
    lib = _lib.load()
    K, S, B, L = inputs["eps"].shape
    T = L * (L + 1) // 2
    d = {k: v.float().contiguous().to(device) for k, v in inputs.items()}

    def empty(*shape):
        return torch.full(shape, float("nan"), device=device)
    z, klz = empty(K, S, B, L), empty(K, S, B)
    qvar, qcov = empty(K, B, L), empty(K, B, L, L)
    dqloc, dqpre = empty(K, B, L), empty(K, B, T)
    dprior = empty(K, B, L + T)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def p(tensor):
        return ctypes.c_void_p(tensor.data_ptr())
    _lib.check(lib.scvae_mvn_tril_logprob_pair_fwd(
        p(d["qloc"]), p(d["qpre"]), p(d["Wpl"]), p(d["bpl"]), p(d["Wps"]),
        p(d["bps"]), p(d["eps"]), p(z), p(klz), p(qvar), p(qcov), K, S, B, L,
        stream), "scvae_mvn_tril_logprob_pair_fwd")
    _lib.check(lib.scvae_mvn_tril_logprob_pair_bwd(
        p(d["qloc"]), p(d["qpre"]), p(d["Wpl"]), p(d["bpl"]), p(d["Wps"]),
        p(d["bps"]), p(d["eps"]), p(d["dz"]), p(d["gklz"]), p(dqloc),
        p(dqpre), p(dprior), K, S, B, L, stream),
        "scvae_mvn_tril_logprob_pair_bwd")
    torch.cuda.synchronize()
    # the prior gradients after their reduction: dW[k] = sum over the cells,
    # db = sum over the clusters of dW (the dense layers on the one-hot)
    per_cluster = dprior.cpu().double().sum(dim=1)
    return {
        "z": z.cpu().double(), "klz": klz.cpu().double(),
        "qvar": qvar.cpu().double(), "qcov": qcov.cpu().double(),
        "dqloc": dqloc.cpu().double(), "dqpre": dqpre.cpu().double(),
        "dWpl": per_cluster[:, :L], "dbpl": per_cluster[:, :L].sum(dim=0),
        "dWps": per_cluster[:, L:], "dbps": per_cluster[:, L:].sum(dim=0),
    }, dprior


def _relative(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.mark.parametrize("K,S,B,L", SHAPES)
def test_pair_matches_fp64(cuda_device, K, S, B, L):
    inputs = _inputs(K, S, B, L, seed=L)
    want = _reference(inputs, torch.float64)
    fp32 = _reference(inputs, torch.float32)
    got, _ = _device(inputs, cuda_device)
    failures = []
    for name in want:
        e32 = _relative(fp32[name], want[name])
        err = _relative(got[name], want[name])
        print("{:6s} L={:2d}: kernel {:.3e}  fp32 torch {:.3e}  ratio {:.2f}"
              .format(name, L, err, e32, err / max(e32, 1e-30)))
        if not err <= 8 * e32 + 1e-7:
            failures.append((name, err, e32))
    assert not failures, failures


def test_clipped_scale_entries(cuda_device):
    """A scale pre-activation of -200: softplus underflows, the FLT_MIN clip
    holds the entry (a diagonal and an off-diagonal one of the posterior
    triangle, an off-diagonal one of the prior).  klz stays finite, the
    gradient at those entries is zero, the rest still matches fp64."""
    K, S, B, L = 2, 2, 5, 6
    T = L * (L + 1) // 2
    inputs = _inputs(K, S, B, L, seed=99)
    # fill_triangular: x[0] is element (L-1, L-1), x[1] is (L-1, L-2)
    m = fo.fill_triangular(torch.arange(T, dtype=torch.float64))
    assert m[L - 1, L - 1] == 0 and m[L - 1, L - 2] == 1
    inputs["qpre"][0, 3, 0] = -200.0
    inputs["qpre"][1, 2, 1] = -200.0
    inputs["Wps"][1, 1] = -200.0
    want = _reference(inputs, torch.float64)
    fp32 = _reference(inputs, torch.float32)
    got, dprior = _device(inputs, cuda_device)
    assert torch.isfinite(got["klz"]).all()
    assert torch.isfinite(got["z"]).all()
    assert got["dqpre"][0, 3, 0] == 0.0 and got["dqpre"][1, 2, 1] == 0.0
    assert (dprior[1, :, L + 1] == 0).all()
    assert want["dqpre"][0, 3, 0] == 0.0 and want["dWps"][1, 1] == 0.0
    for name in want:
        e32 = _relative(fp32[name], want[name])
        err = _relative(got[name], want[name])
        print("{:6s} clipped: kernel {:.3e}  fp32 torch {:.3e}".format(
            name, err, e32))
        assert err <= 8 * e32 + 1e-7, name
