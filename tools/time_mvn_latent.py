"""Time the latent stage of a GMVAE step, forward + backward kernel, for both mixtures: the
"multivariate gaussian" pair of the full-covariance mixture (csrc/mvn_tril.hip) and the diagonal
"softplus gaussian" pair (csrc/gmvae_kernels.hip), through their stand-alone C-ABI entries.
    python tools/time_mvn_latent.py [K] [B] [S] [L] [launches]
Defaults: the K = 20, B = 512, S = 1, L = 25 of the GMVAE benchmark.  (The per-cell prior gradients
are summed over the cells by group_col_sum inside a step; that launch is not part of either
figure.)"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from scvae_amd import _lib

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
S = int(sys.argv[3]) if len(sys.argv) > 3 else 1
L = int(sys.argv[4]) if len(sys.argv) > 4 else 25
launches = int(sys.argv[5]) if len(sys.argv) > 5 else 200
T = L * (L + 1) // 2
lib = _lib.load()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(5)
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def randn(*shape, scale=1.0):
    return torch.randn(*shape, device=dev, generator=g) * scale


def p(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


eps, dz, gklz = randn(K, S, B, L), randn(K, S, B, L, scale=0.1), randn(K, S, B, scale=0.05)
z, klz = torch.empty(K, S, B, L, device=dev), torch.empty(K, S, B, device=dev)
qloc, dqloc = randn(K * B, L), torch.empty(K * B, L, device=dev)
Wpl, bpl = randn(K, L), randn(L, scale=0.1)


def pair(width, fwd, bwd, with_qcov):
    qsc, Wps, bps = randn(K * B, width, scale=0.3), randn(K, width, scale=0.3), randn(width, scale=0.1)
    dqsc = torch.empty(K * B, width, device=dev)
    dprior = torch.empty(K * B, L + width, device=dev)
    outputs = [p(z), p(klz), None] + ([None] if with_qcov else [])

    def forward():
        _lib.check(fwd(p(qloc), p(qsc), p(Wpl), p(bpl), p(Wps), p(bps), p(eps), *outputs, K, S, B,
                       L, stream), "forward")

    def backward():
        _lib.check(bwd(p(qloc), p(qsc), p(Wpl), p(bpl), p(Wps), p(bps), p(eps), p(dz), p(gklz),
                       p(dqloc), p(dqsc), p(dprior), K, S, B, L, stream), "backward")
    return forward, backward, (klz, dqsc, dprior)


def time_ms(launch):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


for name, width, fwd, bwd, with_qcov in (
        ("multivariate gaussian (full covariance)", T, lib.scvae_mvn_tril_logprob_pair_fwd,
         lib.scvae_mvn_tril_logprob_pair_bwd, True),
        ("softplus gaussian (diagonal)", L, lib.scvae_softplus_gaussian_logprob_pair_fwd,
         lib.scvae_softplus_gaussian_logprob_pair_bwd, False)):
    forward, backward, (klz_out, dqsc, dprior) = pair(width, fwd, bwd, with_qcov)
    f, b = time_ms(forward), time_ms(backward)
    print("{}: K {} B {} S {} L {}: forward {:.1f} us, backward {:.1f} us, together {:.1f} us; "
          "checksum klz {:.6e} dscale {:.6e} dprior {:.6e}".format(
              name, K, B, S, L, 1e3 * f, 1e3 * b, 1e3 * (f + b), klz_out.double().sum().item(),
              dqsc.double().abs().sum().item(), dprior.double().abs().sum().item()))
