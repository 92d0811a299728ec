"""The latent stage of the full-covariance mixture (scvae_amd/csrc/mvn_tril.hip)
through its three stand-alone C-ABI entries, held to fp64 ELEMENT BY ELEMENT.

Every comparison is ``|got - want| <= bound(element)`` (``_mixture_oracle.hold``)
with ``want`` and ``bound`` from tests/_fullcov_elements_oracle.py, where each
bound is derived in the module docstring from the roundings the kernels perform
(the total allowed twice); tests/test_fullcov_elements_host.py takes a NumPy fp32
evaluation of the same formulation through the same checks on the same cases and
shows that the listed mutations are rejected.  No mask: every element of every
output is held.  Outputs are NaN-filled before the call and followed by a canary
region that has to come back untouched.  Each test prints err / bound per output.

  geometry      L through every wave count of either kernel's block and both
                sides of each boundary (forward 4 | 54-55 | 3 | 63-64 | 2; backward
                4 | 37-38 | 3 | 44-45 | 2 | 54-55 | 1), L = 32 / 33; K B = 7 (idle
                waves), K B the wave count, K = 3, S in {1, 3}; diagonally dominant
                triangles, where the bound is tight at every width
  probes        the log-determinant alone (u == 0 exactly); one-hot eps (z is one
                column of A: every fill_triangular entry on its own)
  conditioning  the dense recipe of test_gpu_fullcov_kernels.py at L = 25 and 64;
                u_i = +-(1 +- 2^-10): the cancellation in g (1 - u_i^2) / P_ii
  the clip      pre-activations on both sides of softplus(pre) = FLT_MIN, on a
                posterior diagonal, a posterior off-diagonal and a prior
                off-diagonal entry; sum_s g / A_ii beyond fp32
"""
import ctypes

import numpy as np
import pytest
import torch

import _fullcov_elements_oracle as eo

pytestmark = pytest.mark.gpu

CANARY, CANARY_FLOATS = 12345.678, 64
OTHER_CASES = [c for c in eo.CASES if c[0] != "dominant"]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Device:
    """The entries on the GPU: NumPy fp32 in, NumPy fp32 out."""

    def __init__(self, device):
        from scvae_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.device = device
        self._inputs, self._outputs = [], []

    def up(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self._inputs.append(t)      # (kept until ``down``: see test_gpu_mixture_stage.py)
        return t

    def out(self, *shape):
        # NaN-filled (an element left unwritten fails its bound), a canary behind it
        n = int(np.prod(shape))
        t = torch.full((n + CANARY_FLOATS,), float("nan"), device=self.device)
        t[n:] = CANARY
        self._outputs.append((t, n))
        return t[:n].view(*shape) if n else t[:0]

    def call(self, name, *args, expect_error=False):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = getattr(self.lib, name)(*args, stream)
        if expect_error:
            return rc
        try:
            self._lib.check(rc, name)
        except Exception as e:      # (nothing more runs on a device that reported an error)
            pytest.exit("{}: {}".format(name, e), returncode=3)
        return rc

    def down(self, *ts):
        try:
            torch.cuda.synchronize()
            r = [t.cpu().numpy() for t in ts]
            tails = [t[n:].cpu().numpy() for t, n in self._outputs]
        except RuntimeError as e:
            pytest.exit("device error: {}".format(e), returncode=3)
        for tail in tails:
            assert (tail == np.float32(CANARY)).all(), "canary overwritten"
        self._inputs.clear()
        self._outputs.clear()
        return r

    def _ins(self, arrays):
        d = {k: self.up(v) for k, v in arrays.items()}
        return d, [_p(d[k]) for k in ("qloc", "qpre", "Wpl", "bpl", "Wps", "bps", "eps")]

    def forward(self, arrays, K, S, B, L, stats=True):
        d, ins = self._ins(arrays)
        z, klz = self.out(K, S, B, L), self.out(K, S, B)
        qvar = self.out(K * B, L) if stats else None
        qcov = self.out(K * B, L, L) if stats else None
        self.call("scvae_mvn_tril_logprob_pair_fwd", *ins, _p(z), _p(klz), _p(qvar), _p(qcov),
                  K, S, B, L)
        names = ("z", "klz", "qvar", "qcov")[:4 if stats else 2]
        return dict(zip(names, self.down(*(t for t in (z, klz, qvar, qcov) if t is not None))))

    def backward(self, arrays, K, S, B, L):
        T = eo.tri(L)
        d, ins = self._ins(arrays)
        dqloc, dqsc, dprior = self.out(K * B, L), self.out(K * B, T), self.out(K * B, L + T)
        self.call("scvae_mvn_tril_logprob_pair_bwd", *ins, _p(d["dz"]), _p(d["gklz"]),
                  _p(dqloc), _p(dqsc), _p(dprior), K, S, B, L)
        return dict(zip(("dqloc", "dqsc", "dprior"), self.down(dqloc, dqsc, dprior)))

    def pair(self, arrays, K, S, B, L):
        got = self.forward(arrays, K, S, B, L)
        got.update(self.backward(arrays, K, S, B, L))
        return got

    def prior_stats(self, arrays, K, L, covariances=True):
        ins = [_p(self.up(arrays[k])) for k in ("Wpl", "bpl", "Wps", "bps")]
        means, variances = self.out(K, L), self.out(K, L)
        cov = self.out(K, L, L) if covariances else None
        self.call("scvae_mvn_tril_prior_stats", *ins, K, L, _p(means), _p(variances), _p(cov))
        names = ("means", "variances", "covariances")[:3 if covariances else 2]
        return dict(zip(names, self.down(*(t for t in (means, variances, cov) if t is not None))))


@pytest.fixture
def run(cuda_device):
    return Device(cuda_device)


@pytest.fixture(scope="module")
def report():
    """(row, output) -> largest err / bound; printed when the module is done."""
    table = {}
    yield table
    eo.print_table(table, "the device")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("L", eo.GEOMETRY_L)
def test_geometry(run, report, L):
    """Diagonally dominant triangles, forward and backward, at every (K, S, B) of
    ``eo.geometry_shapes``; and z / klz of the call without qvar / qcov are the
    bits of the call with them."""
    for case in eo.CASES:
        if case[0] == "dominant" and case[4] == L:
            eo.check_pair(run, *case, report)
    K, S, B = 1, 3, 7
    arrays = eo.inputs("dominant", K, S, B, L)
    full, bare = run.forward(arrays, K, S, B, L), run.forward(arrays, K, S, B, L, stats=False)
    for name in ("z", "klz"):
        assert (_bits(full[name]) == _bits(bare[name])).all(), name


@pytest.mark.parametrize("case", OTHER_CASES, ids=lambda c: "{}-L{}".format(c[0], c[4]))
def test_probes_conditioning_and_clip(run, report, case):
    eo.check_pair(run, *case, report)


@pytest.mark.parametrize("K,L", eo.PRIOR_STATS_CASES)
def test_prior_stats(run, report, K, L):
    """means, variances and covariances per element, the covariances symmetric bit
    for bit; without covariances the other two carry the same bits."""
    eo.check_prior_stats(run, K, L, report)
    arrays = eo.inputs("dense", K, 1, 1, L)
    full, bare = run.prior_stats(arrays, K, L), run.prior_stats(arrays, K, L, covariances=False)
    for name in ("means", "variances"):
        assert (_bits(full[name]) == _bits(bare[name])).all(), name
    d = np.arange(L)
    assert (_bits(full["covariances"][:, d, d]) == _bits(full["variances"])).all()


def test_prior_stats_clip(run, report):
    """The prior's entry (L-1, 0) held at FLT_MIN, through covariance (L-1, 0)."""
    eo.check_prior_stats(run, eo.CLIP_SHAPE[0], eo.CLIP_SHAPE[3], report, kind="clip")


def test_empty_batch_and_refused_widths(run):
    """B = 0 returns 0 and writes nothing; L = 0 and L = 65 are refused with an
    error code before any launch: every output keeps its NaN fill."""
    K, S, L = 2, 2, 6
    T = eo.tri(L)
    arrays = eo.inputs("dense", K, S, 3, L)
    d, ins = run._ins(arrays)
    for B, LL, refused in ((0, L, False), (3, 0, True), (3, 65, True)):
        outs = [run.out(n) for n in (K * S * 3 * L, K * S * 3, K * 3 * L, K * 3 * L * L)]
        rc = run.call("scvae_mvn_tril_logprob_pair_fwd", *ins, *[_p(t) for t in outs],
                      K, S, B, LL, expect_error=True)
        assert (rc != 0) == refused, (B, LL, rc)
        bouts = [run.out(n) for n in (K * 3 * L, K * 3 * T, K * 3 * (L + T))]
        rc = run.call("scvae_mvn_tril_logprob_pair_bwd", *ins, _p(d["dz"]), _p(d["gklz"]),
                      *[_p(t) for t in bouts], K, S, B, LL, expect_error=True)
        assert (rc != 0) == refused, (B, LL, rc)
        if refused:
            souts = [run.out(n) for n in (K * L, K * L, K * L * L)]
            rc = run.call("scvae_mvn_tril_prior_stats",
                          *[_p(d[k]) for k in ("Wpl", "bpl", "Wps", "bps")], K, LL,
                          *[_p(t) for t in souts], expect_error=True)
            assert rc != 0, (LL, rc)
            bouts += souts
        for a in run.down(*outs, *bouts):       # (``d`` keeps the inputs alive)
            assert np.isnan(a).all(), (B, LL)
