"""The device silhouette (``csrc/silhouette.hip``, ``analyses/silhouette.py``)
against the fp64 oracle of ``_silhouette_oracle.py``: the kernel through its C
entry with guard regions around everything it writes (a, b, s, the score, the
workspace) and NaN in the pitch padding of X, then the Python wrapper,
determinism, the rejected sizes and ``scvae evaluate --silhouette-score``.

Bounds, u = 2^-24.  A distance: the direct form sum_l (x_l - y_l)^2 in fp32
(one rounding for the difference, a fused multiply-add per coordinate) is
within (L + 2) u relative, its square root within (L + 2) / 2 u, and the
square root instruction adds 2 u (1 ulp).  A row's distances to the columns of
one tile segment are added in fp32, at most T = 64 non-negative terms: the
kernel adds them as a tree 7 additions deep, within 7 u <= (T - 1) u of their
sum.  Segments and tiles are joined in fp64, the division is in fp64, and one
rounding to fp32 (u) ends it.  So a and b are within
eps = ((L + 2) / 2 + T + 1) u relative (the last rounding is inside the factor
two below); the kernel may take another cluster for b than the oracle on a
near-tie, but that cluster's mean is within eps of the true minimum as well.
s = (b - a) / max(a, b) = 1 - a / b or b / a - 1: the ratio of two numbers
within eps each moves by at most 2 eps (the ratio is at most 1), and the
division and the rounding of s add 2 u.  The tests allow twice each.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _silhouette_oracle as so

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
T = 64          # SIL_TILE: the longest fp32 sum of the kernel
PAD = 256       # guard elements on either side of every written buffer

CASES = sorted(so.all_cases())


class Guarded:
    """A device buffer of ``n`` elements between two sentinel regions."""

    def __init__(self, n, dtype, device):
        self.sentinel = 0x5A if dtype == torch.uint8 else 12345
        self.full = torch.full((n + 2 * PAD,), self.sentinel, dtype=dtype,
                               device=device)
        self.data = self.full[PAD:PAD + n]

    def check(self):
        assert bool((self.full[:PAD] == self.sentinel).all())
        assert bool((self.full[PAD + self.data.numel():]
                     == self.sentinel).all())


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr()) if tensor is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _upload(x, ldx, device):
    """x with row pitch ldx (the pad columns hold NaN: never to be read)."""
    full = torch.full((x.shape[0], ldx), float("nan"), dtype=torch.float32,
                      device=device)
    full[:, :x.shape[1]] = torch.from_numpy(np.array(x))
    return full


def epsilon(latent_size):
    return ((latent_size + 2) / 2 + T + 1) * U


@functools.lru_cache(maxsize=None)
def _grouped(name):
    """The case in the kernel's layout: rows sorted by cluster (stable),
    offsets [K + 1], and the permutation."""
    x, labels, ldx = so.all_cases()[name]
    _, ids = np.unique(labels, return_inverse=True)
    ids = ids.reshape(-1)
    order = np.argsort(ids, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids))]).astype(
        np.int64)
    xs = np.ascontiguousarray(x[order])
    for array in (xs, offsets, order):
        array.setflags(write=False)
    return xs, offsets, order, ldx


def device_silhouette(xs, offsets, ldx, device, with_outputs=True):
    """(a, b, s) as device tensors in the grouped order and the score tensor;
    every buffer the entry writes sits between sentinels."""
    from scvae_amd import _lib
    lib = _lib.load()
    n, latent_size = xs.shape
    k = len(offsets) - 1
    xd = _upload(xs, ldx, device)
    od = torch.from_numpy(np.array(offsets)).to(device)
    outputs = [Guarded(n, torch.float32, device) for _ in range(3)]
    score = Guarded(1, torch.float64, device)
    nbytes = lib.scvae_silhouette_workspace_bytes(n, latent_size, k)
    assert nbytes > 0
    workspace = Guarded(nbytes, torch.uint8, device)
    pointers = [_ptr(o.data) if with_outputs else None for o in outputs]
    _lib.check(lib.scvae_silhouette_samples(
        _ptr(xd), ldx, n, latent_size, _ptr(od), k, *pointers,
        _ptr(score.data), _ptr(workspace.data), workspace.data.numel(),
        _stream(device)), "scvae_silhouette_samples")
    torch.cuda.synchronize()
    for buffer in outputs + [score, workspace]:
        buffer.check()
    if not with_outputs:
        for o in outputs:
            assert bool((o.data == o.sentinel).all())
    return [o.data.clone() for o in outputs], score.data.clone()


def check_against_oracle(a, b, s, score, want, latent_size, own_counts):
    """a, b, s fp32 [N] and the score against the oracle's fp64 (a, b, s), all
    in one row order."""
    wa, wb, ws = want
    eps = epsilon(latent_size)
    assert a.dtype == b.dtype == s.dtype == np.float32

    def worst(error, bound):
        return float(np.max(error / np.maximum(bound, 1e-300) * (bound > 0)))
    error_a, error_b = np.abs(a - wa), np.abs(b - wb)
    error_s = np.abs(s - ws)
    s_bound = 2 * (2 * eps + 2 * U)
    print("a error / bound: {:.3f}, b: {:.3f}, s: {:.3f}".format(
        worst(error_a, 2 * eps * wa), worst(error_b, 2 * eps * wb),
        float(error_s.max() / s_bound)))
    assert np.all(error_a <= 2 * eps * wa)      # (a = 0 exactly where wa = 0)
    assert np.all(error_b <= 2 * eps * wb)
    assert np.all(error_s <= s_bound)
    # the zero rules are exact
    assert np.all(s[own_counts == 1] == 0.0) and np.all(a[own_counts == 1] == 0)
    assert np.all(s[np.maximum(wa, wb) == 0.0] == 0.0)
    print("score {:.9f}, oracle {:.9f}".format(score, float(ws.mean())))
    assert abs(score - float(ws.mean())) <= s_bound
    # ... and the score is the fp64 mean of the s the kernel wrote
    assert abs(score - float(s.astype(np.float64).mean())) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_entry_against_oracle(cuda_device, name):
    xs, offsets, order, ldx = _grouped(name)
    (a, b, s), score = device_silhouette(xs, offsets, ldx, cuda_device)
    want = [w[order] for w in so.expected(name)]
    own_counts = np.repeat(np.diff(offsets), np.diff(offsets))
    check_against_oracle(a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy(),
                         float(score.item()), want, xs.shape[1], own_counts)


def test_duplicate_rows_give_exact_values(cuda_device):
    """Clusters that are one point repeated: a = 0 and s = 1 exactly;
    identical rows split over two clusters: a = b = 0 and s = 0."""
    xs, offsets, order, ldx = _grouped("duplicates")
    assert np.array_equal(order, np.argsort(so.duplicate_case()[1],
                                            kind="stable"))
    (a, b, s), score = device_silhouette(xs, offsets, ldx, cuda_device)
    a, b, s = a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()
    assert np.all(a == 0.0)
    assert np.all(b[:100] > 0.0) and np.all(s[:100] == 1.0)
    assert np.all(b[100:] == 0.0) and np.all(s[100:] == 0.0)
    assert float(score.item()) == 100.0 / 104.0


def test_outputs_are_optional_and_calls_repeat_bit_for_bit(cuda_device):
    name = "2051x100x20x100"
    xs, offsets, order, ldx = _grouped(name)
    first, first_score = device_silhouette(xs, offsets, ldx, cuda_device)
    second, second_score = device_silhouette(xs, offsets, ldx, cuda_device)
    for one, other in zip(first + [first_score], second + [second_score]):
        assert torch.equal(one, other)
    _, bare_score = device_silhouette(xs, offsets, ldx, cuda_device,
                                      with_outputs=False)
    assert torch.equal(bare_score, first_score)


@pytest.mark.parametrize("name", ["1000x25x20x25", "65x7x64x7", "edges"])
def test_wrapper_returns_the_callers_row_order(cuda_device, name):
    """Shuffled rows and label values that are no 0 .. K - 1 (7, -3, 100,
    ...): ``silhouette_samples`` answers in the order it was asked in."""
    from scvae_amd.analyses import silhouette_samples, silhouette_score
    x, labels, _ = so.all_cases()[name]
    k = int(labels.max()) + 1
    rng = np.random.default_rng(k)
    values = np.array([7, -3, 100] + list(1000 - 13 * np.arange(k)))[:k]
    assert len(set(values.tolist())) == k
    shuffle = rng.permutation(len(labels))
    given = values[labels[shuffle]]
    got = silhouette_samples(x[shuffle], given, device=cuda_device)
    assert got.dtype == np.float32 and got.shape == (len(labels),)
    want = so.expected(name)[2][shuffle]
    s_bound = 2 * (2 * epsilon(x.shape[1]) + 2 * U)
    assert np.all(np.abs(got - want) <= s_bound)
    again = silhouette_samples(x[shuffle], given, device=cuda_device)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    score = silhouette_score(x[shuffle], given, device=cuda_device)
    assert isinstance(score, float)
    assert abs(score - float(want.mean())) <= s_bound
    assert abs(score - float(got.astype(np.float64).mean())) <= 1e-12


def test_entry_rejects_sizes_outside_the_limits(cuda_device):
    """-1 with a message for L = 257, K = 1, K = N and a workspace one byte
    short; nothing is launched: the outputs keep their fill."""
    from scvae_amd import _lib
    lib = _lib.load()
    n, k = 100, 4
    nbytes = lib.scvae_silhouette_workspace_bytes(n, 8, k)
    x = torch.zeros(n, 257, dtype=torch.float32, device=cuda_device)
    offsets = torch.tensor([0, 25, 50, 75, 100], dtype=torch.int64,
                           device=cuda_device)
    outputs = [Guarded(n, torch.float32, cuda_device) for _ in range(3)]
    score = Guarded(1, torch.float64, cuda_device)
    workspace = Guarded(nbytes, torch.uint8, cuda_device)

    def entry(latent_size, clusters, workspace_bytes):
        return lib.scvae_silhouette_samples(
            _ptr(x), 257, n, latent_size, _ptr(offsets), clusters,
            *[_ptr(o.data) for o in outputs], _ptr(score.data),
            _ptr(workspace.data), workspace_bytes, _stream(cuda_device))
    for arguments, limit in (((257, k, nbytes), "L <="),
                             ((8, 1, nbytes), "K >= 2"),
                             ((8, n, nbytes), "K <= N - 1"),
                             ((8, k, nbytes - 1), "workspace_bytes")):
        assert entry(*arguments) == -1, arguments
        message = lib.scvae_last_error().decode()
        assert "bad argument" in message and limit in message, message
    torch.cuda.synchronize()
    for buffer in outputs + [score, workspace]:
        assert bool((buffer.full == buffer.sentinel).all())
    assert entry(8, k, nbytes) == 0
    torch.cuda.synchronize()
    for buffer in outputs + [score, workspace]:
        buffer.check()
    assert float(score.data.item()) == 0.0      # every row is the same point


def test_cli_evaluate_with_silhouette_score(tmp_path, cuda_device, capsys):
    """``scvae evaluate -P k-means --silhouette-score``: the printed value is
    the device's score of the predicted clusters over the latent values of
    the evaluation set, and that score is the oracle's."""
    from scvae_amd import cli
    from scvae_amd.analyses import silhouette
    arguments = ["synthetic_1k", "-M", str(tmp_path), "-r", "poisson", "-l",
                 "3", "-H", "20", "-B", "100", "--split-data-set"]
    cli.main(["train"] + arguments + ["-e", "2"])
    capsys.readouterr()
    calls = []
    score = silhouette.silhouette_score

    def recording_score(values, labels, device=None):
        result = score(values, labels, device)
        calls.append((np.array(values), np.array(labels), result))
        return result
    silhouette.silhouette_score = recording_score
    try:
        results = cli.main(["evaluate"] + arguments + [
            "-P", "k-means", "--silhouette-score"])
    finally:
        silhouette.silhouette_score = score
    out = capsys.readouterr().out
    transformed, reconstructed, latent = results["end_of_training"]
    assert "silhouette score on the device not used" not in out
    assert len(calls) == (2 if transformed.has_labels else 1)
    lines = out.splitlines()
    assert sum(line.startswith("Clustering of the") for line in lines) == 1
    kinds = ["clusters", "labels"]
    for kind, (values, labels, result) in zip(kinds, calls):
        assert values.shape == (100, 3) and labels.shape == (100,)
        assert np.array_equal(values, np.asarray(latent["z"].values))
        assert "    silhouette score ({}): {:.4f}".format(kind, result) in lines
        distinct = len(np.unique(labels))
        if 2 <= distinct <= 99:
            want = so.silhouette(values.astype(np.float32), labels)[2]
            s_bound = 2 * (2 * epsilon(3) + 2 * U)
            assert abs(result - float(want.mean())) <= s_bound
        else:
            assert np.isnan(result)
    assert np.array_equal(calls[0][1], transformed.predicted_cluster_ids)
    assert any(2 <= len(np.unique(c[1])) <= 99 for c in calls)

    cli.main(["evaluate"] + arguments + ["-P", "k-means"])
    assert "silhouette" not in capsys.readouterr().out
