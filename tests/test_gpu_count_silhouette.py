"""The count-space silhouette on the device (``csrc/count_silhouette.hip``,
``analyses/count_silhouette.py``) against the oracle of
``_count_silhouette_oracle.py``: the distance stage element by element
against the exact integers, then a, b, s and the score, through the C entries
with guard regions around everything they write; the Python wrappers,
determinism, the rejected sizes and ``scvae evaluate --silhouette-space
counts``.

Bounds, u = 2^-24.  A distance: d2 is an exact integer below 2^50 and
converts to fp64 exactly; the fp64 square root is within 2^-52 relative and
the one rounding to fp32 within u, so |d - sqrt(d2)| <= (u + 2^-51) sqrt(d2).
The oracle's own root is within 2^-53: D = u + 2^-50 covers both.  A sum of
distances over a cluster is taken in fp64 (at most N non-negative terms:
within N 2^-53 relative, whatever the order), the division in fp64 (2^-53),
so the fp64 a and b are within E = D + (N + 2) 2^-53 relative, and the fp32
ones the entry writes within E + u.  The kernel may take another cluster for
b than the oracle on a near-tie, but that cluster's mean is within E of the
true minimum as well.  s = (b - a) / max(a, b) = 1 - a / b or b / a - 1 is
formed in fp64 from the fp64 a and b: the ratio of two numbers within E each
moves by at most 2 E / (1 - E) (the ratio is at most 1), three fp64
operations add 3 x 2^-53, and the rounding of s to fp32 adds u.  The tests
allow twice each.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse
import torch

import _count_silhouette_oracle as co

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
D_BOUND = U + 2.0 ** -50          # a distance, relative; well below 4 u
PAD = 256       # guard elements on either side of every written buffer

CASES = sorted(co.all_cases())


def ab_bound(n):
    return D_BOUND + (n + 2) * 2.0 ** -53 + U


def s_bound(n):
    e = D_BOUND + (n + 2) * 2.0 ** -53
    return 2 * e / (1 - e) + 3 * 2.0 ** -53 + U


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

    def untouched(self):
        return bool((self.full == self.sentinel).all())


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr()) if tensor is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _upload(x, ldx, device):
    """x as uint16 rows of pitch ldx; the pad columns are zero, as the
    layout has them."""
    full = np.zeros((x.shape[0], ldx), dtype=np.uint16)
    full[:, :x.shape[1]] = x
    tensor = torch.from_numpy(full.view(np.int16)).to(device).view(
        torch.uint16)
    assert tensor.data_ptr() % 16 == 0
    return tensor


def _minimum_workspace(n, strip_rows):
    return (8 * n + (4 * n + 7) // 8 * 8
            + strip_rows * 4 * ((n + 15) // 16 * 16))


@functools.lru_cache(maxsize=None)
def _grouped(name):
    """The case in the kernel's layout: rows sorted by cluster (stable),
    offsets [K + 1], and the permutation."""
    x, labels, ldx = co.all_cases()[name]
    _, ids = np.unique(labels, return_inverse=True)
    ids = ids.reshape(-1)
    order = np.argsort(ids, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids))]).astype(
        np.int64)
    xs = np.ascontiguousarray(x[order])
    for array in (xs, offsets, order):
        array.setflags(write=False)
    return xs, offsets, order, ldx


def device_distances(xd, ldx, n, features, i0, rows, device):
    """The strip d [rows, N] of the entry, every written buffer guarded, the
    pitch of d three elements beyond N."""
    from scvae_amd import _lib
    lib = _lib.load()
    ldd = n + 3
    d = Guarded(rows * ldd, torch.float32, device)
    workspace = Guarded(8 * n, torch.uint8, device)
    _lib.check(lib.scvae_count_distances_u16(
        _ptr(xd), ldx, n, features, i0, rows, _ptr(d.data), ldd,
        _ptr(workspace.data), workspace.data.numel(), _stream(device)),
        "scvae_count_distances_u16")
    torch.cuda.synchronize()
    d.check()
    workspace.check()
    strip = d.data.view(rows, ldd)
    assert bool((strip[:, n:] == d.sentinel).all())
    return strip[:, :n].cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_distances_against_the_exact_integers(cuda_device, name):
    """Two strips, the second ragged and at i0 > 0: every element against
    the fp64 root of the oracle's exact integer, zero exactly where the rows
    are equal and nowhere else, symmetric bit for bit."""
    x, _, ldx = co.all_cases()[name]
    n, features = x.shape
    xd = _upload(x, ldx, cuda_device)
    first = 128 * max(1, (n * 5 // 8) // 128) if n > 128 else n // 2
    d = np.concatenate([
        device_distances(xd, ldx, n, features, 0, first, cuda_device),
        device_distances(xd, ldx, n, features, first, n - first,
                         cuda_device)])
    assert d.dtype == np.float32 and d.shape == (n, n)
    d2 = co.expected_squared_distances(name)
    want = np.sqrt(d2.astype(np.float64))
    error = np.abs(d.astype(np.float64) - want)
    # (u + 2^-51) sqrt(d2) from the route integer -> fp64 -> root -> fp32,
    # 2^-53 for the oracle's root: see the head of this file
    print("worst distance error / bound: {:.3f}".format(
        float(np.max(error / np.maximum(D_BOUND * want, 1e-300)
                     * (want > 0)))))
    assert D_BOUND <= 4 * U
    assert np.all(error <= D_BOUND * want)
    assert np.array_equal(d == 0.0, d2 == 0)
    assert np.all((d2 == 0)[np.arange(n), np.arange(n)])
    assert np.array_equal(d.view(np.uint32), d.T.view(np.uint32))
    if name == "saturated":
        assert d2[0, 4] == 520 * 65535 ** 2
        assert d[0, 4] == np.float32(np.sqrt(np.float64(520 * 65535 ** 2)))


def device_silhouette(xs, offsets, ldx, device, with_outputs=True,
                      strip_rows=None):
    """(a, b, s) as device tensors in the grouped order and the score tensor;
    every buffer the entry writes sits between sentinels.  ``strip_rows``: a
    workspace that leaves a strip of that many rows."""
    from scvae_amd import _lib
    lib = _lib.load()
    n, features = xs.shape
    k = len(offsets) - 1
    xd = _upload(xs, ldx, device)
    od = torch.from_numpy(np.array(offsets)).to(device)
    outputs = [Guarded(n, torch.float32, device) for _ in range(3)]
    score = Guarded(1, torch.float64, device)
    nbytes = lib.scvae_count_silhouette_workspace_bytes(n, features, k)
    assert nbytes > 0
    if strip_rows is not None:
        nbytes = _minimum_workspace(n, strip_rows)
    workspace = Guarded(nbytes, torch.uint8, device)
    pointers = [_ptr(o.data) if with_outputs else None for o in outputs]
    _lib.check(lib.scvae_count_silhouette_samples_u16(
        _ptr(xd), ldx, n, features, _ptr(od), k, *pointers,
        _ptr(score.data), _ptr(workspace.data), workspace.data.numel(),
        _stream(device)), "scvae_count_silhouette_samples_u16")
    torch.cuda.synchronize()
    for buffer in outputs + [score, workspace]:
        buffer.check()
    if not with_outputs:
        for o in outputs:
            assert o.untouched()
    return [o.data.clone() for o in outputs], score.data.clone()


def check_against_oracle(a, b, s, score, want, own_counts):
    """a, b, s fp32 [N] and the score against the oracle's fp64 (a, b, s), all
    in one row order."""
    wa, wb, ws = want
    n = len(ws)
    assert a.dtype == b.dtype == s.dtype == np.float32

    def worst(error, bound):
        return float(np.max(error / np.maximum(bound, 1e-300) * (bound > 0)))
    error_a, error_b = np.abs(a - wa), np.abs(b - wb)
    error_s = np.abs(s - ws)
    print("a error / bound: {:.3f}, b: {:.3f}, s: {:.3f}".format(
        worst(error_a, 2 * ab_bound(n) * wa),
        worst(error_b, 2 * ab_bound(n) * wb),
        float(error_s.max() / (2 * s_bound(n)))))
    assert np.all(error_a <= 2 * ab_bound(n) * wa)  # (a = 0 exactly at wa = 0)
    assert np.all(error_b <= 2 * ab_bound(n) * wb)
    assert np.all(error_s <= 2 * s_bound(n))
    # the zero rules are exact
    assert np.all(s[own_counts == 1] == 0.0) and np.all(a[own_counts == 1] == 0)
    assert np.all(s[np.maximum(wa, wb) == 0.0] == 0.0)
    print("score {:.9f}, oracle {:.9f}".format(score, float(ws.mean())))
    assert abs(score - float(ws.mean())) <= 2 * s_bound(n)
    # ... and the score is the fp64 mean of the s the kernel wrote
    assert abs(score - float(s.astype(np.float64).mean())) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_entry_against_oracle(cuda_device, name):
    xs, offsets, order, ldx = _grouped(name)
    (a, b, s), score = device_silhouette(xs, offsets, ldx, cuda_device)
    want = [w[order] for w in co.expected(name)]
    own_counts = np.repeat(np.diff(offsets), np.diff(offsets))
    check_against_oracle(a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy(),
                         float(score.item()), want, own_counts)


def test_saturated_rows_give_exact_values(cuda_device):
    """Identical rows in different clusters: a = b = 0 and s = 0; clusters
    that are one row repeated: a = 0, s = 1; a twin in another cluster:
    b = 0, s = -1."""
    xs, offsets, order, ldx = _grouped("saturated")
    assert np.array_equal(order, [0, 2, 1, 3] + list(range(4, 12)))
    (a, b, s), score = device_silhouette(xs, offsets, ldx, cuda_device)
    a, b, s = a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()
    assert np.all(a[:10] == 0.0) and np.all(b[:4] == 0.0)
    assert np.all(s[:4] == 0.0)
    assert np.all(b[4:10] > 0.0) and np.all(s[4:10] == 1.0)
    assert np.all(a[10:] == np.float32(np.sqrt(np.float64(520 * 65535 ** 2))))
    assert np.all(b[10:] == 0.0) and np.all(s[10:] == -1.0)
    assert float(score.item()) == 4.0 / 12.0


def test_strips_outputs_and_repeats(cuda_device):
    """A workspace that leaves strips of 128 and of 256 rows gives the bits
    of the one that holds all rows; so do a second call and a call without
    the optional outputs."""
    name = "1000x2000x999"
    xs, offsets, order, ldx = _grouped(name)
    first, first_score = device_silhouette(xs, offsets, ldx, cuda_device)
    second, second_score = device_silhouette(xs, offsets, ldx, cuda_device)
    for one, other in zip(first + [first_score], second + [second_score]):
        assert torch.equal(one, other)
    for strip_rows in (128, 256, 300):
        strips, strips_score = device_silhouette(
            xs, offsets, ldx, cuda_device, strip_rows=strip_rows)
        for one, other in zip(first + [first_score], strips + [strips_score]):
            assert torch.equal(one, other)
    _, bare_score = device_silhouette(xs, offsets, ldx, cuda_device,
                                      with_outputs=False, strip_rows=128)
    assert torch.equal(bare_score, first_score)


def _given_labels(labels, seed):
    """The clusters of ``labels`` under arbitrary values (7, -3, 100, ...)."""
    k = int(labels.max()) + 1
    values = np.array([7, -3, 100] + list(1000 - 13 * np.arange(k)))[:k]
    assert len(set(values.tolist())) == k
    return values[labels]


@pytest.mark.parametrize("name", ["130x300x5", "65x515x64", "edges"])
@pytest.mark.parametrize("sparse", [False, True])
def test_wrapper_returns_the_callers_row_order(cuda_device, name, sparse):
    """Shuffled rows and label values that are no 0 .. K - 1:
    ``count_silhouette_samples`` answers in the order it was asked in,
    for sparse and for dense input."""
    from scvae_amd.analyses import (
        count_silhouette_samples, count_silhouette_score)
    x, labels, _ = co.all_cases()[name]
    n = len(labels)
    shuffle = np.random.default_rng(n).permutation(n)
    given = _given_labels(labels, n)[shuffle]
    values = x[shuffle]
    if sparse:
        values = scipy.sparse.csr_matrix(values.astype(np.float32))
    got = count_silhouette_samples(values, given, device=cuda_device)
    assert got.dtype == np.float32 and got.shape == (n,)
    want = co.expected(name)[2][shuffle]
    assert np.all(np.abs(got - want) <= 2 * s_bound(n))
    again = count_silhouette_samples(values, given, device=cuda_device)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    score = count_silhouette_score(values, given, device=cuda_device)
    assert isinstance(score, float)
    assert abs(score - float(want.mean())) <= 2 * s_bound(n)
    assert abs(score - float(got.astype(np.float64).mean())) <= 1e-12


def test_wrapper_scores_the_sample(cuda_device):
    """``sample_size=100, random_state=3`` on the 1000 x 2000 rows: the
    oracle's score of ``RandomState(3).permutation(1000)[:100]``."""
    from scvae_amd.analyses import count_silhouette_score
    x, labels, _ = co.all_cases()["1000x2000x999"]
    labels = labels % 7
    chosen = np.random.RandomState(3).permutation(1000)[:100]
    want = co.silhouette(x[chosen], labels[chosen])[2]
    for values in (x, scipy.sparse.csr_matrix(x.astype(np.float32))):
        score = count_silhouette_score(values, labels, sample_size=100,
                                       random_state=3, device=cuda_device)
        print("score {:.9f}, oracle {:.9f}".format(score, float(want.mean())))
        assert abs(score - float(want.mean())) <= 2 * s_bound(100)


def test_entries_reject_sizes_outside_the_limits(cuda_device):
    """-1 with a message for F = 65 537, K = 1, K = N, N = 2, a pitch below
    F rounded up to 64 and a workspace one byte short; nothing is launched:
    the outputs keep their fill."""
    from scvae_amd import _lib
    lib = _lib.load()
    n, k, features, ldx = 100, 4, 8, 64
    nbytes = lib.scvae_count_silhouette_workspace_bytes(n, features, k)
    assert nbytes == _minimum_workspace(n, n)
    x = torch.zeros(n, ldx, dtype=torch.int16, device=cuda_device)
    offsets = torch.tensor([0, 25, 50, 75, 100], dtype=torch.int64,
                           device=cuda_device)
    outputs = [Guarded(n, torch.float32, cuda_device) for _ in range(3)]
    score = Guarded(1, torch.float64, cuda_device)
    workspace = Guarded(nbytes, torch.uint8, cuda_device)
    d = Guarded(n * n, torch.float32, cuda_device)

    def samples(rows, genes, clusters, workspace_bytes, pitch=ldx):
        return lib.scvae_count_silhouette_samples_u16(
            _ptr(x), pitch, rows, genes, _ptr(offsets), clusters,
            *[_ptr(o.data) for o in outputs], _ptr(score.data),
            _ptr(workspace.data), workspace_bytes, _stream(cuda_device))

    def distances(rows, genes, i0, strip, workspace_bytes, pitch=ldx):
        return lib.scvae_count_distances_u16(
            _ptr(x), pitch, rows, genes, i0, strip, _ptr(d.data), n,
            _ptr(workspace.data), workspace_bytes, _stream(cuda_device))
    for arguments, limit in (((n, 65537, k, nbytes), "F <="),
                             ((n, features, 1, nbytes), "K >= 2"),
                             ((n, features, n, nbytes), "K <= N - 1"),
                             ((2, features, 2, nbytes), "N >= 3"),
                             ((n, 65, k, nbytes), "ldx"),
                             ((n, features, k, nbytes, 60), "ldx"),
                             ((n, features, k, nbytes - 1),
                              "workspace_bytes")):
        assert samples(*arguments) == -1, arguments
        message = lib.scvae_last_error().decode()
        assert "bad argument" in message and limit in message, message
    for arguments, limit in (((n, 65537, 0, n, nbytes), "F <="),
                             ((2, features, 0, 2, nbytes), "N >= 3"),
                             ((n, features, 1, n, nbytes), "rows"),
                             ((n, features, 0, 0, nbytes), "rows"),
                             ((n, 65, 0, n, nbytes), "ldx"),
                             ((n, features, 0, n, 8 * n - 1),
                              "workspace_bytes")):
        assert distances(*arguments) == -1, arguments
        message = lib.scvae_last_error().decode()
        assert "bad argument" in message and limit in message, message
    torch.cuda.synchronize()
    for buffer in outputs + [score, workspace, d]:
        assert buffer.untouched()
    assert samples(n, features, k, nbytes) == 0
    assert distances(n, features, 0, n, nbytes) == 0
    torch.cuda.synchronize()
    for buffer in outputs + [score, workspace, d]:
        buffer.check()
    assert float(score.data.item()) == 0.0      # every row is the same cell
    assert bool((d.data == 0.0).all())


def test_cli_evaluate_with_count_space_silhouette(tmp_path, cuda_device,
                                                  capsys):
    """``scvae evaluate -P k-means --silhouette-score --silhouette-space
    counts``: the printed values are the device's scores of the predicted
    clusters and labels over the counts of the evaluation set, and those are
    the oracle's."""
    from scvae_amd import cli
    from scvae_amd.analyses import count_silhouette
    arguments = ["synthetic_1k", "-M", str(tmp_path), "-r", "poisson", "-l",
                 "3", "-H", "20", "-B", "100", "--split-data-set"]
    cli.main(["train"] + arguments + ["-e", "2"])
    capsys.readouterr()
    calls = []
    score = count_silhouette.count_silhouette_score

    def recording_score(values, labels, **keyword_arguments):
        result = score(values, labels, **keyword_arguments)
        calls.append((values, np.array(labels), result))
        return result
    count_silhouette.count_silhouette_score = recording_score
    try:
        results = cli.main(["evaluate"] + arguments + [
            "-P", "k-means", "--silhouette-score", "--silhouette-space",
            "counts"])
    finally:
        count_silhouette.count_silhouette_score = score
    out = capsys.readouterr().out
    transformed, reconstructed, latent = results["end_of_training"]
    assert "silhouette score on the device not used" not in out
    assert len(calls) == (2 if transformed.has_labels else 1)
    lines = out.splitlines()
    assert sum(line.startswith("Clustering of the") for line in lines) == 1
    assert not any(line.startswith("    silhouette score (clusters):")
                   for line in lines)
    assert not any("sampled" in line for line in lines)
    counts = transformed.values
    counts = counts.toarray() if hasattr(counts, "toarray") else counts
    counts = np.asarray(counts)
    n = counts.shape[0]
    assert n == 100 and np.array_equal(counts, np.floor(counts))
    kinds = ["clusters", "labels"]
    for kind, (values, labels, result) in zip(kinds, calls):
        assert values is transformed.values and labels.shape == (n,)
        assert "    silhouette score ({}; count space): {:.4f}".format(
            kind, result) in lines
        distinct = len(np.unique(labels))
        if 2 <= distinct <= n - 1:
            want = co.silhouette(counts.astype(np.int64), labels)[2]
            assert abs(result - float(want.mean())) <= 2 * s_bound(n)
        else:
            assert np.isnan(result)
    assert np.array_equal(calls[0][1], transformed.predicted_cluster_ids)
    assert any(2 <= len(np.unique(c[1])) <= n - 1 for c in calls)
