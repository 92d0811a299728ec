"""The device k-means (``csrc/kmeans.hip``, ``analyses/kmeans.py``) against the
fp64 oracle of ``_kmeans_oracle.py``: the three kernels through their C
entries with guard regions around every buffer they write, then whole fits,
determinism, k-means++ seeding and ``scvae evaluate --prediction-on-device``.

u = 2^-24.  The direct form sum_l (x_l - c_l)^2 in fp32 (one rounding for the
difference, a fused multiply-add per coordinate) is within (L + 2) u d^2 of the
exact value; the tests allow twice that.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _kmeans_oracle as ko

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 256            # guard elements on either side of every written buffer
RANGE = 1024         # rows of one workgroup of the update kernel (KM_RANGE)

#: (N, L, K, ldx): the shapes of the issue, an N that spans three update
#: ranges plus a ragged tail, and a row pitch above L
SHAPES = [
    (1000, 25, 20, 25), (4099, 100, 20, 100), (777, 2, 5, 2),
    (3000, 128, 64, 128), (2000, 1, 3, 1), (1, 1, 1, 1), (65, 7, 65, 7),
    (63, 256, 32, 256), (8192 + 5, 32, 256, 32), (3 * RANGE + 77, 10, 7, 10),
    (500, 25, 20, 40)]
FIT_SHAPES = SHAPES[:5]


def _id(shape):
    return "x".join(str(s) for s in shape)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Blob data, K distinct rows as start centres, and the oracle's assign
    against them -- computed once, read by every test of the shape."""
    n, latent_size, k, _ = shape
    x, planted, _ = ko.blobs(n, latent_size, k, seed=n + 31 * k)
    start = ko.distinct_rows(x, k, seed=7)
    d2 = ko.squared_distances(x, start)
    for array in (x, start, d2):
        array.setflags(write=False)
    return x, start, d2


@functools.lru_cache(maxsize=None)
def _oracle_fit(shape):
    x, start, _ = _case(shape)
    return ko.lloyd(x, start)


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


def _workspace(lib, n, latent_size, k, device):
    nbytes = lib.scvae_kmeans_workspace_bytes(n, latent_size, k)
    assert nbytes > 0
    return Guarded(nbytes, torch.uint8, device)


def device_assign(x, centres, ldx, device):
    from scvae_amd import _lib
    lib = _lib.load()
    n, latent_size = x.shape
    k = centres.shape[0]
    xd = _upload(x, ldx, device)
    cd = torch.from_numpy(np.array(centres)).to(device)
    labels = Guarded(n, torch.int32, device)
    min_d2 = Guarded(n, torch.float32, device)
    inertia = Guarded(1, torch.float64, device)
    workspace = _workspace(lib, n, latent_size, k, device)
    _lib.check(lib.scvae_kmeans_assign(
        _ptr(xd), ldx, n, latent_size, _ptr(cd), k, _ptr(labels.data),
        _ptr(min_d2.data), _ptr(inertia.data), _ptr(workspace.data),
        workspace.data.numel(), _stream(device)), "scvae_kmeans_assign")
    torch.cuda.synchronize()
    for buffer in (labels, min_d2, inertia, workspace):
        buffer.check()
    return (labels.data.cpu().numpy(), min_d2.data.cpu().numpy(),
            float(inertia.data.item()))


def device_update(x, labels, centres, ldx, device):
    from scvae_amd import _lib
    lib = _lib.load()
    n, latent_size = x.shape
    k = centres.shape[0]
    xd = _upload(x, ldx, device)
    cd = torch.from_numpy(np.array(centres)).to(device)
    ld = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(
        device)
    new = Guarded(k * latent_size, torch.float32, device)
    counts = Guarded(k, torch.int32, device)
    shift = Guarded(1, torch.float64, device)
    workspace = _workspace(lib, n, latent_size, k, device)
    _lib.check(lib.scvae_kmeans_update(
        _ptr(xd), ldx, n, latent_size, _ptr(ld), _ptr(cd), k, _ptr(new.data),
        _ptr(counts.data), _ptr(shift.data), _ptr(workspace.data),
        workspace.data.numel(), _stream(device)), "scvae_kmeans_update")
    torch.cuda.synchronize()
    for buffer in (new, counts, shift, workspace):
        buffer.check()
    return (new.data.cpu().numpy().reshape(k, latent_size),
            counts.data.cpu().numpy(), float(shift.data.item()))


def check_assign(d2, latent_size, labels, min_d2, inertia):
    """The assign contract of the issue against the fp64 distances d2 [N, K]."""
    n, k = d2.shape
    rel = 2 * (latent_size + 2) * U
    order = np.argsort(d2, axis=1, kind="stable")
    rows = np.arange(n)
    first = order[:, 0]
    d_first = d2[rows, first]
    print("min_d2 error / bound: {:.3f}".format(float(np.max(
        np.abs(min_d2 - d_first) / np.maximum(rel * d_first, 1e-300)
        * (d_first > 0)))))
    assert np.all(np.abs(min_d2 - d_first) <= rel * d_first)
    if k > 1:
        second = order[:, 1]
        d_second = d2[rows, second]
        ambiguous = (d_second - d_first) <= rel * (d_first + d_second)
        print("ambiguous rows: {} of {}".format(int(ambiguous.sum()), n))
        assert ambiguous.mean() <= 0.01
        assert np.array_equal(labels[~ambiguous], first[~ambiguous])
        assert np.all((labels[ambiguous] == first[ambiguous])
                      | (labels[ambiguous] == second[ambiguous]))
    else:
        assert np.all(labels == 0)
    want = float(d_first.sum())
    assert abs(inertia - want) <= rel * want


def centre_bound(x, labels, centres64):
    """|c - c64| <= 2^-23 |c64| + 2 * 2^-53 * sum_{i in k} |x_il|: the rounding
    of the mean to fp32 (half an ulp, 2^-24 |c64|, doubled), plus the fp64
    accumulation -- n_k additions in any order are within n_k 2^-53 sum|x| of
    the exact sum, 2^-53 sum|x| after the division by n_k -- once for the
    kernel and once for the oracle's own sum."""
    k = centres64.shape[0]
    absolute = np.zeros_like(centres64)
    np.add.at(absolute, labels, np.abs(x.astype(np.float64)))
    return 2.0 ** -23 * np.abs(centres64) + 2 * 2.0 ** -53 * absolute


def check_update(x, labels, old, new, counts, shift):
    k, latent_size = old.shape
    want, want_counts, want_shift = ko.update(x, labels, old)
    assert np.array_equal(counts, want_counts)
    bound = centre_bound(x, labels, want)
    filled = want_counts > 0
    error = np.abs(new.astype(np.float64) - want)
    print("centre error / bound: {:.3f}".format(float(
        (error[filled] / np.maximum(bound[filled], 1e-300)).max())))
    assert np.all(error[filled] <= bound[filled])
    # an empty cluster keeps its centre, bit for bit
    assert np.array_equal(new[~filled].view(np.uint32),
                          old[~filled].view(np.uint32))
    # the shift of centres that are each within `bound`, summed in fp64:
    # |d(sum (c - c0)^2)| <= sum 2 |c64 - c0| e + e^2, plus K L roundings
    moved = np.abs(want - old.astype(np.float64))
    bound[~filled] = 0.0
    shift_bound = float((2 * moved * bound + bound ** 2).sum()
                        + k * latent_size * 2.0 ** -52 * want_shift)
    assert abs(shift - want_shift) <= shift_bound
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_assign_and_update_against_oracle(cuda_device, shape):
    n, latent_size, k, ldx = shape
    x, start, d2 = _case(shape)
    labels, min_d2, inertia = device_assign(x, start, ldx, cuda_device)
    check_assign(d2, latent_size, labels, min_d2, inertia)
    new, counts, shift = device_update(x, labels, start, ldx, cuda_device)
    check_update(x, labels, start, new, counts, shift)


def test_update_keeps_the_centre_of_an_empty_cluster(cuda_device):
    """(3000, 128, 64) with four centres moved away from every row: no row
    takes them, and they come back bit-identical."""
    shape = SHAPES[3]
    n, latent_size, k, ldx = shape
    x, start, _ = _case(shape)
    centres = start.copy()
    empty = [0, 17, 40, 63]
    centres[empty] += np.float32(1000.0)
    labels, min_d2, inertia = device_assign(x, centres, ldx, cuda_device)
    check_assign(ko.squared_distances(x, centres), latent_size, labels,
                 min_d2, inertia)
    new, counts, shift = device_update(x, labels, centres, ldx, cuda_device)
    assert counts[empty].tolist() == [0, 0, 0, 0]
    assert np.array_equal(new[empty].view(np.uint32),
                          centres[empty].view(np.uint32))
    check_update(x, labels, centres, new, counts, shift)
    # the second iteration of the oracle's fit from `start` empties four
    # clusters by itself: its labels against the centres of the first
    history = _oracle_fit(shape)[4]
    centres = ko.update(x, history[0], start)[0].astype(np.float32)
    labels = history[1]
    empty = np.flatnonzero(np.bincount(labels, minlength=k) == 0)
    assert len(empty) == 4
    new, counts, shift = device_update(x, labels, centres, ldx, cuda_device)
    assert np.array_equal(new[empty].view(np.uint32),
                          centres[empty].view(np.uint32))
    check_update(x, labels, centres, new, counts, shift)


@pytest.mark.parametrize("n,latent_size,k", [(2000, 2, 12), (1500, 7, 5),
                                             (700, 130, 10)])
def test_exact_ties_take_the_lowest_index(cuda_device, n, latent_size, k):
    """Integer coordinates in [-8, 8]: every difference, square and sum is
    exact in fp32 (at most 130 * 16^2 < 2^24), so the distances are the
    integers and equal distances are exactly equal."""
    rng = np.random.default_rng(n)
    centres = rng.integers(-8, 9, size=(k, latent_size)).astype(np.float32)
    centres[3] = centres[1]                      # duplicated centres
    centres[k - 1] = centres[0]
    x = rng.integers(-8, 9, size=(n, latent_size)).astype(np.float32)
    # rows equidistant from centres 0 and 2 (and so from k - 1): centre 0
    # with its first coordinate moved half way towards a copy shifted by 4
    centres[2] = centres[0]
    centres[2, 0] = centres[0, 0] + (4 if centres[0, 0] <= 0 else -4)
    x[:10] = centres[0]
    x[:10, 0] = (centres[0, 0] + centres[2, 0]) / 2
    x[10:20] = centres[1]                        # on a duplicated centre
    d2 = ko.squared_distances(x, centres)
    want = d2.argmin(axis=1)
    ordered = np.sort(d2, axis=1)
    assert (ordered[:, 0] == ordered[:, 1]).sum() >= 20
    labels, min_d2, inertia = device_assign(x, centres, latent_size,
                                            cuda_device)
    assert np.array_equal(labels, want)
    assert np.array_equal(min_d2.astype(np.float64), ordered[:, 0])
    assert inertia == float(ordered[:, 0].sum())


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[7],
                                   SHAPES[9], SHAPES[10]], ids=_id)
def test_min_d2_update_against_oracle(cuda_device, shape):
    from scvae_amd import _lib
    lib = _lib.load()
    n, latent_size, k, ldx = shape
    x, _, _ = _case(shape)
    xd = _upload(x, ldx, cuda_device)
    rel = 2 * (latent_size + 2) * U
    min_d2 = Guarded(n, torch.float32, cuda_device)
    min_d2.data.fill_(float("inf"))
    want = np.full(n, np.inf)
    for row in (n // 3, n - 1, 0):
        _lib.check(lib.scvae_kmeans_min_d2_update(
            _ptr(xd), ldx, n, latent_size, row, _ptr(min_d2.data),
            _stream(cuda_device)), "scvae_kmeans_min_d2_update")
        torch.cuda.synchronize()
        min_d2.check()
        want = np.minimum(want, ko.squared_distances(x, x[row:row + 1])[:, 0])
        got = min_d2.data.cpu().numpy()
        assert np.all(np.abs(got - want) <= rel * want)
        assert got[row] == 0.0


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=_id)
def test_fit_follows_the_oracle_trajectory(cuda_device, shape):
    from scvae_amd.analyses.kmeans import DeviceKMeans
    n, latent_size, k, _ = shape
    x, start, _ = _case(shape)
    centres, labels, inertia, n_iter, _ = _oracle_fit(shape)
    model = DeviceKMeans(k, device=cuda_device).fit(x, initial_centres=start)
    print("iterations: device {}, oracle {}".format(model.n_iter_, n_iter))
    assert model.n_iter_ == n_iter
    assert np.array_equal(model.labels_, labels)
    assert model.labels_.dtype == np.int32
    assert model.cluster_centers_.dtype == np.float32
    # centres of clusters that hold rows at the end: means of those rows
    filled = np.bincount(labels, minlength=k) > 0
    bound = centre_bound(x, labels, centres)
    error = np.abs(model.cluster_centers_.astype(np.float64) - centres)
    assert np.all(error[filled] <= bound[filled])
    rel = 2 * (latent_size + 2) * U
    assert abs(model.inertia_ - inertia) <= rel * inertia
    assert np.array_equal(model.predict(x), model.labels_)


def test_fits_repeat_bit_for_bit(cuda_device):
    from scvae_amd.analyses.kmeans import DeviceKMeans
    shape = SHAPES[1]
    x, start, _ = _case(shape)
    k = shape[2]

    def same(a, b):
        assert np.array_equal(a.cluster_centers_.view(np.uint32),
                              b.cluster_centers_.view(np.uint32))
        assert np.array_equal(a.labels_, b.labels_)
        assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_
    same(DeviceKMeans(k, device=cuda_device).fit(x, initial_centres=start),
         DeviceKMeans(k, device=cuda_device).fit(x, initial_centres=start))
    seeded = [DeviceKMeans(k, n_init=2, seed=11, device=cuda_device).fit(x)
              for _ in range(2)]
    same(*seeded)
    assert seeded[0].seed_rows_ == seeded[1].seed_rows_


def test_seeding_and_planted_partition(cuda_device):
    from scvae_amd.analyses.kmeans import DeviceKMeans
    n, latent_size, k = 2000, 10, 8
    x, planted, _ = ko.blobs(n, latent_size, k, seed=5, spread=10.0)
    assert len(np.unique(x, axis=0)) == n
    model = DeviceKMeans(k, n_init=10, seed=0, device=cuda_device).fit(x)
    assert len(model.seed_rows_) == 10
    for rows in model.seed_rows_:     # rows of X, pairwise distinct
        assert len(rows) == k and len(set(rows)) == k
        assert all(0 <= row < n for row in rows)
    assert ko.adjusted_rand_index(planted, model.labels_) == 1.0
    assert ko.adjusted_rand_index(planted, model.predict(x)) == 1.0
    # fewer rows than clusters to predict
    assert np.array_equal(model.predict(x[:3]), model.labels_[:3])
    with pytest.raises(ValueError, match="finite"):
        DeviceKMeans(2, device=cuda_device).fit(
            np.array([[0.0], [np.nan], [1.0]]))


def test_cli_evaluate_with_prediction_on_device(tmp_path, cuda_device,
                                                capsys):
    """``scvae evaluate -P k-means --prediction-on-device``: the same lines
    and attachments as without the switch, the clustering from the device."""
    from scvae_amd import cli
    from scvae_amd.analyses import kmeans, prediction
    arguments = ["synthetic_1k", "-M", str(tmp_path), "-r", "poisson", "-l",
                 "3", "-H", "20", "-B", "100", "--split-data-set"]
    cli.main(["train"] + arguments + ["-e", "2"])
    capsys.readouterr()
    fits = []
    fit = kmeans.DeviceKMeans.fit

    def recording_fit(self, values, initial_centres=None):
        fits.append(np.asarray(values).shape)
        return fit(self, values, initial_centres)
    kmeans.DeviceKMeans.fit = recording_fit
    try:
        results = cli.main(["evaluate"] + arguments + [
            "-P", "k-means", "--prediction-on-device"])
    finally:
        kmeans.DeviceKMeans.fit = fit
    out = capsys.readouterr().out
    assert len(fits) == 1 and fits[0][1] == 3
    assert "Prediction method: k-means." in out
    assert "Predicting labels for evaluation set using k-means" in out
    assert "k-means on the device not used" not in out
    transformed, reconstructed, latent = results["end_of_training"]
    for version in (transformed, reconstructed, latent["z"]):
        assert version.prediction_specifications.name.startswith("kmeans_")
        assert len(version.predicted_cluster_ids) == 100
        if transformed.has_labels:
            assert len(version.predicted_labels) == 100
    if transformed.has_labels:
        assert "adjusted Rand index" in out

    # sizes over the limit (K L > 8192): one line, then scikit-learn
    rng = np.random.default_rng(0)

    class Stub:
        kind = "training"
        has_labels = False
        number_of_examples = 90
        values = rng.standard_normal((90, 250))
    cluster_ids, _, _ = prediction.predict_labels(
        Stub(), Stub(), method="k-means", number_of_clusters=40,
        on_device=True)
    out = capsys.readouterr().out
    assert out.count("k-means on the device not used") == 1
    assert len(cluster_ids) == 90
