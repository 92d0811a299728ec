"""Host side of the device k-means: the fp64 oracle the GPU tests compare
against is pinned to scikit-learn's Lloyd, the C entries refuse sizes outside
their limits without touching a GPU, and ``--prediction-on-device`` reaches
``predict_labels``."""
import ctypes

import numpy
import pytest

import _kmeans_oracle as ko


@pytest.mark.parametrize("n,latent_size,k,tol", [
    (1000, 25, 20, 1e-4), (777, 2, 5, 1e-4), (2000, 1, 3, 1e-4),
    (1500, 10, 8, 0.0)])
def test_oracle_follows_scikit_learn_lloyd(n, latent_size, k, tol):
    """Same start, no cluster empties: the oracle and
    ``KMeans(init=C0, n_init=1, algorithm="lloyd")`` give the same labels and
    iteration count, centres and inertia to 1e-10 relative."""
    cluster = pytest.importorskip("sklearn.cluster")
    x, _, _ = ko.blobs(n, latent_size, k, seed=n + k)
    x = x.astype(numpy.float64)
    start = ko.distinct_rows(x, k, seed=1)
    centres, labels, inertia, n_iter, history = ko.lloyd(x, start, tol=tol)
    for step in history:   # the precondition of the comparison
        assert numpy.bincount(step, minlength=k).min() > 0
    model = cluster.KMeans(n_clusters=k, init=start, n_init=1,
                           algorithm="lloyd", tol=tol, max_iter=300).fit(x)
    assert numpy.array_equal(model.labels_, labels)
    assert model.n_iter_ == n_iter
    scale = numpy.abs(centres).max()
    assert numpy.abs(model.cluster_centers_ - centres).max() <= 1e-10 * scale
    assert abs(model.inertia_ - inertia) <= 1e-10 * inertia


def test_oracle_rules():
    """Lowest index on equal distances; an empty cluster keeps its centre."""
    x = numpy.array([[0.0, 0.0], [2.0, 0.0], [1.0, 0.0]])
    centres = numpy.array([[2.0, 0.0], [0.0, 0.0], [0.0, 0.0], [9.0, 9.0]])
    labels, d2, inertia = ko.assign(x, centres)
    assert labels.tolist() == [1, 0, 0] and d2.tolist() == [0.0, 0.0, 1.0]
    assert inertia == 1.0
    new, counts, shift = ko.update(x, labels, centres)
    assert counts.tolist() == [2, 1, 0, 0]
    assert new.tolist() == [[1.5, 0.0], [0.0, 0.0], [0.0, 0.0], [9.0, 9.0]]
    assert shift == 0.25
    assert ko.adjusted_rand_index([0, 0, 1, 1], [3, 3, 5, 5]) == 1.0
    assert ko.adjusted_rand_index([0, 0, 1, 1], [0, 1, 0, 1]) < 0.0


def _last_error(lib):
    return lib.scvae_last_error().decode()


def test_kmeans_entries_refuse_sizes_outside_the_limits():
    """-1 and a message naming the limit, with no GPU needed (every pointer is
    checked before anything is launched)."""
    from scvae_amd import _lib
    lib = _lib.load()
    buffer = (ctypes.c_double * 64)()
    p = ctypes.cast(buffer, ctypes.c_void_p)
    big = 1 << 30

    def assign(n, latent_size, k, x=p, centres=p, labels=p, inertia=p,
               workspace=p):
        return lib.scvae_kmeans_assign(
            x, latent_size, n, latent_size, centres, k, labels, None, inertia,
            workspace, big, None)

    def update(n, latent_size, k, x=p, labels=p, centres=p, new=p, counts=p,
               shift=p, workspace=p):
        return lib.scvae_kmeans_update(
            x, latent_size, n, latent_size, labels, centres, k, new, counts,
            shift, workspace, big, None)

    assert lib.scvae_kmeans_workspace_bytes(1000, 25, 20) > 0
    for entry in (assign, update, lib.scvae_kmeans_workspace_bytes):
        for sizes, limit in (((10, 4, 11), "K <= N"),
                             ((1000, 100, 100), "K * L <="),
                             ((1000, 257, 2), "L <="),
                             ((1000, 2, 257), "K <="),
                             ((1 << 31, 2, 2), "N <"),
                             ((0, 2, 0), "N >= 1")):
            assert entry(*sizes) == -1, (entry, sizes)
            assert "bad argument" in _last_error(lib)
            assert limit in _last_error(lib), (_last_error(lib), limit)
    for name in ("x", "centres", "labels", "inertia", "workspace"):
        assert assign(100, 4, 3, **{name: None}) == -1, name
        assert "bad argument" in _last_error(lib)
    for name in ("x", "labels", "centres", "new", "counts", "shift",
                 "workspace"):
        assert update(100, 4, 3, **{name: None}) == -1, name
        assert "bad argument" in _last_error(lib)
    # a workspace smaller than scvae_kmeans_workspace_bytes, a pitch below L
    assert lib.scvae_kmeans_assign(p, 4, 100, 4, p, 3, p, None, p, p, 64,
                                   None) == -1
    assert lib.scvae_kmeans_assign(p, 3, 100, 4, p, 3, p, None, p, p, big,
                                   None) == -1
    assert lib.scvae_kmeans_min_d2_update(None, 4, 100, 4, 0, p, None) == -1
    assert lib.scvae_kmeans_min_d2_update(p, 4, 100, 4, 0, None, None) == -1
    assert lib.scvae_kmeans_min_d2_update(p, 4, 100, 4, 100, p, None) == -1
    assert lib.scvae_kmeans_min_d2_update(p, 257, 100, 257, 0, p, None) == -1
    assert "L <=" in _last_error(lib)


def test_limit_reason_matches_the_entries():
    from scvae_amd import _lib
    from scvae_amd.analyses.kmeans import limit_reason
    lib = _lib.load()
    for sizes in ((1000, 25, 20), (1, 1, 1), (8197, 32, 256), (10, 4, 11),
                  (1000, 100, 100), (1000, 257, 2), (1000, 2, 257),
                  (300, 256, 32), (300, 33, 256)):
        inside = lib.scvae_kmeans_workspace_bytes(*sizes) > 0
        assert (limit_reason(*sizes) is None) == inside, sizes


def test_device_kmeans_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib
    from scvae_amd.analyses.kmeans import DeviceKMeans
    with pytest.raises(_lib.HipLibraryError, match="no CPU path"):
        DeviceKMeans(3).fit(numpy.zeros((10, 2), dtype=numpy.float32))


class _LatentSet:
    kind = "training"
    has_labels = False
    number_of_examples = 12

    def __init__(self):
        self.values = numpy.arange(24.0).reshape(12, 2)
        self.updates = []

    def update_predictions(self, **keyword_arguments):
        self.updates.append(keyword_arguments)


def test_prediction_on_device_switch_reaches_predict_labels(monkeypatch):
    from scvae_amd import cli
    from scvae_amd.analyses import prediction
    assert set(prediction.PREDICTION_METHODS) == {"k-means", "model"}

    # the flag parses and is handed to evaluate()
    seen = []
    monkeypatch.setattr(cli, "evaluate", lambda **kw: seen.append(kw) or 0)
    cli.main(["evaluate", "some_data", "-P", "k-means",
              "--prediction-on-device"])
    cli.main(["evaluate", "some_data", "-P", "k-means"])
    assert [kw["prediction_on_device"] for kw in seen] == [True, False]
    assert seen[0]["prediction_method"] == "k-means"

    # _predict hands it to predict_labels
    calls = []

    def record(training_set, evaluation_set, specifications=None,
               on_device=False, **rest):
        calls.append(on_device)
        return numpy.zeros(12, dtype=numpy.int32), None, None
    monkeypatch.setattr(prediction, "predict_labels", record)

    class Model:
        def evaluate(self, **keyword_arguments):
            return {"z": _LatentSet()}
    specifications = prediction.PredictionSpecifications(
        "k-means", number_of_clusters=3, training_set_kind="training")
    for on_device in (True, False, None):
        sets = [_LatentSet() for _ in range(3)]
        arguments = (Model(), [sets[0], sets[1], {"z": sets[2]}],
                     _LatentSet(), specifications, 4, None, False, False,
                     "end_of_training")
        if on_device is None:
            cli._predict(*arguments)
        else:
            cli._predict(*arguments, on_device=on_device)
        assert all(len(s.updates) == 1 for s in sets)
    assert calls == [True, False, False]


def test_predict_labels_passes_on_device_to_the_method(monkeypatch):
    from scvae_amd.analyses import prediction
    calls = []

    def method(training_set, evaluation_set, number_of_clusters,
               on_device=False):
        calls.append(on_device)
        return numpy.zeros(12, dtype=numpy.int32), None, None
    for name in ("k-means", "model"):
        monkeypatch.setitem(prediction.PREDICTION_METHODS[name], "function",
                            method)
    sets = _LatentSet(), _LatentSet()
    prediction.predict_labels(*sets, method="k-means", number_of_clusters=3,
                              on_device=True)
    prediction.predict_labels(*sets, method="k-means", number_of_clusters=3)
    prediction.predict_labels(*sets, method="model", number_of_clusters=3,
                              on_device=True)
    assert calls == [True, False, True]
    assert set(prediction.PREDICTION_METHODS) == {"k-means", "model"}


def test_switch_falls_back_to_scikit_learn_outside_the_limits(capsys):
    """K L > 8192: one line saying why, then scikit-learn as without the
    switch (no GPU is touched)."""
    pytest.importorskip("sklearn")
    from scvae_amd.analyses import prediction
    rng = numpy.random.default_rng(0)

    class Wide(_LatentSet):
        number_of_examples = 80

        def __init__(self):
            super().__init__()
            self.values = rng.standard_normal((80, 300))
    cluster_ids, _, _ = prediction.predict_labels(
        Wide(), Wide(), method="k-means", number_of_clusters=40,
        on_device=True)
    out = capsys.readouterr().out
    assert out.count("k-means on the device not used") == 1
    assert "latent size 300" in out
    assert "Predicting labels for evaluation set using k-means" in out
    assert len(cluster_ids) == 80 and set(cluster_ids) <= set(range(40))
