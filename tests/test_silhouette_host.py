"""Host side of the device silhouette: the fp64 oracle the GPU tests compare
against is pinned to scikit-learn's ``silhouette_samples``, ``limit_reason``
agrees with the C entries, the ``nan`` rule needs no GPU, and
``--silhouette-score`` reaches ``evaluate`` and ``_predict``."""
import ctypes
import math

import numpy
import pytest

import _silhouette_oracle as so


@pytest.mark.parametrize("name", sorted(so.all_cases()))
def test_oracle_follows_scikit_learn(name):
    """On fp64 copies of the GPU cases, to 1e-9 absolute: scikit-learn takes
    its distances in the expanded form |x|^2 - 2 x.y + |y|^2 (worst seen
    9.1e-11), the oracle in the direct form.  The four identical rows split
    over two clusters are left out: the expanded form may give a small
    non-zero distance where the true one is 0, and with a = b = 0 that
    rounding alone would decide s."""
    metrics = pytest.importorskip("sklearn.metrics")
    x, labels, _ = so.all_cases()[name]
    x64 = numpy.array(x, dtype=numpy.float64)
    a, b, s = so.expected(name)
    want = metrics.silhouette_samples(x64, labels)
    exact = numpy.ones(len(s), dtype=bool)
    if name == "duplicates":
        # exact zeros are the point of this case: the oracle alone decides
        assert numpy.all(s[:100] == 1.0) and numpy.all(s[100:] == 0.0)
        assert numpy.all(a == 0.0) and numpy.all(b[100:] == 0.0)
        assert numpy.all(b[:100] > 0.0)
        exact[100:] = False
    error = numpy.abs(s - want)[exact]
    print("worst |s - scikit-learn|: {:.3g}".format(
        float(error.max()) if error.size else 0.0))
    assert numpy.all(error <= 1e-9)
    assert numpy.all(a >= 0.0) and numpy.all(b >= 0.0)
    assert numpy.all(numpy.abs(s) <= 1.0)


def test_oracle_cases_cover_what_they_claim():
    x, labels = so.blob_case((65, 7, 64, 7))
    counts = numpy.bincount(labels)
    assert sorted(counts.tolist()) == [1] * 63 + [2]
    pair = numpy.flatnonzero(labels == numpy.argmax(counts))
    assert numpy.array_equal(x[pair[0]], x[pair[1]])
    a, b, s = so.expected("65x7x64x7")
    assert numpy.all(s[counts[labels] == 1] == 0.0)
    assert numpy.all(s[pair] == 1.0)
    x, labels = so.edge_case()
    assert numpy.bincount(labels).tolist() == [1, 63, 64, 65, 129]
    for name in ("1000x25x20x25", "2051x100x20x100", "777x2x5x2"):
        s = so.expected(name)[2]
        assert (s > 0.05).any() and (s < -0.05).any(), name


#: every limit with the first value on each side of it
LIMIT_CASES = [
    ((1000, 0, 20), False), ((1000, 1, 20), True), ((1000, 256, 20), True),
    ((1000, 257, 20), False), ((2, 4, 2), False), ((3, 4, 2), True),
    ((2 ** 31 - 1, 4, 2), True), ((2 ** 31, 4, 2), False),
    ((1000, 4, 1), False), ((1000, 4, 2), True), ((1000, 4, 999), True),
    ((1000, 4, 1000), False), ((3, 1, 3), False), ((1000, 25, 20), True)]


@pytest.mark.parametrize("sizes,inside", LIMIT_CASES)
def test_limit_reason_and_the_entries_agree(sizes, inside):
    from scvae_amd import _lib
    from scvae_amd.analyses.silhouette import limit_reason
    lib = _lib.load()
    reason = limit_reason(*sizes)
    assert (reason is None) == inside
    nbytes = lib.scvae_silhouette_workspace_bytes(*sizes)
    assert (nbytes > 0) == inside
    if inside:
        assert nbytes >= 4 * sizes[0] and nbytes % 8 == 0
    else:
        assert nbytes == -1 and isinstance(reason, str) and reason
        assert "bad argument" in lib.scvae_last_error().decode()


def test_limit_reason_names_the_limit():
    from scvae_amd.analyses.silhouette import limit_reason
    assert "latent size 257" in limit_reason(1000, 257, 20)
    assert "2 cells" in limit_reason(2, 4, 2)
    assert "2^31" in limit_reason(2 ** 31, 4, 2)
    assert "1 clusters" in limit_reason(1000, 4, 1)
    assert "1000 clusters for 1000 cells" in limit_reason(1000, 4, 1000)


def test_entry_refuses_bad_arguments_without_a_gpu():
    """-1 and a message naming the limit; every pointer and size is checked
    before anything is launched."""
    from scvae_amd import _lib
    lib = _lib.load()
    buffer = (ctypes.c_double * 64)()
    p = ctypes.cast(buffer, ctypes.c_void_p)
    big = 1 << 40

    def entry(n, latent_size, k, x=p, offsets=p, score=p, workspace=p,
              nbytes=big, ldx=None):
        return lib.scvae_silhouette_samples(
            x, latent_size if ldx is None else ldx, n, latent_size, offsets,
            k, None, None, None, score, workspace, nbytes, None)
    for sizes, limit in (((1000, 257, 20), "L <="), ((1000, 0, 20), "L >= 1"),
                         ((1000, 4, 1), "K >= 2"), ((1000, 4, 1000), "K <= N"),
                         ((2, 4, 2), "N >= 3"), ((1 << 31, 4, 2), "N <")):
        assert entry(*sizes) == -1, sizes
        message = lib.scvae_last_error().decode()
        assert "bad argument" in message and limit in message, message
    for name in ("x", "offsets", "score", "workspace"):
        assert entry(100, 4, 3, **{name: None}) == -1, name
        assert "bad argument" in lib.scvae_last_error().decode()
    need = lib.scvae_silhouette_workspace_bytes(100, 4, 3)
    assert entry(100, 4, 3, nbytes=need - 1) == -1
    assert "workspace_bytes" in lib.scvae_last_error().decode()
    assert entry(100, 4, 3, ldx=3) == -1


def test_score_is_nan_outside_the_cluster_counts_without_a_gpu(monkeypatch):
    """Fewer than 2 or more than N - 1 distinct labels: the reference's rule
    (clustering.py:125-127), answered before anything touches the device."""
    from scvae_amd.analyses import silhouette

    def never(*arguments, **keyword_arguments):
        raise AssertionError("the device path was entered")
    monkeypatch.setattr(silhouette, "_run", never)
    monkeypatch.setattr(silhouette._lib, "load", never)
    values = numpy.arange(20.0, dtype=numpy.float32).reshape(10, 2)
    assert math.isnan(silhouette.silhouette_score(values, [4] * 10))
    assert math.isnan(silhouette.silhouette_score(values, numpy.arange(10)))
    assert math.isnan(silhouette.silhouette_score(
        values, ["a", "b", "c", "d", "e", "f", "g", "h", "i", "j"]))


def test_device_silhouette_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib, analyses
    values = numpy.arange(20.0, dtype=numpy.float32).reshape(10, 2)
    labels = [0, 1] * 5
    for function in (analyses.silhouette_samples, analyses.silhouette_score):
        with pytest.raises(_lib.HipLibraryError, match="no CPU path") as info:
            function(values, labels)
        assert "No GPU visible" in str(info.value)
        assert "silhouette" in str(info.value)


def test_wrapper_checks_its_input_before_the_device(monkeypatch):
    from scvae_amd.analyses import silhouette
    values = numpy.zeros((10, 2), dtype=numpy.float32)
    with pytest.raises(ValueError, match="finite"):
        silhouette.silhouette_samples(
            numpy.array([[0.0], [numpy.nan], [1.0]]), [0, 1, 0])
    with pytest.raises(ValueError, match="9 labels for 10 rows"):
        silhouette.silhouette_samples(values, [0, 1, 0] * 3)
    with pytest.raises(ValueError, match="matrix"):
        silhouette.silhouette_samples(numpy.zeros(10), [0, 1] * 5)
    # sizes outside the limits are a ValueError naming the limit (with a GPU
    # in sight; without one the missing GPU is reported first)
    monkeypatch.setattr(silhouette.torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match="latent size 300"):
        silhouette.silhouette_samples(
            numpy.zeros((10, 300), dtype=numpy.float32), [0, 1] * 5)
    with pytest.raises(ValueError, match="1 clusters for 10 cells"):
        silhouette.silhouette_samples(values, [3] * 10)


class _LatentSet:
    kind = "test"
    has_labels = False
    number_of_examples = 12
    excluded_classes = ()

    def __init__(self):
        rng = numpy.random.default_rng(3)
        self.values = rng.standard_normal((12, 2))
        self.updates = []

    def update_predictions(self, **keyword_arguments):
        self.updates.append(keyword_arguments)


def test_silhouette_score_switch_reaches_evaluate_and_predict(monkeypatch,
                                                              capsys):
    from scvae_amd import cli
    from scvae_amd.analyses import prediction, silhouette

    # the flag parses and is handed to evaluate()
    seen = []
    monkeypatch.setattr(cli, "evaluate", lambda **kw: seen.append(kw) or 0)
    cli.main(["evaluate", "some_data", "-P", "k-means", "--silhouette-score"])
    cli.main(["evaluate", "some_data", "-P", "k-means"])
    assert [kw["silhouette_score"] for kw in seen] == [True, False]
    assert [kw["prediction_on_device"] for kw in seen] == [False, False]

    # _predict prints the lines after the metrics, from the latent values z
    cluster_ids = numpy.array([0, 1, 2] * 4, dtype=numpy.int32)

    def predict(training_set, evaluation_set, specifications=None,
                on_device=False, **rest):
        return cluster_ids, predict.labels, None
    monkeypatch.setattr(prediction, "predict_labels", predict)
    calls = []

    def score(values, labels, device=None):
        calls.append((numpy.asarray(values), numpy.asarray(labels)))
        return 0.25 if len(calls) % 2 else -0.125
    monkeypatch.setattr(silhouette, "silhouette_score", score)

    class Model:
        def evaluate(self, **keyword_arguments):
            return {"z": _LatentSet()}
    specifications = prediction.PredictionSpecifications(
        "k-means", number_of_clusters=3, training_set_kind="training")

    def run(labelled, **switch):
        sets = [_LatentSet() for _ in range(3)]
        if labelled:
            names = numpy.array(["p", "q", "q"] * 4)
            for s in sets:
                s.has_labels, s.labels = True, names
            predict.labels = numpy.array(["p", "q", "p"] * 4)
        else:
            predict.labels = None
        del calls[:]
        capsys.readouterr()
        cli._predict(Model(), [sets[0], sets[1], {"z": sets[2]}],
                     _LatentSet(), specifications, 4, None, False, False,
                     "end_of_training", **switch)
        return sets[2], capsys.readouterr().out.splitlines()

    latent, lines = run(False, silhouette_score=True)
    assert len(calls) == 1
    assert numpy.array_equal(calls[0][0], latent.values)
    assert numpy.array_equal(calls[0][1], cluster_ids)
    at = lines.index("Clustering of the test set (kmeans_3):")
    assert lines[at + 1] == "    silhouette score (clusters): 0.2500"
    assert not any("(labels)" in line for line in lines)

    latent, lines = run(True, silhouette_score=True)
    assert len(calls) == 2
    assert numpy.array_equal(calls[1][1], predict.labels)
    assert lines.count("Clustering of the test set (kmeans_3):") == 1
    at = lines.index("    silhouette score (clusters): 0.2500")
    assert lines[at - 1].startswith("    accuracy:")
    assert lines[at + 1] == "    silhouette score (labels): -0.1250"

    for switch in ({}, {"silhouette_score": False}):
        for labelled in (False, True):
            _, lines = run(labelled, **switch)
            assert not calls
            assert not any("silhouette" in line for line in lines)
            assert any(line.startswith("Clustering of") for line in lines) \
                == labelled


def test_metric_falls_back_to_scikit_learn_outside_the_limits(monkeypatch,
                                                              capsys):
    """Latent size 300: one line saying why, then what the reference
    computes; inside the limits the device call, and ``nan`` by the
    reference's rule before either."""
    metrics = pytest.importorskip("sklearn.metrics")
    from scvae_amd.analyses import prediction, silhouette
    calls = []

    def score(values, labels, device=None):
        calls.append(numpy.asarray(values).shape)
        return 0.5
    monkeypatch.setattr(silhouette, "silhouette_score", score)
    rng = numpy.random.default_rng(0)
    wide = rng.standard_normal((80, 300))
    labels = rng.integers(4, size=80)
    got = prediction.silhouette_metric(wide, labels)
    out = capsys.readouterr().out
    assert out == ("silhouette score on the device not used: latent size 300 "
                   "(1 to 256 supported).\n")
    assert not calls
    assert got == pytest.approx(
        float(metrics.silhouette_score(wide, labels)), abs=1e-12)
    assert prediction.silhouette_metric(wide[:, :20], labels) == 0.5
    assert calls == [(80, 20)]
    assert capsys.readouterr().out == ""
    assert math.isnan(prediction.silhouette_metric(wide, [1] * 80))
    assert math.isnan(prediction.silhouette_metric(wide, numpy.arange(80)))
    assert capsys.readouterr().out == "" and calls == [(80, 20)]
    # above 20 000 cells the host path samples 20 000, as the reference does
    seen = {}

    def sampled(X, labels, sample_size=None):
        seen["sample_size"] = sample_size
        return 0.0
    monkeypatch.setattr(metrics, "silhouette_score", sampled)
    prediction.silhouette_metric(numpy.zeros((20001, 300)),
                                 numpy.arange(20001) % 3)
    assert seen["sample_size"] == 20000
    prediction.silhouette_metric(numpy.zeros((20000, 300)),
                                 numpy.arange(20000) % 3)
    assert seen["sample_size"] is None
