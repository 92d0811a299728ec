"""Host side of the count-space silhouette: the int64 / fp64 oracle the GPU
tests compare against is pinned to scikit-learn's ``silhouette_samples``,
sampling follows ``sklearn.metrics.silhouette_score(sample_size=)``,
``limit_reason`` agrees with the C entries, the ``nan`` rule needs no GPU,
and ``--silhouette-space`` reaches ``evaluate`` and ``_predict``."""
import ctypes
import math

import numpy
import pytest
import scipy.sparse

import _count_silhouette_oracle as co

#: the worst |s - scikit-learn| seen over the cases below (257x257x2; with
#: integer inputs scikit-learn's expanded form is exact in fp64 as well, and
#: what is left is the order of the sums)
WORST_SEEN_AGAINST_SCIKIT_LEARN = 1.05e-15


@pytest.mark.parametrize("name", sorted(co.all_cases()))
def test_oracle_follows_scikit_learn(name):
    """On fp64 copies of the GPU cases.  scikit-learn takes its distances in
    the expanded form |x|^2 - 2 x.y + |y|^2 in fp64, the oracle from exact
    integers; the worst difference of s seen on the CPU this was written on
    is WORST_SEEN_AGAINST_SCIKIT_LEARN (printed per case), and ten times that
    is allowed.  Left out: the saturated case and the rows of the other cases
    that have an identical twin -- the expanded form may give a small
    non-zero distance where the true one is 0, and where a or b is 0 that
    rounding alone decides s."""
    metrics = pytest.importorskip("sklearn.metrics")
    if name == "saturated":
        a, b, s = co.expected(name)
        assert numpy.all(a[:10] == 0.0) and numpy.all(b[:4] == 0.0)
        assert numpy.all(s[:4] == 0.0) and numpy.all(s[4:10] == 1.0)
        assert numpy.all(b[10:] == 0.0) and numpy.all(s[10:] == -1.0)
        d2 = co.expected_squared_distances(name)
        assert d2[0, 4] == 520 * 65535 ** 2 and d2.dtype == numpy.int64
        return
    x, labels, _ = co.all_cases()[name]
    a, b, s = co.expected(name)
    want = metrics.silhouette_samples(x.astype(numpy.float64), labels)
    d2 = co.expected_squared_distances(name)
    twins = (d2 == 0).sum(axis=1) > 1
    assert twins.sum() == (2 if name in ("65x515x64", "1000x2000x999") else 0)
    error = numpy.abs(s - want)[~twins]
    print("worst |s - scikit-learn|: {:.3g}".format(float(error.max())))
    assert numpy.all(error <= 10 * WORST_SEEN_AGAINST_SCIKIT_LEARN)
    assert numpy.all(a >= 0.0) and numpy.all(b >= 0.0)
    assert numpy.all(numpy.abs(s) <= 1.0)
    assert numpy.all(s[twins] == 1.0) and numpy.all(a[twins] == 0.0)


def test_oracle_cases_cover_what_they_claim():
    x, labels, ldx = co.all_cases()["65x515x64"]
    counts = numpy.bincount(labels)
    assert sorted(counts.tolist()) == [1] * 63 + [2]
    pair = numpy.flatnonzero(labels == numpy.argmax(counts))
    assert numpy.array_equal(x[pair[0]], x[pair[1]])
    x, labels, _ = co.all_cases()["1000x2000x999"]
    assert len(numpy.unique(labels)) == 999
    x, labels, _ = co.all_cases()["edges"]
    assert numpy.bincount(labels).tolist() == [1, 63, 64, 65, 129]
    assert x.shape == (322, 70)
    x, labels, ldx = co.all_cases()["200x32738x20"]
    assert x.max() >= 1000 and ldx == 32768
    gram = x.astype(numpy.int64) @ x.astype(numpy.int64).T
    assert gram.max() > 2 ** 24     # no single fp32 sum could carry it
    for name, (x, labels, ldx) in co.all_cases().items():
        assert x.dtype == numpy.uint16 and labels.shape == (x.shape[0],)
        assert ldx % 8 == 0 and ldx >= (x.shape[1] + 63) // 64 * 64, name
    for name in ("130x300x5", "200x32738x20", "edges"):
        s = co.expected(name)[2]
        assert (s > 0.02).any() and (s < -0.02).any(), name


def test_sampling_scores_the_rows_scikit_learn_would(monkeypatch):
    """``count_silhouette_score(sample_size=m, random_state=r)`` hands
    exactly the rows ``RandomState(r).permutation(N)[:m]`` and their labels
    to the device call, sparse or dense."""
    from scvae_amd.analyses import count_silhouette
    x, labels, _ = co.all_cases()["130x300x5"]
    seen = []

    def run(values, given, device):
        dense = values.toarray() if hasattr(values, "toarray") else values
        seen.append((numpy.array(dense), numpy.array(given)))
        return None, 0.125
    monkeypatch.setattr(count_silhouette, "_run", run)
    for values in (x, scipy.sparse.csr_matrix(x.astype(numpy.float32))):
        for m, r in ((50, 3), (129, 0), (130, 7)):
            del seen[:]
            assert count_silhouette.count_silhouette_score(
                values, labels, sample_size=m, random_state=r) == 0.125
            chosen = numpy.random.RandomState(r).permutation(130)[:m]
            assert len(seen) == 1
            assert numpy.array_equal(seen[0][0], x[chosen])
            assert numpy.array_equal(seen[0][1], labels[chosen])
    del seen[:]
    count_silhouette.count_silhouette_score(x, labels)
    assert numpy.array_equal(seen[0][0], x)
    # a sample with one cluster left, or with as many clusters as rows:
    # scikit-learn's error
    lopsided = numpy.zeros(130, dtype=numpy.int64)
    lopsided[0] = 1
    chosen = numpy.random.RandomState(0).permutation(130)[:5]
    assert 0 not in chosen
    with pytest.raises(ValueError, match="Number of labels is 1"):
        count_silhouette.count_silhouette_score(
            x, lopsided, sample_size=5, random_state=0)
    with pytest.raises(ValueError, match="Number of labels is 2"):
        count_silhouette.count_silhouette_score(
            x, numpy.arange(130) % 129, sample_size=2, random_state=0)


#: every limit with the first value on each side of it: (N, F, K)
LIMIT_CASES = [
    ((1000, 0, 20), False), ((1000, 1, 20), True), ((1000, 65536, 20), True),
    ((1000, 65537, 20), False), ((2, 4, 2), False), ((3, 4, 2), True),
    ((2 ** 20, 4, 2), True), ((2 ** 20 + 1, 4, 2), False),
    ((1000, 4, 1), False), ((1000, 4, 2), True), ((1000, 4, 999), True),
    ((1000, 4, 1000), False), ((3, 1, 3), False), ((20000, 32738, 20), True)]


@pytest.mark.parametrize("sizes,inside", LIMIT_CASES)
def test_limit_reason_and_the_entries_agree(sizes, inside):
    from scvae_amd import _lib
    from scvae_amd.analyses.count_silhouette import limit_reason
    lib = _lib.load()
    reason = limit_reason(*sizes)
    assert (reason is None) == inside
    nbytes = lib.scvae_count_silhouette_workspace_bytes(*sizes)
    assert (nbytes > 0) == inside
    n = sizes[0]
    if inside:
        pitch = (n + 15) // 16 * 16
        fixed = 8 * n + (4 * n + 7) // 8 * 8
        assert nbytes % 8 == 0
        assert nbytes >= fixed + min(n, 128) * 4 * pitch
        # the strip is bounded, not N^2
        assert nbytes <= fixed + max(256 << 20, 128 * 4 * pitch)
    else:
        assert nbytes == -1 and isinstance(reason, str) and reason
        assert "bad argument" in lib.scvae_last_error().decode()


def test_limit_reason_names_the_limit():
    from scvae_amd.analyses.count_silhouette import limit_reason
    assert "65537 features" in limit_reason(1000, 65537, 20)
    assert "0 features" in limit_reason(1000, 0, 20)
    assert "2 cells" in limit_reason(2, 4, 2)
    assert "2^20" in limit_reason(2 ** 20 + 1, 4, 2)
    assert "1 clusters" in limit_reason(1000, 4, 1)
    assert "1000 clusters for 1000 cells" in limit_reason(1000, 4, 1000)
    # the stored values: integers in [0, 65 535]
    ok = numpy.array([[0, 65535], [3, 4], [5, 6]])
    assert limit_reason(3, 2, 2, ok.astype(numpy.float32)) is None
    assert limit_reason(3, 2, 2, scipy.sparse.csr_matrix(ok)) is None
    assert "not integers" in limit_reason(3, 2, 2, ok + 0.5)
    assert "outside 0 to 65535" in limit_reason(3, 2, 2, ok + 1)
    assert "outside 0 to 65535" in limit_reason(3, 2, 2, ok - 1)
    assert "not finite" in limit_reason(
        3, 2, 2, numpy.array([[0.0, numpy.inf]] * 3))
    sparse = scipy.sparse.csr_matrix(numpy.array([[0.0, 2.5], [1, 0], [0, 0]]))
    assert "not integers" in limit_reason(3, 2, 2, sparse)
    assert "type" in limit_reason(3, 2, 2, numpy.array([["a", "b"]] * 3))


def _minimum_workspace(n):
    return (8 * n + (4 * n + 7) // 8 * 8
            + min(n, 128) * 4 * ((n + 15) // 16 * 16))


def test_entries_refuse_bad_arguments_without_a_gpu():
    """-1 and a message naming the limit; every pointer and size is checked
    before anything is launched."""
    from scvae_amd import _lib
    lib = _lib.load()
    buffer = (ctypes.c_double * 64)()
    address = ctypes.addressof(buffer)
    address += -address % 16
    p = ctypes.c_void_p(address)
    big = 1 << 40

    def samples(n, f, k, x=p, offsets=p, score=p, workspace=p, nbytes=big,
                ldx=None):
        return lib.scvae_count_silhouette_samples_u16(
            x, (f + 63) // 64 * 64 if ldx is None else ldx, n, f, offsets, k,
            None, None, None, score, workspace, nbytes, None)

    def distances(n, f, i0=0, rows=1, x=p, d=p, ldd=None, workspace=p,
                  nbytes=big, ldx=None):
        return lib.scvae_count_distances_u16(
            x, (f + 63) // 64 * 64 if ldx is None else ldx, n, f, i0, rows,
            d, n if ldd is None else ldd, workspace, nbytes, None)

    def refused(code, limit):
        assert code == -1
        message = lib.scvae_last_error().decode()
        assert "bad argument" in message and limit in message, message
    for sizes, limit in (((1000, 65537, 20), "F <="), ((1000, 0, 20), "F >= 1"),
                         ((1000, 4, 1), "K >= 2"), ((1000, 4, 1000), "K <= N"),
                         ((2, 4, 2), "N >= 3"), ((2 ** 20 + 1, 4, 2), "N <=")):
        refused(samples(*sizes), limit)
    for sizes, limit in (((1000, 65537), "F <="), ((1000, 0), "F >= 1"),
                         ((2, 4), "N >= 3"), ((2 ** 20 + 1, 4), "N <=")):
        refused(distances(*sizes), limit)
    for name in ("x", "offsets", "score", "workspace"):
        refused(samples(100, 4, 3, **{name: None}), name)
    for name in ("x", "d", "workspace"):
        refused(distances(100, 4, **{name: None}), name)
    # a short workspace
    refused(samples(100, 4, 3, nbytes=_minimum_workspace(100) - 1),
            "workspace_bytes")
    refused(samples(1000, 4, 3, nbytes=_minimum_workspace(1000) - 1),
            "workspace_bytes")
    refused(distances(100, 4, nbytes=799), "workspace_bytes")
    # a workspace or rows off their alignment
    odd = ctypes.c_void_p(address + 4)
    refused(samples(100, 4, 3, workspace=odd), "workspace")
    refused(distances(100, 4, workspace=odd), "workspace")
    refused(samples(100, 4, 3, x=ctypes.c_void_p(address + 8)), "x")
    # the pitch: a multiple of 8, at least F rounded up to 64
    for f, ldx in ((4, 4), (4, 56), (4, 68), (65, 64), (65, 120)):
        refused(samples(100, f, 3, ldx=ldx), "ldx")
        refused(distances(100, f, ldx=ldx), "ldx")
    # the strip: inside the rows, the pitch of d at least N
    refused(distances(100, 4, i0=-1), "i0")
    refused(distances(100, 4, i0=0, rows=0), "rows")
    refused(distances(100, 4, i0=60, rows=41), "rows")
    refused(distances(100, 4, ldd=99), "ldd")


def test_score_is_nan_outside_the_cluster_counts_without_a_gpu(monkeypatch):
    """Fewer than 2 or more than N - 1 distinct labels: the reference's rule
    (clustering.py:125-127), answered before anything touches the device."""
    from scvae_amd.analyses import count_silhouette, prediction

    def never(*arguments, **keyword_arguments):
        raise AssertionError("the device path was entered")
    monkeypatch.setattr(count_silhouette, "_run", never)
    monkeypatch.setattr(count_silhouette, "_device_call", never)
    monkeypatch.setattr(count_silhouette._lib, "load", never)
    monkeypatch.setattr(count_silhouette.torch.cuda, "is_available", never)
    values = numpy.arange(20, dtype=numpy.uint16).reshape(10, 2)
    for function in (count_silhouette.count_silhouette_score,
                     prediction.count_silhouette_metric):
        assert math.isnan(function(values, [4] * 10))
        assert math.isnan(function(values, numpy.arange(10)))
        assert math.isnan(function(scipy.sparse.csr_matrix(values),
                                   list("abcdefghij")))
    assert math.isnan(count_silhouette.count_silhouette_score(
        values, [4] * 10, sample_size=5, random_state=0))


def test_device_count_silhouette_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib, analyses
    values = numpy.arange(20, dtype=numpy.uint16).reshape(10, 2)
    labels = [0, 1] * 5
    for function in (analyses.count_silhouette_samples,
                     analyses.count_silhouette_score):
        with pytest.raises(_lib.HipLibraryError, match="no CPU path") as info:
            function(values, labels)
        assert "No GPU visible" in str(info.value)
        assert "count-space silhouette" in str(info.value)


def test_wrapper_checks_its_input_before_the_device(monkeypatch):
    from scvae_amd.analyses import count_silhouette

    def never(*arguments, **keyword_arguments):
        raise AssertionError("the device path was entered")
    monkeypatch.setattr(count_silhouette, "_device_call", never)
    monkeypatch.setattr(count_silhouette.torch.cuda, "is_available",
                        lambda: True)
    monkeypatch.setattr(count_silhouette.torch.cuda, "mem_get_info",
                        lambda device=None: (1 << 30, 1 << 30))
    values = numpy.zeros((10, 2), dtype=numpy.uint16)
    with pytest.raises(ValueError, match="9 labels for 10 rows"):
        count_silhouette.count_silhouette_samples(values, [0, 1, 0] * 3)
    with pytest.raises(ValueError, match="matrix"):
        count_silhouette.count_silhouette_samples(numpy.zeros(10), [0, 1] * 5)
    with pytest.raises(ValueError, match="not integers"):
        count_silhouette.count_silhouette_samples(values + 0.25, [0, 1] * 5)
    with pytest.raises(ValueError, match="1 clusters for 10 cells"):
        count_silhouette.count_silhouette_samples(values, [3] * 10)
    # the uint16 rows against a quarter of the free memory
    wide = scipy.sparse.csr_matrix((40000, 32738), dtype=numpy.float32)
    with pytest.raises(ValueError, match="quarter of the free device memory"):
        count_silhouette.count_silhouette_samples(wide, numpy.arange(40000) % 3)


class _Set:
    kind = "test"
    has_labels = False
    number_of_examples = 12
    excluded_classes = ()

    def __init__(self, values):
        self.values = values
        self.updates = []

    def update_predictions(self, **keyword_arguments):
        self.updates.append(keyword_arguments)


def test_silhouette_space_switch_reaches_evaluate_and_predict(monkeypatch,
                                                              capsys):
    from scvae_amd import cli
    from scvae_amd.analyses import (
        count_silhouette, prediction, silhouette)

    # the flag parses and is handed to evaluate()
    seen = []
    monkeypatch.setattr(cli, "evaluate", lambda **kw: seen.append(kw) or 0)
    base = ["evaluate", "some_data", "-P", "k-means"]
    cli.main(base + ["--silhouette-score", "--silhouette-space", "counts"])
    cli.main(base + ["--silhouette-score", "--silhouette-space", "latent"])
    cli.main(base + ["--silhouette-score"])
    cli.main(base)
    assert [kw["silhouette_space"] for kw in seen] == [
        "counts", "latent", "latent", "latent"]
    assert [kw["silhouette_score"] for kw in seen] == [
        True, True, True, False]
    with pytest.raises(SystemExit):
        cli.main(base + ["--silhouette-space", "genes"])
    capsys.readouterr()

    cluster_ids = numpy.array([0, 1, 2] * 4, dtype=numpy.int32)

    def predict(training_set, evaluation_set, specifications=None,
                on_device=False, **rest):
        return cluster_ids, predict.labels, None
    monkeypatch.setattr(prediction, "predict_labels", predict)
    calls, latent_calls = [], []

    def count_score(values, labels, sample_size=None, random_state=None,
                    device=None):
        calls.append((values, numpy.asarray(labels), sample_size))
        return 0.25 if len(calls) % 2 else -0.125
    monkeypatch.setattr(count_silhouette, "count_silhouette_score",
                        count_score)
    monkeypatch.setattr(count_silhouette, "limit_reason",
                        lambda *arguments, **keywords: None)
    monkeypatch.setattr(
        silhouette, "silhouette_score",
        lambda values, labels, device=None: latent_calls.append(1) or 0.5)
    rng = numpy.random.default_rng(3)

    class Model:
        def evaluate(self, **keyword_arguments):
            return {"z": _Set(rng.standard_normal((12, 2)))}
    specifications = prediction.PredictionSpecifications(
        "k-means", number_of_clusters=3, training_set_kind="training")

    def run(labelled, cells=12, **switch):
        counts = scipy.sparse.csr_matrix(
            rng.poisson(1.0, size=(cells, 5)).astype(numpy.float32))
        sets = [_Set(counts), _Set(counts.copy()),
                _Set(rng.standard_normal((cells, 2)))]
        if labelled:
            names = numpy.array(["p", "q", "q"] * 4)
            for s in sets:
                s.has_labels, s.labels = True, names
            predict.labels = numpy.array(["p", "q", "p"] * 4)
        else:
            predict.labels = None
        del calls[:], latent_calls[:]
        capsys.readouterr()
        cli._predict(Model(), [sets[0], sets[1], {"z": sets[2]}],
                     _Set(None), specifications, 4, None, False, False,
                     "end_of_training", **switch)
        return sets[0], capsys.readouterr().out.splitlines()

    counts_on = {"silhouette_score": True, "silhouette_space": "counts"}
    transformed, lines = run(False, **counts_on)
    assert len(calls) == 1 and not latent_calls
    assert calls[0][0] is transformed.values and calls[0][2] is None
    assert numpy.array_equal(calls[0][1], cluster_ids)
    at = lines.index("Clustering of the test set (kmeans_3):")
    assert lines[at + 1] == (
        "    silhouette score (clusters; count space): 0.2500")
    assert not any("(labels" in line for line in lines)
    assert not any("sampled" in line for line in lines)

    transformed, lines = run(True, **counts_on)
    assert len(calls) == 2 and not latent_calls
    assert numpy.array_equal(calls[1][1], predict.labels)
    assert lines.count("Clustering of the test set (kmeans_3):") == 1
    at = lines.index("    silhouette score (clusters; count space): 0.2500")
    assert lines[at - 1].startswith("    accuracy:")
    assert lines[at + 1] == (
        "    silhouette score (labels; count space): -0.1250")

    # the default space: the latent lines, byte for byte, and no count call
    for switch in ({"silhouette_score": True},
                   {"silhouette_score": True, "silhouette_space": "latent"}):
        _, lines = run(True, **switch)
        assert not calls and len(latent_calls) == 2
        assert "    silhouette score (clusters): 0.5000" in lines
        assert "    silhouette score (labels): 0.5000" in lines
        assert not any("count space" in line for line in lines)
    # the space alone asks for nothing
    for switch in ({}, {"silhouette_space": "counts"},
                   {"silhouette_score": False, "silhouette_space": "counts"}):
        _, lines = run(True, **switch)
        assert not calls and not latent_calls
        assert not any("silhouette" in line for line in lines)


def test_sampled_line_comes_before_the_scores(monkeypatch, capsys):
    """More than 20 000 cells: ``(count space: 20000 of N cells sampled)``,
    then the lines, and the device call gets ``sample_size=20000``."""
    from scvae_amd import cli
    from scvae_amd.analyses import count_silhouette, prediction
    cells = 20001
    cluster_ids = numpy.arange(cells) % 3
    monkeypatch.setattr(
        prediction, "predict_labels",
        lambda **keyword_arguments: (cluster_ids, None, None))
    calls = []

    def count_score(values, labels, sample_size=None, random_state=None,
                    device=None):
        calls.append(sample_size)
        return 0.5
    monkeypatch.setattr(count_silhouette, "count_silhouette_score",
                        count_score)
    monkeypatch.setattr(count_silhouette, "limit_reason",
                        lambda *arguments, **keywords: None)

    class Model:
        def evaluate(self, **keyword_arguments):
            return {"z": _Set(numpy.zeros((cells, 2)))}
    counts = scipy.sparse.csr_matrix((cells, 5), dtype=numpy.float32)
    specifications = prediction.PredictionSpecifications(
        "k-means", number_of_clusters=3, training_set_kind="training")
    cli._predict(Model(), [_Set(counts), _Set(counts),
                           {"z": _Set(numpy.zeros((cells, 2)))}],
                 _Set(None), specifications, 4, None, False, False,
                 "end_of_training", silhouette_score=True,
                 silhouette_space="counts")
    lines = capsys.readouterr().out.splitlines()
    at = lines.index("    (count space: 20000 of 20001 cells sampled)")
    assert lines[at + 1] == (
        "    silhouette score (clusters; count space): 0.5000")
    assert lines[at - 1] == "Clustering of the test set (kmeans_3):"
    assert calls == [20000]


def test_metric_falls_back_to_scikit_learn_outside_the_limits(monkeypatch,
                                                              capsys):
    """Values that are no integers: one line saying why, then what the
    reference computes; inside the limits the device call."""
    metrics = pytest.importorskip("sklearn.metrics")
    from scvae_amd.analyses import count_silhouette, prediction
    calls = []

    def score(values, labels, sample_size=None, random_state=None,
              device=None):
        calls.append((values.shape, sample_size, random_state))
        return 0.5
    monkeypatch.setattr(count_silhouette, "count_silhouette_score", score)
    monkeypatch.setattr(count_silhouette.torch.cuda, "is_available",
                        lambda: False)
    rng = numpy.random.default_rng(0)
    counts = rng.poisson(2.0, size=(80, 30)).astype(numpy.float32)
    labels = rng.integers(4, size=80)
    scaled = counts / 3
    got = prediction.count_silhouette_metric(scaled, labels)
    assert capsys.readouterr().out == (
        "count-space silhouette score on the device not used: values that "
        "are not integers (integer counts supported).\n")
    assert not calls
    assert got == pytest.approx(
        float(metrics.silhouette_score(scaled, labels)), abs=1e-12)
    for values in (counts, scipy.sparse.csr_matrix(counts)):
        assert prediction.count_silhouette_metric(
            values, labels, random_state=5) == 0.5
    assert calls == [((80, 30), None, 5)] * 2
    assert capsys.readouterr().out == ""
    # above 20 000 cells both paths sample 20 000, as the reference does
    seen = {}

    def sampled(X, labels, sample_size=None, random_state=None):
        seen["sample_size"] = sample_size
        return 0.0
    monkeypatch.setattr(metrics, "silhouette_score", sampled)
    many = numpy.arange(20001) % 3
    prediction.count_silhouette_metric(numpy.full((20001, 3), 0.5), many)
    assert seen["sample_size"] == 20000
    assert "not integers" in capsys.readouterr().out
    prediction.count_silhouette_metric(numpy.full((20000, 3), 0.5), many[1:])
    assert seen["sample_size"] is None
    del calls[:]
    prediction.count_silhouette_metric(
        numpy.ones((20001, 3), dtype=numpy.uint16), many)
    prediction.count_silhouette_metric(
        numpy.ones((20000, 3), dtype=numpy.uint16), many[1:])
    assert calls == [((20001, 3), 20000, None), ((20000, 3), None, None)]
