"""What of the t-SNE of the latent space runs without a GPU: the fp64 oracle
(``_tsne_oracle.py``) against scikit-learn's own functions, the limits, the
lines ``decompose_latent`` prints, the command line and the C ABI entries."""
import os
import re

import numpy
import pytest

import _tsne_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_follows_scikit_learn():
    """``_joint_probabilities`` and ``_kl_divergence`` of scikit-learn take
    the fp32 squared distances and work in fp64, as the oracle does from the
    same distances: the two differ by the order of fp64 sums only.  A sum of
    n = 40 terms carries at most n u relative (u = 2^-53); P passes through
    two such sums (the row sum and sumP) and a handful of operations, the KL
    divergence and the gradient through one more over n^2 terms: 1e-12
    relative is three orders above all of that and six below the fp32 level
    that the device is held to."""
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    rng = numpy.random.default_rng(5)
    n = 40
    x = rng.standard_normal((n, 5)).astype(numpy.float32)
    d2 = oracle.squared_distances(x).astype(numpy.float32)
    want_P = squareform(t_sne._joint_probabilities(d2, 12.0, 0))
    beta, sums, steps = oracle.perplexity_search(
        d2.astype(numpy.float64), 12.0)
    assert numpy.all(steps < oracle.SEARCH_STEPS)
    P = oracle.joint_probabilities(d2.astype(numpy.float64), beta, sums)
    assert numpy.all(numpy.abs(P - want_P) <= 1e-12 * want_P)
    assert abs(P.sum() - 1.0) <= 1e-12
    # every row has the perplexity asked for
    for i in range(n):
        H, S, raw = oracle.row_entropy(d2[i], i, beta[i])
        assert abs(H - numpy.log(12.0)) <= oracle.SEARCH_TOLERANCE
        assert S == raw == sums[i]
    y = rng.standard_normal((n, 2)) * 3.0
    for exaggeration in (1.0, 12.0):
        want_kl, want_grad = t_sne._kl_divergence(
            y.ravel(), squareform(P * exaggeration, checks=False), 1.0, n, 2)
        kl, grad, Z = oracle.kl_divergence_and_gradient(P, y, exaggeration)
        assert abs(kl - want_kl) <= 1e-12 * abs(want_kl)
        scale = numpy.abs(want_grad).max()
        assert numpy.all(
            numpy.abs(grad.ravel() - want_grad) <= 1e-12 * scale)
        assert Z > 0


def test_oracle_update_follows_scikit_learn():
    """Two stages of three iterations through scikit-learn's
    ``_gradient_descent`` and through the oracle's loop: the same embedding
    to fp64 rounding (six updates of sums over 30 terms: 1e-11 relative to
    the largest coordinate is far above it).  The learning rate is 1: with
    the automatic one, 50 for so few rows, every early iteration multiplies
    the embedding -- and any rounding difference -- by about 80."""
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    rng = numpy.random.default_rng(6)
    n = 30
    x = rng.standard_normal((n, 4)).astype(numpy.float32)
    y0 = rng.standard_normal((n, 2)) * 1e-4
    trace = []
    got = oracle.fit(x, y0, perplexity=8.0, max_iter=6, learning_rate=1.0,
                     exploration_iterations=3, trace=trace)
    assert len(trace) == 6 and got["n_iter"] == 5
    assert [t["momentum"] for t in trace] == [0.5] * 3 + [0.8] * 3
    assert [t["exaggeration"] for t in trace] == [12.0] * 3 + [1.0] * 3
    P = squareform(got["P"], checks=False)
    arguments = dict(n_iter_check=50, min_grad_norm=1e-7,
                     learning_rate=got["learning_rate"], verbose=0)
    p, _, it = t_sne._gradient_descent(
        t_sne._kl_divergence, y0.ravel().copy(), it=0, max_iter=3,
        momentum=0.5, n_iter_without_progress=3, args=[P * 12.0, 1.0, n, 2],
        **arguments)
    p, _, it = t_sne._gradient_descent(
        t_sne._kl_divergence, p, it=it + 1, max_iter=6, momentum=0.8,
        n_iter_without_progress=300, args=[P, 1.0, n, 2], **arguments)
    assert it == got["n_iter"]
    want = p.reshape(n, 2)
    assert numpy.all(numpy.abs(got["embedding"] - want)
                     <= 1e-11 * numpy.abs(want).max())


def test_initial_embedding_is_the_scaled_pca():
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    from scvae_amd.analyses import tsne
    rng = numpy.random.default_rng(7)
    values = (rng.standard_normal((50, 6)) * numpy.arange(1, 7) + 3.0)
    centred = tsne.centre(values)
    assert centred.dtype == numpy.float32 and centred.shape == (50, 6)
    assert numpy.all(numpy.abs(
        centred - (values - values.mean(axis=0))) <= 2.0 ** -24 * 30)
    y0 = tsne.initial_embedding(centred)
    want = PCA(n_components=2, svd_solver="full").fit_transform(
        centred.astype(numpy.float64))
    want = want / want[:, 0].std() * 1e-4
    assert y0.shape == (50, 2) and y0.dtype == numpy.float64
    assert numpy.allclose(y0, want, rtol=0, atol=1e-12)
    assert abs(y0[:, 0].std() - 1e-4) <= 1e-18
    with pytest.raises(ValueError, match="variance"):
        tsne.initial_embedding(numpy.ones((5, 3)))


def test_limit_reason():
    from scvae_amd.analyses.tsne import limit_reason
    assert limit_reason(4, 1, 3.0) is None
    assert limit_reason(200000, 100, 30.0) is None
    assert limit_reason(68579, 25, 30.0) is None
    assert "examples" in limit_reason(3, 25, 2.0)
    assert "examples" in limit_reason(200001, 25, 30.0)
    assert "features" in limit_reason(1000, 101, 30.0)
    assert "features" in limit_reason(1000, 0, 30.0)
    assert "perplexity" in limit_reason(30, 25, 30.0)
    assert "perplexity" in limit_reason(30, 25, 0.0)
    assert limit_reason(31, 25, 30.0) is None
    assert "components" in limit_reason(1000, 25, 30.0, 3)


def test_argument_checks():
    from scvae_amd.analyses.tsne import DeviceTSNE
    for arguments in ({"perplexity": 0.0}, {"early_exaggeration": 0.5},
                      {"learning_rate": -1.0},
                      {"max_iter": 10, "exploration_iterations": 20}):
        with pytest.raises(ValueError):
            DeviceTSNE(**arguments)
    model = DeviceTSNE()
    assert (model.perplexity, model.early_exaggeration, model.max_iter,
            model.exploration_iterations, model.n_iter_without_progress,
            model.min_grad_norm, model.learning_rate) == (
                30.0, 12.0, 1000, 250, 300, 1e-7, "auto")


def test_device_tsne_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib
    from scvae_amd.analyses import DeviceTSNE
    x = numpy.random.default_rng(0).standard_normal((40, 5))
    with pytest.raises(_lib.HipLibraryError, match="no CPU path"):
        DeviceTSNE().fit_transform(x)


class _FakeTSNE:
    fitted = []

    def fit_transform(self, values):
        _FakeTSNE.fitted.append(numpy.array(values))
        self.kl_divergence_, self.n_iter_ = 0.5, 999
        return numpy.asarray(values)[:, :2] * 2.0


def test_decompose_latent_lines(monkeypatch, capsys):
    pytest.importorskip("sklearn")
    from scvae_amd.analyses import tsne
    rng = numpy.random.default_rng(8)
    monkeypatch.setattr(tsne, "DeviceTSNE", _FakeTSNE)
    _FakeTSNE.fitted.clear()
    # too many examples: the reference's line, nothing fitted
    monkeypatch.setattr(tsne, "MAXIMUM_NUMBER_OF_EXAMPLES_FOR_TSNE", 59)
    values = rng.standard_normal((60, 5))
    assert tsne.decompose_latent(
        values, "t-SNE", "latent space for z set") is None
    assert capsys.readouterr().out == (
        "The number of examples for latent space for z set is too large to "
        "decompose it using t-SNE. Skipping.\n\n")
    assert not _FakeTSNE.fitted
    monkeypatch.undo()
    monkeypatch.setattr(tsne, "DeviceTSNE", _FakeTSNE)
    # inside the limits
    fit = tsne.decompose_latent(values, "tsne", "latent space for z set")
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Decomposing latent space for z set using t-SNE."
    assert re.fullmatch(r"Latent space for z set decomposed \(.+\)\.",
                        lines[1]) and len(lines) == 2
    assert numpy.array_equal(fit["coordinates"], values[:, :2] * 2.0)
    assert isinstance(fit["model"], _FakeTSNE) and fit["duration"] >= 0
    assert len(_FakeTSNE.fitted) == 1
    # too many features: two lines, PCA to min(50, N - 1) components first
    for rows, components in ((60, 50), (31, 30)):
        wide = rng.standard_normal((rows, 101))
        fit = tsne.decompose_latent(wide, "t-SNE", "latent space for z set")
        lines = capsys.readouterr().out.splitlines()
        assert lines[0] == (
            "The number of features for latent space for z set is too large "
            "to decompose it using t-SNE in due time.")
        assert lines[1] == (
            "Decomposing latent space for z set to {} components using PCA "
            "beforehand.".format(components))
        assert re.fullmatch(
            r"Latent space for z set pre-decomposed \(.+\)\.", lines[2])
        assert lines[3] == "Decomposing latent space for z set using t-SNE."
        assert lines[4].startswith("Latent space for z set decomposed (")
        reduced = _FakeTSNE.fitted[-1]
        assert reduced.shape == (rows, components)
        from sklearn.decomposition import PCA
        assert numpy.allclose(
            reduced, PCA(n_components=components).fit_transform(wide),
            rtol=0, atol=1e-9)
        assert fit["coordinates"].shape == (rows, 2)
    # PCA of a latent set: the existing decompose
    fit = tsne.decompose_latent(values, "pca", "latent space for z set")
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Decomposing latent space for z set using PCA."
    assert lines[1].startswith("Latent space for z set decomposed (")
    from scvae_amd.analyses import decompose
    assert numpy.array_equal(fit["coordinates"], decompose(values)[0])
    assert fit["model"] is None


def test_outside_the_limits_scikit_learn_takes_over(monkeypatch, capsys):
    manifold = pytest.importorskip("sklearn.manifold")
    from scvae_amd.analyses import tsne
    seen = []

    class Recorder:
        def __init__(self, **arguments):
            seen.append(arguments)

        def fit_transform(self, values):
            return numpy.zeros((len(values), 2))

    monkeypatch.setattr(manifold, "TSNE", Recorder)
    monkeypatch.setattr(tsne, "DeviceTSNE", None)
    values = numpy.random.default_rng(9).standard_normal((20, 5))
    fit = tsne.decompose_latent(values, "t-SNE", "latent space for z set")
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Decomposing latent space for z set using t-SNE."
    assert lines[1] == (
        "t-SNE on the device not used: a perplexity of 30 for 20 examples "
        "(it must be below their number).")
    assert seen == [{"n_components": 2, "random_state": 42}]
    assert fit["coordinates"].shape == (20, 2)


def test_flag_parses_and_reaches_evaluate(monkeypatch, capsys):
    import inspect
    from scvae_amd import cli
    assert inspect.signature(cli.evaluate).parameters[
        "latent_space"].default is False
    seen = []
    monkeypatch.setattr(cli, "evaluate", lambda **kw: seen.append(kw) or 0)
    cli.main(["evaluate", "some_data"])
    cli.main(["evaluate", "some_data", "--latent-space",
              "--decomposition-methods", "pca", "t-SNE"])
    assert [kw["latent_space"] for kw in seen] == [False, True]
    assert seen[1]["decomposition_methods"] == ["pca", "t-SNE"]
    assert seen[1]["decompositions"] is False
    with pytest.raises(SystemExit):
        cli.main(["evaluate", "--help"])
    assert "--latent-space" in capsys.readouterr().out


class _Set:
    def __init__(self, version, values, labels=None):
        self.version, self.values = version, values
        self.kind = "test"
        self.example_names = numpy.array(
            ["c{}".format(i) for i in range(len(values))])
        self.has_labels = labels is not None
        self.labels = labels


def test_report_lines_and_files(tmp_path, monkeypatch, capsys):
    pytest.importorskip("sklearn")
    from scvae_amd import cli
    from scvae_amd.analyses import tsne
    monkeypatch.setattr(tsne, "DeviceTSNE", _FakeTSNE)
    rng = numpy.random.default_rng(10)
    z = rng.standard_normal((40, 3))
    labels = numpy.array(["a", "b"] * 20)
    sets = {"z": _Set("z", z, labels),
            "y": _Set("y", rng.standard_normal((40, 2)))}
    cli._report_latent_space(sets, ["PCA", "ICA", "t-SNE"], str(tmp_path))
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Decomposition method `ICA` is not built: skipped."
    assert lines[1] == "Decomposing latent space for z set using PCA."
    assert lines[2].startswith("Latent space for z set decomposed (")
    assert lines[3] == ""
    assert lines[4] == "Decomposing latent space for z set using t-SNE."
    assert lines[5].startswith("Latent space for z set decomposed (")
    assert lines[6] == "    KL divergence: 0.5; 1000 iterations."
    assert lines[7:] == [""]
    # the set with two features is left out, as in the reference
    assert sorted(p.name for p in tmp_path.iterdir()) == ["latent_space-z"]
    rows = (tmp_path / "latent_space-z" / "t_sne.tsv").read_text().splitlines()
    assert rows[0] == "example\ttSNE 1\ttSNE 2\tlabel" and len(rows) == 41
    assert rows[2] == "c1\t{!r}\t{!r}\tb".format(
        float(z[1, 0] * 2.0), float(z[1, 1] * 2.0))
    rows = (tmp_path / "latent_space-z" / "pca.tsv").read_text().splitlines()
    assert rows[0] == "example\tPC 1\tPC 2\tlabel" and len(rows) == 41


def test_header_and_bindings():
    from scvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "scvae_hip.h")).read()
    for name, arguments in (("scvae_tsne_workspace_bytes", 2),
                            ("scvae_tsne_perplexity", 11),
                            ("scvae_tsne_gradient", 15),
                            ("scvae_tsne_update", 9)):
        assert re.search(r"\b{}\(".format(name), header), name
        assert len(_lib.SIGNATURES[name][1]) == arguments
    assert "subanalyses.py:595-673" in header
    lib = _lib.load()
    assert lib.scvae_tsne_workspace_bytes(1, 25) == -1
    assert b"bad argument" in lib.scvae_last_error()
    assert lib.scvae_tsne_workspace_bytes(64, 129) == -1
    size = lib.scvae_tsne_workspace_bytes(68579, 25)
    assert size >= 8 * 68579 + 4 * 512 * 68579 and size % 8 == 0
    assert lib.scvae_tsne_workspace_bytes(200000, 100) > size
    assert lib.scvae_tsne_perplexity(None, 25, 64, 25, 30.0, None, None, None,
                                     None, 0, None) == -1
    assert lib.scvae_tsne_gradient(None, 25, 64, 25, None, None, 128.0, None,
                                   1.0, None, None, None, None, 0, None) == -1
    assert lib.scvae_tsne_update(None, None, None, None, 64, 0.5, 200.0, 0.01,
                                 None) == -1
