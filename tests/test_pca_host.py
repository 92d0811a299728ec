"""What the PCA needs no GPU for: the subspace-iteration loop on the NumPy
operator against the SVD oracle, the sign rule, the argument checks, the
command-line flags, and the refusal to run without a GPU."""
import numpy
import pytest

from _pca_oracle import (
    MAXIMUM_ITERATIONS, SETS, Oracle, count_like, flip, gamma)


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("n,f,seed", SETS)
def test_loop_on_the_numpy_operator(n, f, seed, block):
    from scvae_amd.analyses.decomposition import DevicePCA, NumpyOperator
    x = count_like(n, f, seed)
    reference = Oracle(x) if block == 8 else _oracle(n, f, seed)
    reference.assert_separated()
    assert 0.6 < (x == 0).mean() < 0.85 and 50 <= x.max() <= 400
    model = DevicePCA(block_size=block, tolerance=1e-10,
                      operator=NumpyOperator)
    coordinates = model.fit_transform(x)
    print("{} iterations, residuals {}".format(
        model.n_iterations_, model.residuals_))
    assert model.converged_ and model.n_iterations_ <= MAXIMUM_ITERATIONS
    eigenvalues = model.singular_values_ ** 2
    for k in range(2):
        residual = float(model.residuals_[k])
        assert residual <= 1e-10
        assert abs(eigenvalues[k] - reference.eigenvalues[k]) <= (
            reference.eigenvalue_bound(k, residual))
        difference = numpy.linalg.norm(
            model.components_[k] - reference.components[k])
        assert difference <= reference.vector_bound(k, residual)
        want = reference.centred @ reference.components[k]
        bound = (numpy.linalg.norm(reference.centred, axis=1) * difference
                 + 2 * gamma(f + 2) * (numpy.abs(reference.centred)
                                       @ numpy.abs(model.components_[k])))
        assert numpy.all(numpy.abs(coordinates[:, k] - want) <= bound)
        assert abs(model.explained_variance_ratio_[k]
                   - reference.eigenvalues[k] / reference.total) <= (
            reference.eigenvalue_bound(k, residual) / reference.total
            + 4 * gamma(n * f))
    assert numpy.array_equal(model.explained_variance_,
                             eigenvalues / (n - 1)) or numpy.allclose(
        model.explained_variance_, eigenvalues / (n - 1), rtol=1e-15)
    assert numpy.array_equal(model.transform(x[:7]), coordinates[:7]) or (
        numpy.allclose(model.transform(x[:7]), coordinates[:7], rtol=0,
                       atol=1e-9))


_CACHE = {}


def _oracle(n, f, seed):
    if (n, f, seed) not in _CACHE:
        _CACHE[n, f, seed] = Oracle(count_like(n, f, seed))
    return _CACHE[n, f, seed]


def test_block_shrinks_and_degenerate_fits():
    from scvae_amd.analyses.decomposition import (
        DevicePCA, NumpyOperator, subspace_iteration)
    x = count_like(20, 2003, 6)
    result = subspace_iteration(NumpyOperator(x), block_size=32)
    assert result["block"] == 19 and result["converged"]
    assert result["iterations"] <= 2
    with pytest.raises(ValueError, match="no variance"):
        DevicePCA(operator=NumpyOperator).fit(
            numpy.full((5, 9), 3.0, dtype=numpy.float32))
    with pytest.raises(ValueError, match="at least as many"):
        DevicePCA(operator=NumpyOperator).fit(
            numpy.arange(12, dtype=numpy.float32).reshape(2, 6))
    rng = numpy.random.default_rng(0)
    noise = rng.standard_normal((60, 300)).astype(numpy.float32)
    model = DevicePCA(maximum_iterations=2, operator=NumpyOperator)
    model.fit(noise)
    assert model.converged_ is False and model.n_iterations_ == 2
    assert numpy.all(numpy.isfinite(model.components_))


def test_sign_rule_on_ties():
    from scvae_amd.analyses.decomposition import flip_signs
    components = numpy.array([[0.5, -0.5, 0.1], [-0.5, 0.5, 0.1],
                              [0.1, -0.7, 0.7], [0.0, 0.0, 0.0]])
    signs = flip_signs(components)
    assert list(signs) == [1.0, -1.0, -1.0, 1.0]
    flipped = components * signs[:, None]
    assert numpy.array_equal(flipped[:3], flip(components)[:3])
    for row in flipped[:3]:
        assert row[numpy.argmax(numpy.abs(row))] > 0
    svd_flip = pytest.importorskip("sklearn.utils.extmath").svd_flip
    u = numpy.zeros((4, 3))
    _, want = svd_flip(u, components[:3].copy(), u_based_decision=False)
    assert numpy.array_equal(flipped[:3], want)


def test_argument_checks():
    from scvae_amd.analyses import decomposition
    from scvae_amd.analyses.decomposition import DevicePCA, limit_reason
    for arguments in ({"n_components": 0}, {"block_size": 1},
                      {"block_size": 33}, {"tolerance": -1.0},
                      {"tolerance": float("nan")},
                      {"maximum_iterations": 0}):
        with pytest.raises(ValueError):
            DevicePCA(**arguments)
    assert limit_reason(100, 3000) is None
    assert limit_reason(2 ** 31 - 1, 2 ** 20, 2, 32) is None
    assert "features" in limit_reason(100, 2 ** 20 + 1)
    assert "examples" in limit_reason(2 ** 31, 3000)
    assert "examples" in limit_reason(1, 3000)
    assert "components" in limit_reason(100, 3000, 33, 33)
    assert "block" in limit_reason(100, 3000, 2, 40)
    assert "components from" in limit_reason(2, 3000, 2, 16)
    assert decomposition.method_name("t_sne") == "t-SNE"
    assert decomposition.method_name("pca") == "PCA"
    x = numpy.ones((4, 3), dtype=numpy.float32)
    for method in ("svd", "ica", "tsne"):
        with pytest.raises(NotImplementedError, match=r"decomposition\.py"):
            decomposition.decompose(x, method=method)
    with pytest.raises(ValueError, match="not found"):
        decomposition.decompose(x, method="umap")
    with pytest.raises(RuntimeError, match="not been fitted"):
        DevicePCA().transform(x)


def test_decompose_on_the_host_follows_scikit_learn():
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    from scvae_amd.analyses import decompose
    x = numpy.array(count_like(300, 2101, 1)[:, :50])
    other = numpy.array(count_like(130, 2050, 2)[:9, :50])
    output = decompose(x, other_value_sets={"other": other, "none": None})
    model = PCA(n_components=2)
    assert len(output) == 2
    assert numpy.array_equal(output[0], model.fit_transform(x))
    assert numpy.array_equal(output[1]["other"], model.transform(other))
    assert output[1]["none"] is None
    output = decompose(x, centroids={"means": x[:3].astype("f8")})
    assert len(output) == 2 and output[1]["means"].shape == (3, 2)
    assert numpy.allclose(output[1]["means"], model.transform(x[:3]),
                          rtol=0, atol=1e-4)


def test_device_pca_refuses_to_run_without_gpu():
    import scipy.sparse
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib, analyses
    x = numpy.array(count_like(64, 4099, 4))
    for call in (lambda: analyses.DevicePCA().fit(x),
                 lambda: analyses.DevicePCA().fit_transform(
                     scipy.sparse.csr_matrix(x)),
                 lambda: analyses.decompose(x),
                 lambda: analyses.decompose(scipy.sparse.csr_matrix(
                     x[:, :50]))):
        with pytest.raises(_lib.HipLibraryError, match="no CPU path") as info:
            call()
        assert "No GPU visible" in str(info.value)
        assert "decomposition" in str(info.value)


def test_evaluate_help_lists_the_flags(capsys):
    from scvae_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["evaluate", "--help"])
    out = capsys.readouterr().out
    assert "--decompositions" in out
    assert "--decomposition-methods METHOD [METHOD ...]" in out


def test_flags_parse_and_reach_evaluate(monkeypatch):
    from scvae_amd import cli
    seen = []
    monkeypatch.setattr(cli, "evaluate", lambda **kw: seen.append(kw) or 0)
    cli.main(["evaluate", "some_data"])
    cli.main(["evaluate", "some_data", "--decompositions"])
    cli.main(["evaluate", "some_data", "--decompositions",
              "--decomposition-methods", "pca", "tsne", "--analysis-level",
              "extensive", "--analyses-directory", "somewhere"])
    assert [kw["decompositions"] for kw in seen] == [False, True, True]
    assert [kw["decomposition_methods"] for kw in seen] == [
        "PCA", "PCA", ["pca", "tsne"]]
    assert [kw["analysis_level"] for kw in seen] == [
        "normal", "normal", "extensive"]
    assert [kw["analyses_directory"] for kw in seen] == [
        None, None, "somewhere"]
    with pytest.raises(SystemExit):   # there is no `analyse` command
        cli.main(["analyse", "some_data", "--decompositions"])


class _Set:
    kind = "test"
    name = "set"
    has_labels = True
    labels = numpy.array(["a", "b", "a"])
    example_names = numpy.array(["c1", "c2", "c3"])
    values = numpy.zeros((3, 4), dtype=numpy.float32)


def test_report_lines_and_files(tmp_path, capsys):
    from scvae_amd import cli
    reconstructed = _Set()
    cli._report_decompositions(reconstructed, ["PCA"], None, str(tmp_path))
    assert capsys.readouterr().out == "" and not list(tmp_path.iterdir())
    reconstructed.decomposition = {
        "coordinates": numpy.array([[1.5, -2.0], [0.25, 3.0], [0.0, 1e-9]]),
        "explained_variance_ratio": numpy.array([0.61234567, 0.2]),
        "iterations": 7, "converged": True, "duration": 0.25}
    cli._report_decompositions(reconstructed, ["PCA", "ICA"], None,
                               str(tmp_path))
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Decomposition method `ICA` is not built: skipped."
    assert lines[1] == "Decomposing reconstructions set using PCA."
    assert lines[2].startswith("Reconstructions set decomposed (")
    assert lines[3] == ("    Explained variance ratios: 0.61235, 0.2; "
                        "7 iterations.")
    assert lines[4:] == [""]
    rows = (tmp_path / "reconstructions" / "pca.tsv").read_text().splitlines()
    assert rows == ["example\tPC 1\tPC 2\tlabel", "c1\t1.5\t-2.0\ta",
                    "c2\t0.25\t3.0\tb", "c3\t0.0\t1e-09\ta"]
    reconstructed.decomposition["converged"] = False
    cli._report_decompositions(reconstructed, ["PCA"], None, str(tmp_path))
    assert "7 iterations (not converged)." in capsys.readouterr().out
