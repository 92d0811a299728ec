"""The PCA kernels (``csrc/pca.hip``) element by element against fp64 NumPy,
``DevicePCA`` against the SVD oracle on the five count-like sets, its other
behaviour, ``decompose``, and the decompositions of ``evaluate`` end to end.
Every bound is derived beside its assert."""
import ctypes
import functools
import re

import numpy
import pytest
import torch

from _pca_oracle import (
    MAXIMUM_ITERATIONS, SETS, Oracle, U, count_like, gamma)

pytestmark = pytest.mark.gpu

#: (rows, features, pitch): one row; odd sizes below a tile; a column slice
#: of a wider tensor (16-byte aligned rows); an odd pitch over several row
#: ranges and feature blocks
SHAPES = [(1, 5, 5), (17, 67, 67), (130, 2050, 2112), (333, 4099, 4099)]
BLOCKS = [2, 8, 16]


@functools.lru_cache(maxsize=None)
def kernel_case(rows, features):
    """Non-integer fp32 values, about 70 % zeros, some all-zero columns."""
    rng = numpy.random.default_rng(1000 * rows + features)
    x = (rng.poisson(3.0, (rows, features)) * rng.random((rows, features))
         * (rng.random((rows, features)) < 0.3)).astype(numpy.float32)
    x[:, ::7] = 0
    x.setflags(write=False)
    return x


def placed(x, pitch, device):
    """``x`` on the device as the columns 4 .. 4 + features of a
    [rows, pitch] tensor (pitch > features) or as it is."""
    rows, features = x.shape
    if pitch == features:
        return torch.from_numpy(numpy.array(x)).to(device)
    wide = torch.full((rows, pitch), float("nan"), dtype=torch.float32,
                      device=device)
    view = wide[:, 4:4 + features]
    view.copy_(torch.from_numpy(numpy.array(x)))
    assert view.stride(0) == pitch
    return view


def _p(tensor):
    return ctypes.c_void_p(tensor.data_ptr()) if tensor is not None else None


def device_moments(t):
    from scvae_amd import _lib
    lib = _lib.load()
    rows, features = t.shape
    pitch = t.stride(0) if rows > 1 else features
    mu = torch.empty(features, dtype=torch.float64, device=t.device)
    total = torch.empty(1, dtype=torch.float64, device=t.device)
    size = lib.scvae_pca_workspace_bytes(rows, features, 1)
    assert size > 0
    workspace = torch.empty(size, dtype=torch.uint8, device=t.device)
    _lib.check(lib.scvae_pca_moments(_p(t), pitch, rows, features, _p(mu),
                                     _p(total), _p(workspace), size, None))
    return mu, float(total.item())


def device_project(t, mu, q):
    from scvae_amd import _lib
    lib = _lib.load()
    rows, features = t.shape
    pitch = t.stride(0) if rows > 1 else features
    qd = torch.from_numpy(numpy.ascontiguousarray(q)).to(t.device)
    y = torch.full((rows, q.shape[1]), float("nan"), dtype=torch.float64,
                   device=t.device)
    _lib.check(lib.scvae_pca_project(_p(t), pitch, rows, features, _p(mu),
                                     _p(qd), q.shape[1], _p(y), None))
    return y


def device_back_project(t, mu, y):
    from scvae_amd import _lib
    lib = _lib.load()
    rows, features = t.shape
    pitch = t.stride(0) if rows > 1 else features
    block = y.shape[1]
    z = torch.full((features, block), float("nan"), dtype=torch.float64,
                   device=t.device)
    size = lib.scvae_pca_workspace_bytes(rows, features, block)
    workspace = torch.empty(size, dtype=torch.uint8, device=t.device)
    _lib.check(lib.scvae_pca_back_project(
        _p(t), pitch, rows, features, _p(mu), _p(y), block, _p(z),
        _p(workspace), size, None))
    return z


@pytest.mark.parametrize("rows,features,pitch", SHAPES)
def test_column_moments(rows, features, pitch, cuda_device):
    x = kernel_case(rows, features)
    t = placed(x, pitch, cuda_device)
    mu, total = device_moments(t)
    mu = mu.cpu().numpy()
    x64 = x.astype(numpy.float64)
    want = x64.mean(axis=0)
    # a sum of `rows` values in fp64, in any order, and one division, on
    # each side: |mu - want| <= 2 gamma_{rows+1} sum_i |x_ij| / rows
    mean_bound = 2 * gamma(rows + 1) * numpy.abs(x64).sum(axis=0) / rows
    error = numpy.abs(mu - want)
    print("mean: worst error {:.3g}, worst error / bound {:.3g}".format(
        error.max(), (error / numpy.maximum(mean_bound, 1e-300)).max()))
    assert numpy.all(error <= mean_bound)
    assert numpy.all(mu[::7] == 0)          # all-zero columns: exactly
    # total = sum of rows x features terms fl(fl(x - mu)^2): each term
    # within (1 + u)^3 of (x - mu)^2, the sum of them in any order within
    # gamma_{rows features}; as much again for NumPy's sum.  A mean that is
    # off by d_j moves column j's sum by at most 2 d_j sum_i |x_ij - mu_j|
    # + rows d_j^2.
    deviations = numpy.abs(x64 - want)
    want_total = float((deviations ** 2).sum())
    bound = (2 * gamma(rows * features + 3) * want_total
             + float((2 * mean_bound * deviations.sum(axis=0)
                      + rows * mean_bound ** 2).sum()))
    print("total: {:.17g} against {:.17g}, bound {:.3g}".format(
        total, want_total, bound))
    assert abs(total - want_total) <= bound
    if rows == 1:
        assert total == 0.0
    again_mu, again_total = device_moments(t)
    assert torch.equal(again_mu.cpu(), torch.from_numpy(mu))
    assert again_total == total


@pytest.mark.parametrize("block", BLOCKS + [32])
@pytest.mark.parametrize("rows,features,pitch", SHAPES)
def test_project_and_back_project(rows, features, pitch, block, cuda_device):
    x = kernel_case(rows, features)
    t = placed(x, pitch, cuda_device)
    rng = numpy.random.default_rng(block)
    # an asymmetric block: a swapped row and column cannot pass
    q = rng.standard_normal((features, block)) * (
        1 + numpy.arange(block)) + numpy.arange(features)[:, None] * 1e-3
    mu = x.astype(numpy.float64).mean(axis=0) * (1 + 1e-3)  # any mu is taken
    mu_device = torch.from_numpy(mu).to(cuda_device)
    centred = x.astype(numpy.float64) - mu
    y = device_project(t, mu_device, q)
    got = y.cpu().numpy()
    want = centred @ q
    # y_ib = sum_j fl(x_ij - mu_j) q_jb: one rounding in the subtraction,
    # one in each of the `features` multiply-adds, in any order:
    # gamma_{features+2} sum_j |x_ij - mu_j| |q_jb|; NumPy's product the same
    bound = 2 * gamma(features + 2) * (numpy.abs(centred) @ numpy.abs(q))
    error = numpy.abs(got - want)
    print("project: worst error {:.3g}, worst error / bound {:.3g}".format(
        error.max(), (error / numpy.maximum(bound, 1e-300)).max()))
    assert numpy.all(numpy.isfinite(got))
    assert numpy.all(error <= bound)
    # z_jb = sum_i fl(x_ij - mu_j) y_ib the same way over `rows` terms, from
    # the device's own y
    z = device_back_project(t, mu_device, y).cpu().numpy()
    want = centred.T @ got
    bound = 2 * gamma(rows + 2) * (numpy.abs(centred).T @ numpy.abs(got))
    error = numpy.abs(z - want)
    print("back-project: worst error {:.3g}, worst error / bound {:.3g}"
          .format(error.max(), (error / numpy.maximum(bound, 1e-300)).max()))
    assert numpy.all(numpy.isfinite(z))
    assert numpy.all(error <= bound)
    # the same bits again
    assert torch.equal(device_project(t, mu_device, q), y)
    assert numpy.array_equal(
        device_back_project(t, mu_device, y).cpu().numpy(), z)


def test_bad_arguments_through_the_entries(cuda_device):
    from scvae_amd import _lib
    lib = _lib.load()
    t = placed(kernel_case(17, 67), 67, cuda_device)
    mu, _ = device_moments(t)
    q = torch.zeros(67, 2, dtype=torch.float64, device=cuda_device)
    y = torch.zeros(17, 2, dtype=torch.float64, device=cuda_device)
    assert lib.scvae_pca_workspace_bytes(0, 67, 2) == -1
    assert lib.scvae_pca_workspace_bytes(17, 2 ** 20 + 1, 2) == -1
    assert lib.scvae_pca_workspace_bytes(17, 67, 33) == -1
    assert lib.scvae_pca_workspace_bytes(2 ** 31, 67, 2) == -1
    assert lib.scvae_pca_workspace_bytes(2 ** 31 - 1, 2 ** 20, 32) > 0
    for call in (
            lambda: lib.scvae_pca_project(_p(t), 66, 17, 67, _p(mu), _p(q), 2,
                                          _p(y), None),
            lambda: lib.scvae_pca_project(_p(t), 67, 17, 67, _p(mu), _p(q),
                                          33, _p(y), None),
            lambda: lib.scvae_pca_project(_p(t), 67, 17, 67, None, _p(q), 2,
                                          _p(y), None),
            lambda: lib.scvae_pca_project(
                ctypes.c_void_p(t.data_ptr() + 2), 67, 17, 67, _p(mu), _p(q),
                2, _p(y), None),
            lambda: lib.scvae_pca_moments(_p(t), 67, 17, 67, _p(mu), _p(y),
                                          None, 0, None),
            lambda: lib.scvae_pca_back_project(
                _p(t), 67, 0, 67, _p(mu), _p(y), 2, _p(q), None, 0, None)):
        assert call() == -1
        assert "bad argument" in lib.scvae_last_error().decode()
    torch.cuda.synchronize(cuda_device)


# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(n, f, seed):
    return Oracle(count_like(n, f, seed))


def check_fit(model, coordinates, x, reference):
    """A fitted ``DevicePCA`` and its coordinates against the oracle."""
    x64 = numpy.asarray(x, dtype=numpy.float64)
    components = model.components_.shape[0]
    assert model.components_.shape == (components, reference.features)
    assert coordinates.shape == (reference.rows, components)
    eigenvalues = model.singular_values_ ** 2
    mean_bound = reference.mean_bound(x64)
    assert numpy.all(numpy.abs(model.mean_ - reference.mean) <= mean_bound)
    for k in range(components):
        residual = float(model.residuals_[k])
        bound = reference.eigenvalue_bound(k, residual)
        error = abs(eigenvalues[k] - reference.eigenvalues[k])
        print("component {}: residual {:.3g}; eigenvalue error {:.3g} "
              "(bound {:.3g})".format(k, residual, error, bound))
        assert error <= bound
        # the sign rule, then the vector itself (measured directly)
        v = model.components_[k]
        assert v[numpy.argmax(numpy.abs(v))] > 0
        difference = float(numpy.linalg.norm(v - reference.components[k]))
        bound = reference.vector_bound(k, residual)
        print("    vector difference {:.3g} (bound {:.3g})".format(
            difference, bound))
        assert difference <= bound
        assert abs(numpy.linalg.norm(v) - 1) <= 64 * U * reference.features
        # coordinate i = (x_i - mu) . v_k: against the oracle's it moves by
        # at most ||xc_i|| ||v_k - v_k^ref|| (Cauchy-Schwarz), by the means'
        # difference along v (<= ||mean bound||), and by the rounding of
        # the two sums, 2 gamma_{F+2} sum_j |xc_ij| |v_kj|
        want = reference.centred @ reference.components[k]
        bound = (numpy.linalg.norm(reference.centred, axis=1) * difference
                 + numpy.linalg.norm(mean_bound)
                 + 2 * gamma(reference.features + 2)
                 * (numpy.abs(reference.centred) @ numpy.abs(v)))
        error = numpy.abs(coordinates[:, k] - want)
        print("    worst coordinate error {:.3g}, worst error / bound {:.3g}"
              .format(error.max(), (error / bound).max()))
        assert numpy.all(error <= bound)
        # explained-variance ratio lambda_k / total: the eigenvalue's bound
        # over the total, and the total's own rounding (a sum of N F terms)
        ratio = reference.eigenvalues[k] / reference.total
        bound = (reference.eigenvalue_bound(k, residual) / reference.total
                 + ratio * 4 * gamma(reference.rows * reference.features + 3))
        assert abs(model.explained_variance_ratio_[k] - ratio) <= bound
        assert model.explained_variance_[k] == (
            eigenvalues[k] / (reference.rows - 1)) or abs(
                model.explained_variance_[k] * (reference.rows - 1)
                - eigenvalues[k]) <= 4 * U * eigenvalues[k]


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("n,f,seed", SETS)
def test_fit_against_the_oracle(n, f, seed, block, cuda_device):
    from scvae_amd.analyses import DevicePCA
    x = count_like(n, f, seed)
    reference = oracle(n, f, seed)
    reference.assert_separated()
    model = DevicePCA(block_size=block, device=cuda_device)
    coordinates = model.fit_transform(x)
    print("{} iterations, residuals {}".format(
        model.n_iterations_, model.residuals_))
    assert model.converged_ is True
    assert model.n_iterations_ <= MAXIMUM_ITERATIONS
    assert numpy.all(model.residuals_ <= 1e-7)
    check_fit(model, coordinates, x, reference)


def test_same_bits_from_every_input(cuda_device):
    """Two fits with one seed, a sparse input and its dense form, a pitched
    tensor and its contiguous copy: identical bits."""
    import scipy.sparse
    from scvae_amd.analyses import DevicePCA
    n, f, seed = SETS[1]
    x = count_like(n, f, seed)

    def fit(values):
        model = DevicePCA(device=cuda_device)
        coordinates = model.fit_transform(values)
        return (coordinates, model.components_, model.mean_,
                model.explained_variance_ratio_, model.residuals_)
    first = fit(x)
    for values in (x, scipy.sparse.csr_matrix(x),
                   torch.from_numpy(numpy.array(x)).to(cuda_device),
                   placed(x, 2112, cuda_device)):
        for a, b in zip(first, fit(values)):
            assert numpy.array_equal(a, b)
    other = DevicePCA(seed=7, device=cuda_device).fit(x)
    assert not numpy.array_equal(other.components_, first[1])


def test_transform_of_a_second_set(cuda_device):
    import scipy.sparse
    from scvae_amd.analyses import DevicePCA
    n, f, seed = SETS[0]
    x = count_like(n, f, seed)
    reference = oracle(n, f, seed)
    reference.assert_separated()
    second = count_like(77, f, 11)
    model = DevicePCA(device=cuda_device)
    model.fit(x)
    got = model.transform(second)
    centred = second.astype(numpy.float64) - reference.mean
    mean_bound = reference.mean_bound(x)
    for k in range(2):
        difference = float(numpy.linalg.norm(
            model.components_[k] - reference.components[k]))
        assert difference <= reference.vector_bound(
            k, float(model.residuals_[k]))
        # as for the coordinates of the fitted set
        bound = (numpy.linalg.norm(centred, axis=1) * difference
                 + numpy.linalg.norm(mean_bound)
                 + 2 * gamma(f + 2)
                 * (numpy.abs(centred) @ numpy.abs(model.components_[k])))
        error = numpy.abs(got[:, k] - centred @ reference.components[k])
        assert numpy.all(error <= bound)
    assert numpy.array_equal(
        model.transform(scipy.sparse.csr_matrix(second)), got)
    with pytest.raises(ValueError, match="features expected"):
        model.transform(second[:, :-1])


def test_block_shrinks_to_the_rows(cuda_device):
    from scvae_amd.analyses import DevicePCA
    x = count_like(20, 2003, 6)
    reference = Oracle(x)
    model = DevicePCA(block_size=32, device=cuda_device)
    coordinates = model.fit_transform(x)
    # a block of N - 1 = 19 vectors spans the whole row space of the centred
    # matrix: the first Rayleigh-Ritz step is already exact
    assert model.converged_ and model.n_iterations_ <= 2
    assert model.operator_.shape == (20, 2003)
    check_fit(model, coordinates, x, reference)


def test_unconverged_fit_says_so(cuda_device, capsys):
    from scvae_amd.analyses import DevicePCA
    rng = numpy.random.default_rng(3)
    x = rng.standard_normal((400, 2100)).astype(numpy.float32)
    model = DevicePCA(maximum_iterations=2, device=cuda_device)
    coordinates = model.fit_transform(x)
    out = capsys.readouterr().out.splitlines()
    assert model.converged_ is False and model.n_iterations_ == 2
    assert len(out) == 1 and re.fullmatch(
        r"Decomposition not converged after 2 iterations \(largest residual "
        r"\S+, tolerance 1e-07\): these are the last Ritz pairs\.", out[0])
    for values in (coordinates, model.components_, model.residuals_,
                   model.explained_variance_ratio_, model.singular_values_):
        assert numpy.all(numpy.isfinite(values))
    assert numpy.all(model.residuals_ > 1e-7)


def test_constant_matrix_is_refused(cuda_device):
    from scvae_amd.analyses import DevicePCA
    x = numpy.full((30, 2100), 2.5, dtype=numpy.float32)
    with pytest.raises(ValueError, match="no variance"):
        DevicePCA(device=cuda_device).fit(x)


def test_decompose(cuda_device, capsys, monkeypatch):
    from sklearn.decomposition import PCA
    from scvae_amd.analyses import decompose
    from scvae_amd.analyses import decomposition
    n, f, seed = SETS[0]
    x = count_like(n, f, seed)
    small = numpy.array(x[:, :50])
    # up to 2000 dense features: scikit-learn's PCA, as in the reference
    output = decompose(small)
    assert isinstance(output, list) and len(output) == 1
    assert numpy.array_equal(output[0], PCA(n_components=2).fit_transform(
        small))
    fitted = []
    fit_transform = decomposition.DevicePCA.fit_transform

    def spy(self, values):
        fitted.append(self)
        return fit_transform(self, values)
    monkeypatch.setattr(decomposition.DevicePCA, "fit_transform", spy)
    decompose(small)
    assert not fitted
    # the reference's list shapes, on the device path (2101 features)
    other = count_like(40, f, 12)
    centroids = {"means": numpy.stack([x[0], x[1], x[2]]).astype("f8"),
                 "covariance_matrices": numpy.stack(
                     [numpy.diag(numpy.arange(f, dtype="f8") + k)
                      for k in range(3)]),
                 "probabilities": numpy.ones(3) / 3}
    output = decompose(x)
    assert len(output) == 1 and len(fitted) == 1
    model = fitted[0]
    assert model.converged_
    check_fit(model, output[0], x, oracle(n, f, seed))
    capsys.readouterr()
    output = decompose(x, other_value_sets={"other": other, "none": None},
                       centroids=centroids)
    assert len(output) == 3 and len(fitted) == 2
    assert numpy.array_equal(output[0], decompose(x)[0])
    model = fitted[1]
    assert set(output[1]) == {"other", "none"} and output[1]["none"] is None
    assert numpy.array_equal(output[1]["other"], model.transform(other))
    assert output[1]["other"].shape == (40, 2)
    assert set(output[2]) == set(centroids)
    assert output[2]["means"].shape == (3, 2)
    assert numpy.allclose(
        output[2]["means"],
        (centroids["means"] - model.mean_) @ model.components_.T,
        rtol=0, atol=1e-9)
    assert output[2]["covariance_matrices"].shape == (3, 2, 2)
    assert numpy.array_equal(
        output[2]["covariance_matrices"][1],
        model.components_ @ centroids["covariance_matrices"][1]
        @ model.components_.T)
    assert output[2]["probabilities"] is centroids["probabilities"]
    output = decompose(x, other_value_sets=None, centroids=None)
    assert len(output) == 3 and output[1] is None and output[2] is None
    assert capsys.readouterr().out == ""
    for method in ("svd", "ICA", "t-SNE"):
        with pytest.raises(NotImplementedError, match=r"decomposition\.py"):
            decompose(x, method=method)
    with pytest.raises(ValueError, match="not found"):
        decompose(x, method="umap")
    # outside the device limits: one line with the reason, then scikit-learn
    from sklearn.decomposition import IncrementalPCA
    monkeypatch.setattr(decomposition, "MAXIMUM_NUMBER_OF_FEATURES", 2100)
    output = decompose(x)
    assert capsys.readouterr().out == (
        "decomposition on the device not used: 2101 features (1 to 2100 "
        "supported).\n")
    assert len(fitted) == 4
    assert numpy.array_equal(output[0], IncrementalPCA(
        n_components=2, batch_size=100).fit_transform(x))


# ---------------------------------------------------------------------------
def _tiny_set():
    import scipy.sparse
    from scvae_amd.data import DataSet
    n, f = 200, 2101
    x = count_like(300, f, 1)[:n]
    return DataSet("tiny", values=scipy.sparse.csr_matrix(x),
                   example_names=numpy.array(
                       ["cell {}".format(i) for i in range(n)]),
                   feature_names=numpy.arange(f).astype(str), kind="test")


def _check_attached(fit, values, projected=None):
    """An attached decomposition against the oracle of ``values`` (with
    ``projected``: those rows in the space of ``values``)."""
    reference = Oracle(values)
    model = fit["model"]
    assert fit["components"] is model.components_
    assert fit["mean"] is model.mean_
    assert fit["iterations"] == model.n_iterations_
    assert fit["converged"] == model.converged_
    assert fit["duration"] > 0
    assert numpy.array_equal(fit["explained_variance_ratio"],
                             model.explained_variance_ratio_)
    if projected is None:
        check_fit(model, fit["coordinates"], values, reference)
        return
    check_fit(model, fit["fitted_coordinates"], values, reference)
    centred = numpy.asarray(projected, dtype=numpy.float64) - reference.mean
    mean_bound = reference.mean_bound(values)
    for k in range(2):
        difference = float(numpy.linalg.norm(
            model.components_[k] - reference.components[k]))
        bound = (numpy.linalg.norm(centred, axis=1) * difference
                 + numpy.linalg.norm(mean_bound)
                 + 2 * gamma(reference.features + 2)
                 * (numpy.abs(centred) @ numpy.abs(model.components_[k])))
        error = numpy.abs(
            fit["coordinates"][:, k] - centred @ reference.components[k])
        assert numpy.all(error <= bound)


def test_through_the_model(tmp_path, cuda_device):
    from scvae_amd.models import VariationalAutoencoder
    data_set = _tiny_set()
    state = numpy.random.get_state()
    numpy.random.seed(7)
    try:
        model = VariationalAutoencoder(
            feature_size=2101, latent_size=3, hidden_sizes=[8],
            reconstruction_distribution="negative binomial",
            log_directory=str(tmp_path))
        model.train(data_set, number_of_epochs=1, minibatch_size=50)
    finally:
        numpy.random.set_state(state)
    arguments = dict(minibatch_size=50, use_deterministic_z=True,
                     log_results=False)
    plain = model.evaluate(data_set, **arguments)
    assert not hasattr(plain[1], "decomposition")
    extensive = model.evaluate(data_set, decompositions="extensive",
                               **arguments)
    assert numpy.array_equal(extensive[1].values, plain[1].values)
    original = numpy.asarray(data_set.values.todense(), dtype=numpy.float32)
    _check_attached(extensive[1].decomposition, extensive[1].values)
    _check_attached(extensive[1].decomposition_in_original_space, original,
                    projected=extensive[1].values)
    for level in (True, "normal"):
        normal = model.evaluate(data_set, decompositions=level, **arguments)
        assert not hasattr(normal[1], "decomposition_in_original_space")
        assert numpy.array_equal(normal[1].decomposition["coordinates"],
                                 extensive[1].decomposition["coordinates"])
    with pytest.raises(ValueError, match="reconstructed"):
        model.evaluate(data_set, decompositions=True,
                       output_versions=["latent"], **arguments)
    with pytest.raises(ValueError, match="`all` not found"):
        model.evaluate(data_set, decompositions="all", **arguments)


def test_through_the_command_line(tmp_path, cuda_device, monkeypatch, capsys):
    from scvae_amd import cli
    data_set = _tiny_set()
    monkeypatch.setattr(
        cli, "_load_data",
        lambda *a, **kw: (data_set, (data_set, None, data_set), None, None))
    models, analyses = tmp_path / "models", tmp_path / "analyses"
    monkeypatch.setattr(
        cli, "build_directory_path",
        lambda base, **kw: str(analyses if base == "the analyses"
                               else models))
    monkeypatch.setattr(cli, "indices_for_evaluation_subset",
                        lambda data_set: set())
    arguments = dict(latent_size=3, hidden_sizes=[8], minibatch_size=50,
                     reconstruction_distribution="negative binomial",
                     analyses_directory="the analyses")
    cli.train("tiny", number_of_epochs=1, **arguments)
    capsys.readouterr()
    # without the switch: no new lines and no files
    cli.evaluate("tiny", sample_size=0, **arguments)
    plain = capsys.readouterr().out
    assert "ecompos" not in plain and "Explained variance" not in plain
    assert not analyses.exists()
    cli.evaluate("tiny", sample_size=0, analysis_level="extensive",
                 **arguments)
    assert not analyses.exists()
    assert [re.sub(r"\(.*?\)", "()", line) for line in
            capsys.readouterr().out.splitlines()] == [
                re.sub(r"\(.*?\)", "()", line) for line in plain.splitlines()]
    results = cli.evaluate(
        "tiny", sample_size=0, decompositions=True,
        decomposition_methods=["pca", "t-SNE"], analysis_level="extensive",
        **arguments)
    lines = capsys.readouterr().out.splitlines()
    reconstructed = results["end_of_training"][1]
    _check_attached(reconstructed.decomposition, reconstructed.values)
    assert lines.count(
        "Decomposition method `t-SNE` is not built: skipped.") == 1
    for fit, fit_title, name in (
            (reconstructed.decomposition, "reconstructions set",
             "reconstructions"),
            (reconstructed.decomposition_in_original_space,
             "reconstructed set values in originals set",
             "reconstructed-originals")):
        at = lines.index("Decomposing {} using PCA.".format(fit_title))
        assert re.fullmatch(re.escape(
            fit_title[0].upper() + fit_title[1:]) + r" decomposed \(.+\)\.",
            lines[at + 1])
        assert lines[at + 2] == (
            "    Explained variance ratios: {:.5g}, {:.5g}; {} iterations."
            .format(*fit["explained_variance_ratio"], fit["iterations"]))
        assert lines[at + 3] == ""
        files = list(analyses.glob("**/{}/pca.tsv".format(name)))
        assert len(files) == 1
        relative = files[0].relative_to(analyses).parts
        # <model name>/e_<epochs>-mc_<n>-iw_<n>/<name>/pca.tsv
        assert relative[-2:] == (name, "pca.tsv")
        assert re.fullmatch(r"e_1-mc_\d+-iw_\d+", relative[-3])
        assert relative[0] == "VAE" and len(relative) > 4
        rows = files[0].read_text().splitlines()
        assert rows[0].split("\t") == ["example", "PC 1", "PC 2"]
        assert len(rows) == 201
        for i in (0, 199):
            fields = rows[1 + i].split("\t")
            assert fields[0] == "cell {}".format(i)
            assert [float(fields[1]), float(fields[2])] == list(
                fit["coordinates"][i])
    # with a sample: the sampled set in the fitted space, beside the file
    results = cli.evaluate("tiny", sample_size=20, decompositions=True,
                           **arguments)
    capsys.readouterr()
    (reconstructed_set, sampled_set) = (
        results["end_of_training"][0][1], results["end_of_training"][1])
    assert not hasattr(reconstructed_set, "decomposition_in_original_space")
    files = list(analyses.glob("**/reconstructions/pca-sampled.tsv"))
    assert len(files) == 1
    rows = files[0].read_text().splitlines()
    assert len(rows) == 21 and rows[0].split("\t") == [
        "example", "PC 1", "PC 2"]
    want = reconstructed_set.decomposition["model"].transform(
        sampled_set.values)
    assert want.shape == (20, 2)
    assert [float(v) for v in rows[20].split("\t")[1:]] == list(want[19])
    # a method that is not built, alone: one line, nothing fitted
    results = cli.evaluate("tiny", sample_size=0, decompositions=True,
                           decomposition_methods="ica", **arguments)
    out = capsys.readouterr().out
    assert out.count("Decomposition method `ICA` is not built: skipped.") == 1
    assert "Decomposing" not in out
    assert not hasattr(results["end_of_training"][1], "decomposition")
