"""``csrc/distances.hip`` element by element against the fp64 direct-form
oracle (``_distances_oracle.py``, which also derives the bounds), its exact
properties, ``pairwise_distances`` across input types, and the switch through
``ModelBase.evaluate`` and the command line."""
import ctypes
import os
import re

import numpy
import pytest
import scipy.sparse
import torch

import _distances_oracle as oracle

pytestmark = pytest.mark.gpu

EUCLIDEAN, COSINE = 0, 1
METRICS = (("euclidean", EUCLIDEAN, oracle.euclidean_oracle,
            oracle.euclidean_bound),
           ("cosine", COSINE, oracle.cosine_oracle, oracle.cosine_bound))

# (rows, features): one row; below one MFMA block; across one tile edge (129)
# and two (260); below one K step of 4 (1, 3), K tails (5, 67), one staged
# step of 32 and one past it (32, 33), whole steps (64) and many (2050).  K is
# not split, so there is no chunk length to step past.
SHAPES = [(1, 1), (2, 3), (17, 5), (17, 64), (129, 67), (129, 1), (260, 33),
          (260, 2050), (2, 2050), (130, 32)]


def kernel_case(rows, features):
    """As ``test_gpu_pca.kernel_case``: non-integer fp32 values, about 70 %
    zeros, some all-zero columns; and some all-zero rows."""
    rng = numpy.random.default_rng(1000 * rows + features)
    x = (rng.poisson(3.0, (rows, features)) * rng.random((rows, features))
         * (rng.random((rows, features)) < 0.3)).astype(numpy.float32)
    x[:, ::7] = 0
    x[5::11] = 0
    x.setflags(write=False)
    return x


def _p(tensor):
    return ctypes.c_void_p(tensor.data_ptr()) if tensor is not None else None


def run_kernel(x, metric, rows=None, ldo=None):
    """``scvae_pairwise_distances`` on the device tensor ``x`` [N, F] (any
    row pitch); returns the [n, n] result on the host."""
    from scvae_amd import _lib
    lib = _lib.load()
    total_rows, features = x.shape
    index = (torch.as_tensor(numpy.asarray(rows, dtype=numpy.int64))
             .to(x.device) if rows is not None else None)
    n = total_rows if rows is None else len(rows)
    ldo = n if ldo is None else ldo
    out = torch.full((n, ldo), -7.0, dtype=torch.float32, device=x.device)
    size = lib.scvae_pairwise_distances_workspace_bytes(n, features)
    assert size >= 8 * n
    workspace = torch.empty(size, dtype=torch.uint8, device=x.device)
    pitch = x.stride(0) if total_rows > 1 else features
    rc = lib.scvae_pairwise_distances(
        _p(x), pitch, total_rows, features, _p(index), n, metric, _p(out),
        ldo, _p(workspace), size, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.scvae_last_error()
    result = out.cpu().numpy()
    if ldo > n:     # nothing is written past the n columns
        assert numpy.all(result[:, n:] == -7.0)
    return result[:, :n]


def assert_within(got, x, reference, bound, what):
    want = reference(x)
    allowed = bound(x, want)
    error = numpy.abs(got.astype(numpy.float64) - want)
    worst = numpy.unravel_index(numpy.argmax(error / allowed), error.shape)
    print("{}: largest error over its bound {:.3f} at {}: error {:.3e}, "
          "allowed {:.3e}".format(what, error[worst] / allowed[worst], worst,
                                  error[worst], allowed[worst]))
    assert numpy.all(numpy.isfinite(got)), what
    assert numpy.all(error <= allowed), (what, worst, error[worst],
                                         allowed[worst])


def assert_exact_properties(got, what):
    assert numpy.array_equal(got.view(numpy.uint32),
                             got.T.view(numpy.uint32)), what
    assert numpy.all(numpy.diag(got).view(numpy.uint32) == 0), what


@pytest.mark.parametrize("rows,features", SHAPES)
def test_kernel_against_the_oracle(cuda_device, rows, features):
    x = kernel_case(rows, features)
    on_device = torch.from_numpy(numpy.array(x)).to(cuda_device)
    for name, flag, reference, bound in METRICS:
        what = "{} {}x{}".format(name, rows, features)
        got = run_kernel(on_device, flag)
        assert_within(got, x, reference, bound, what)
        assert_exact_properties(got, what)
        again = run_kernel(on_device, flag)
        assert numpy.array_equal(got.view(numpy.uint32),
                                 again.view(numpy.uint32)), what
        if flag == COSINE:     # a zero row: exactly 1 to every other row
            zero = numpy.flatnonzero(~x.any(axis=1))
            for r in zero:
                assert numpy.all(numpy.delete(got[r], r) == 1.0), what
            assert rows < 6 or zero.size > 0


def test_row_pitch_and_output_pitch(cuda_device):
    """The matrix as a column slice of a wider NaN-filled tensor (an odd
    pitch: rows at 4-byte alignment only), the output in a wider one."""
    x = kernel_case(131, 67)
    wide = torch.full((131, 67 + 10), float("nan"), dtype=torch.float32,
                      device=cuda_device)
    view = wide[:, 4:4 + 67]
    view.copy_(torch.from_numpy(numpy.array(x)))
    assert view.stride(0) == 77
    plain = torch.from_numpy(numpy.array(x)).to(cuda_device)
    for name, flag, reference, bound in METRICS:
        got = run_kernel(view, flag, ldo=140)
        assert_within(got, x, reference, bound, name + " pitch")
        assert numpy.array_equal(
            got.view(numpy.uint32),
            run_kernel(plain, flag).view(numpy.uint32))


def test_row_index_with_duplicates(cuda_device):
    """Through a row index, reversed and with duplicates, into a larger
    matrix: the gathered copy's bits, and duplicates at exactly 0."""
    x = kernel_case(400, 67)
    rng = numpy.random.default_rng(8)
    rows = rng.permutation(400)[:150][::-1].copy()
    nonzero = [r for r in rows if x[r].any()]
    rows[140:150] = nonzero[:10]          # ten rows twice
    rows[17] = rows[3] = nonzero[20]      # and across the tile edge: 3, 139
    rows[139] = nonzero[20]
    on_device = torch.from_numpy(numpy.array(x)).to(cuda_device)
    gathered = torch.from_numpy(numpy.array(x[rows])).to(cuda_device)
    for name, flag, reference, bound in METRICS:
        got = run_kernel(on_device, flag, rows=rows)
        assert_within(got, x[rows], reference, bound, name + " index")
        assert_exact_properties(got, name)
        assert numpy.array_equal(
            got.view(numpy.uint32),
            run_kernel(gathered, flag).view(numpy.uint32)), name
        same = (rows[:, None] == rows[None, :])
        assert same.sum() > 150 + 20
        assert numpy.all(got[same].view(numpy.uint32) == 0), name


def test_large_magnitudes_and_one_ulp(cuda_device):
    """Magnitudes near 1e4, two rows that differ in one element by one ulp,
    and two rows with identical values: the expanded form cancels here, the
    bound says by how much, and identical rows still cancel exactly."""
    rng = numpy.random.default_rng(4)
    x = (1e4 * (0.5 + rng.random((20, 67)))).astype(numpy.float32)
    x[11] = x[2]
    x[11, 30] = numpy.nextafter(x[2, 30], numpy.float32(numpy.inf))
    x[15] = x[6]
    on_device = torch.from_numpy(x).to(cuda_device)
    for name, flag, reference, bound in METRICS:
        got = run_kernel(on_device, flag)
        assert_within(got, x, reference, bound, name + " 1e4")
        assert_exact_properties(got, name)
        assert got[15, 6].view(numpy.uint32) == 0, name
    assert oracle.euclidean_oracle(x)[11, 2] == float(x[11, 30] - x[2, 30])


def test_non_finite_values_propagate(cuda_device):
    x = numpy.array(kernel_case(20, 9))
    x[3, 1] = numpy.nan
    x[8, 2] = numpy.inf
    on_device = torch.from_numpy(x).to(cuda_device)
    for name, flag, _, _ in METRICS:
        got = run_kernel(on_device, flag)
        bad = numpy.zeros((20, 20), dtype=bool)
        bad[[3, 8], :] = bad[:, [3, 8]] = True
        numpy.fill_diagonal(bad, False)
        assert numpy.all(numpy.isnan(got[bad])), name
        assert numpy.all(numpy.isfinite(got[~bad])), name
        assert numpy.all(numpy.diag(got) == 0), name


def test_bad_arguments(cuda_device):
    from scvae_amd import _lib
    lib = _lib.load()
    x = torch.zeros(8, 6, dtype=torch.float32, device=cuda_device)
    out = torch.zeros(8, 8, dtype=torch.float32, device=cuda_device)
    workspace = torch.zeros(1024, dtype=torch.uint8, device=cuda_device)
    index = torch.zeros(8, dtype=torch.int64, device=cuda_device)
    good = dict(x=_p(x), ldx=6, total=8, F=6, rows=None, n=8, metric=0,
                out=_p(out), ldo=8, ws=_p(workspace), size=1024)

    def call(**changes):
        a = dict(good, **changes)
        return lib.scvae_pairwise_distances(
            a["x"], a["ldx"], a["total"], a["F"], a["rows"], a["n"],
            a["metric"], a["out"], a["ldo"], a["ws"], a["size"], None)

    assert call() == 0
    assert call(rows=_p(index)) == 0
    torch.cuda.synchronize()
    for changes in (dict(x=None), dict(out=None), dict(ws=None),
                    dict(n=0), dict(n=2 ** 16 + 1), dict(F=0),
                    dict(F=2 ** 20 + 1, ldx=2 ** 20 + 1), dict(ldx=5),
                    dict(n=9), dict(total=0), dict(metric=2),
                    dict(metric=-1), dict(ldo=7), dict(size=8 * 8 - 1),
                    dict(x=ctypes.c_void_p(x.data_ptr() + 2))):
        assert call(**changes) == -1, changes
        assert b"bad argument" in lib.scvae_last_error(), changes
    torch.cuda.synchronize()


def test_pairwise_distances_across_input_types(cuda_device, capsys):
    from scvae_amd.analyses.distances import pairwise_distances
    x = numpy.array(kernel_case(150, 41))
    rows = numpy.random.default_rng(2).permutation(150)[:70]
    on_device = torch.from_numpy(x).to(cuda_device)
    sparse = scipy.sparse.csr_matrix(x)
    for metric in ("Euclidean", "cosine"):
        for index in (None, rows):
            from_tensor = pairwise_distances(on_device, metric, rows=index)
            assert isinstance(from_tensor, torch.Tensor)
            assert from_tensor.is_cuda and from_tensor.dtype == torch.float32
            from_numpy = pairwise_distances(x, metric, rows=index)
            from_sparse = pairwise_distances(sparse, metric, rows=index)
            for other in (from_numpy, from_sparse):
                assert isinstance(other, numpy.ndarray)
                assert other.dtype == numpy.float32
                assert numpy.array_equal(
                    other.view(numpy.uint32),
                    from_tensor.cpu().numpy().view(numpy.uint32))
            n = 150 if index is None else 70
            assert from_numpy.shape == (n, n)
    assert capsys.readouterr().out == ""
    # past the row limit: the line, and scikit-learn's matrix
    import sklearn.metrics
    got = pairwise_distances(on_device, "cosine", maximum_rows=149)
    assert capsys.readouterr().out == (
        "distances on the device not used: 150 rows (1 to 149 supported).\n")
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert numpy.array_equal(
        got.cpu().numpy(), sklearn.metrics.pairwise_distances(
            x, metric="cosine").astype(numpy.float32))
    got = pairwise_distances(x, "euclidean", rows=rows, maximum_rows=70)
    assert capsys.readouterr().out == ""
    host = pairwise_distances(x, "euclidean", rows=rows, on_device=False)
    assert numpy.allclose(got, host, rtol=0, atol=1e-5)


def _small_set(n=1003, features=37):
    from scvae_amd.data import DataSet
    rng = numpy.random.default_rng(23)
    x = (rng.poisson(2.0, (n, features))
         * (rng.random((n, features)) < 0.5)).astype(numpy.float32)
    labels = numpy.array(["b cell", "t cell", "nk"])[rng.integers(0, 3, n)]
    return DataSet("tiny", values=scipy.sparse.csr_matrix(x), labels=labels,
                   example_names=numpy.array(
                       ["cell {}".format(i) for i in range(n)]),
                   feature_names=numpy.arange(features).astype(str),
                   kind="test")


def _files(directory):
    return sorted(os.path.relpath(os.path.join(root, name), directory)
                  for root, _, names in os.walk(directory) for name in names)


def test_through_the_command_line(tmp_path, cuda_device, monkeypatch, capsys):
    from scvae_amd import cli
    from scvae_amd.analyses.distances import (
        hierarchical_order, pairwise_distances)
    data_set = _small_set()
    n = data_set.number_of_examples
    models, analyses = tmp_path / "models", tmp_path / "analyses"
    monkeypatch.setattr(
        cli, "_load_data",
        lambda *a, **kw: (data_set, (data_set, None, data_set), None, None))
    monkeypatch.setattr(
        cli, "build_directory_path",
        lambda base, *a, **kw: str(
            analyses if "analyses" in str(base) else models))
    monkeypatch.setattr(cli, "indices_for_evaluation_subset",
                        lambda data_set: set())
    arguments = dict(latent_size=3, hidden_sizes=[12], minibatch_size=128,
                     reconstruction_distribution="poisson",
                     models_directory="models",
                     analyses_directory="analyses")
    cli.train("tiny", number_of_epochs=1, **arguments)
    capsys.readouterr()
    plain_results = cli.evaluate("tiny", sample_size=0, **arguments)
    plain = capsys.readouterr().out
    files_before = _files(tmp_path)
    assert "distances" not in plain
    assert not analyses.exists()
    assert not hasattr(plain_results["end_of_training"][1],
                       "distance_matrices")
    results = cli.evaluate("tiny", sample_size=0, distances=True,
                           **arguments)
    lines = capsys.readouterr().out.splitlines()
    # the new block: two sets, each a heading, four matrices, a blank line
    at = lines.index("Plotting pairwise distances in reconstructed space.")
    block = lines[at:at + 12]
    duration = r" plotted and saved \(.+\)\."
    for first, version in ((0, "reconstructed"), (6, "z")):
        assert block[first] == (
            "Plotting pairwise distances in {} space.".format(version))
        for k, (metric, sampled, method) in enumerate((
                ("Euclidean", "", "labels"), ("Cosine", "", "labels"),
                ("Euclidean", " for 1000 randomly sampled examples",
                 "hierarchical clustering"),
                ("Cosine", " for 1000 randomly sampled examples",
                 "hierarchical clustering"))):
            assert re.fullmatch(
                "    {} distances in {} space{} sorted using {}".format(
                    metric, version, sampled, method) + duration,
                block[first + 1 + k]), block[first + 1 + k]
        assert block[first + 5] == ""
    # less the new block the text is that of the plain run
    # (durations and the figures of a sampled evaluation differ run to run)
    numbers = re.compile(r"<?[-+]?\d[\d.e+-]*( [a-z]+)?")
    assert [numbers.sub("#", line) for line in lines[:at] + lines[at + 12:]
            ] == [numbers.sub("#", line) for line in plain.splitlines()]
    reconstructed_set, latent_sets = results["end_of_training"][1:3]
    assert numpy.array_equal(reconstructed_set.values,
                             plain_results["end_of_training"][1].values)
    written = [name for name in _files(tmp_path) if name not in files_before
               and name.startswith("analyses")]
    names = ["distances-{}-{}-{}".format(version, metric, method)
             for version in ("reconstructed", "z")
             for method in ("labels", "hierarchical_clustering")
             for metric in ("euclidean", "cosine")]
    assert sorted(os.path.basename(name) for name in written) == sorted(
        name + extension for name in names for extension in (".npy", ".tsv"))
    assert all(os.path.basename(os.path.dirname(name)) == "distances"
               for name in written)
    directory = tmp_path / os.path.dirname(written[0])
    for data, version in ((reconstructed_set, "reconstructed"),
                          (latent_sets["z"], "z")):
        assert [m["name"] for m in data.distance_matrices] == [
            name for name in names if "-{}-".format(version) in name]
        values = torch.from_numpy(numpy.ascontiguousarray(
            data.values, dtype=numpy.float32)).to(cuda_device)
        for matrix in data.distance_matrices:
            stored = numpy.load(directory / (matrix["name"] + ".npy"))
            table = [line.split("\t") for line in (
                directory / (matrix["name"] + ".tsv")).read_text()
                .splitlines()]
            assert table[0] == ["position", "index", "example", "label"]
            indices = numpy.array([int(row[1]) for row in table[1:]])
            assert [row[2] for row in table[1:]] == [
                "cell {}".format(i) for i in indices]
            assert [row[3] for row in table[1:]] == (
                data_set.labels[indices].tolist())
            size = n if matrix["sorting_method"] == "labels" else 1000
            assert stored.shape == (size, size)
            assert stored.dtype == numpy.float32
            assert numpy.array_equal(indices, matrix["indices"])
            want = pairwise_distances(values, matrix["metric"],
                                      rows=indices).cpu().numpy()
            assert numpy.array_equal(stored.view(numpy.uint32),
                                     want.view(numpy.uint32)), matrix["name"]
            if matrix["sorting_method"] == "labels":
                assert data_set.labels[indices].tolist() == sorted(
                    data_set.labels.tolist())
            else:
                sample = numpy.random.RandomState(57).permutation(n)[:1000]
                unsorted = pairwise_distances(
                    values, matrix["metric"], rows=sample).cpu().numpy()
                order = hierarchical_order(unsorted)
                assert numpy.array_equal(indices, sample[order])


def test_through_the_model(tmp_path, cuda_device):
    from scvae_amd.models import VariationalAutoencoder
    data_set = _small_set(n=70)
    state = numpy.random.get_state()
    numpy.random.seed(7)
    try:
        model = VariationalAutoencoder(
            feature_size=37, latent_size=3, hidden_sizes=[12],
            reconstruction_distribution="poisson",
            log_directory=str(tmp_path))
        model.train(data_set, number_of_epochs=1, minibatch_size=32)
    finally:
        numpy.random.set_state(state)
    arguments = dict(minibatch_size=32, use_deterministic_z=True,
                     log_results=False)
    plain = model.evaluate(data_set, **arguments)
    assert not hasattr(plain[1], "distance_matrices")
    assert not hasattr(plain[2]["z"], "distance_matrices")
    both = model.evaluate(data_set, distances=True, **arguments)
    assert numpy.array_equal(both[1].values, plain[1].values)
    assert len(both[1].distance_matrices) == 4
    assert len(both[2]["z"].distance_matrices) == 4
    assert both[1].distance_matrices[0]["distances"].shape == (70, 70)
    assert both[1].distance_matrices[0]["sample_size"] is None
    only = model.evaluate(data_set, distances=True,
                          output_versions=["reconstructed"], **arguments)
    assert len(only.distance_matrices) == 4
    with pytest.raises(ValueError, match="reconstructed"):
        model.evaluate(data_set, distances=True,
                       output_versions=["latent"], **arguments)
    with pytest.raises(ValueError, match="`all` not found"):
        model.evaluate(data_set, distances="all", **arguments)
