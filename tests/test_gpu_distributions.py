"""``scvae_amd/analyses/distributions.py`` on the device against its host
path, which is ``numpy.histogram`` itself: equal counts, equal edge bits.
Then the switch through ``ModelBase.evaluate`` and the command line."""
import os
import re

import numpy
import pytest
import scipy.sparse
import torch

from test_distributions_host import (KINDS, SIZES, same_bits, series_of,
                                     small_sets)

pytestmark = pytest.mark.gpu


def test_histogram_equals_numpy(cuda_device, capsys):
    from scvae_amd.analyses import distributions as D
    for k, kind in enumerate(KINDS):
        for n in SIZES:
            x = series_of(kind, n, 100 * k + n)
            on_device = torch.from_numpy(x).to(cuda_device)
            for shift in (False, True):
                shifted = x + numpy.float32(1) if shift else x
                for bins in ("auto", 1, 10, 20000):
                    for values in (on_device, x):
                        counts, edges = D.histogram(
                            values, bins=bins, shift=shift, on_device=True)
                        want, want_edges = numpy.histogram(shifted, bins=bins)
                        assert same_bits(edges, want_edges), (kind, n, bins)
                        assert numpy.array_equal(counts, want), (kind, n, bins)
                        assert counts.dtype == numpy.int64
                # plot_histogram's ranges: the extremes, and the discrete rule
                for bin_range in (numpy.array((shifted.min(), shifted.max())),
                                  numpy.array((-0.5, shifted.max() + 0.5))):
                    counts, edges = D.histogram(
                        on_device, bins=37, range=bin_range, shift=shift,
                        excess_zero_count=11)
                    want, want_edges = numpy.histogram(
                        shifted, bins=37, range=bin_range)
                    want[0] += 11
                    assert same_bits(edges, want_edges)
                    assert numpy.array_equal(counts, want)
    assert capsys.readouterr().out == ""


def test_percentile_and_order_statistics(cuda_device):
    from scvae_amd.analyses import distributions as D
    for k, kind in enumerate(KINDS):
        for n in (2, 5, 257, 5000):
            x = series_of(kind, n, 50 * k + n)
            on_device = torch.from_numpy(x).to(cuda_device)
            qs = [75, 25, 0, 100, 50, 12.5]
            assert same_bits(D.percentile(on_device, qs),
                             numpy.percentile(x, qs))
            assert same_bits(D.percentile(x, 33.0),
                             numpy.percentile(x, [33.0])[0])
            ranks = [0, n - 1, n // 2, n // 3, (2 * n) // 3]
            assert same_bits(D.order_statistics(on_device, ranks),
                             numpy.sort(x)[ranks])
    matrix = torch.from_numpy(series_of("gamma", 63 * 70, 3).reshape(
        63, 70)).to(cuda_device)
    padded = matrix[:, :65]           # a row pitch, read in place
    assert same_bits(D.percentile(padded, [25, 75]),
                     numpy.percentile(padded.cpu().numpy(), [25, 75]))
    sparse = scipy.sparse.random(30, 40, density=0.2, format="csr",
                                 dtype=numpy.float32, random_state=1)
    assert same_bits(D.order_statistics(sparse, [0, sparse.data.size - 1]),
                     numpy.sort(sparse.data)[[0, -1]])
    with pytest.raises(ValueError, match="outside"):
        D.order_statistics(on_device, [n])


def test_errors_and_fallback(cuda_device, capsys):
    from scvae_amd.analyses import distributions as D
    x = series_of("gamma", 1000, 1)
    on_device = torch.from_numpy(x).to(cuda_device)
    # one bin more than the device takes: the host path, and the line
    bins = 2 ** 20 + 1
    counts, edges = D.histogram(on_device, bins=bins)
    assert capsys.readouterr().out == (
        "distributions on the device not used: {} bins, more than {}.\n"
        .format(bins, 2 ** 20))
    want, want_edges = numpy.histogram(x, bins=bins)
    assert numpy.array_equal(counts, want) and same_bits(edges, want_edges)
    counts, edges = D.histogram(on_device, bins=2 ** 20)
    assert capsys.readouterr().out == ""
    assert numpy.array_equal(counts, numpy.histogram(x, bins=2 ** 20)[0])
    # automatic bins with values outside the range: NumPy drops them first
    counts, edges = D.histogram(on_device, bins="auto", range=(0.5, 2.0))
    assert "not used: automatic bins with values outside" in (
        capsys.readouterr().out)
    want, want_edges = numpy.histogram(x, bins="auto", range=(0.5, 2.0))
    assert numpy.array_equal(counts, want) and same_bits(edges, want_edges)
    # NumPy's errors, in NumPy's words
    for bad_value in (numpy.nan, numpy.inf):
        bad = x.copy()
        bad[17] = bad_value
        with pytest.raises(ValueError) as theirs:
            numpy.histogram(bad, bins=5)
        with pytest.raises(ValueError) as ours:
            D.histogram(torch.from_numpy(bad).to(cuda_device), bins=5)
        assert str(ours.value) == str(theirs.value)
        assert "is not finite" in str(ours.value)
    tiny = numpy.array([1.0, numpy.nextafter(numpy.float32(1), 2)],
                       dtype=numpy.float32)
    with pytest.raises(ValueError, match="Too many bins for data range"):
        D.histogram(torch.from_numpy(tiny).to(cuda_device), bins=5)
    # values outside a given range are left out, NaN too
    bad = x.copy()
    bad[3] = numpy.nan
    counts, _ = D.histogram(torch.from_numpy(bad).to(cuda_device), bins=9,
                            range=(0.5, 2.0))
    assert numpy.array_equal(
        counts, numpy.histogram(bad, bins=9, range=(0.5, 2.0))[0])


def _same_histograms(got, want):
    assert [h["name"] for h in got] == [h["name"] for h in want]
    for ours, theirs in zip(got, want):
        assert same_bits(ours["edges"], theirs["edges"]), ours["name"]
        assert numpy.array_equal(ours["counts"], theirs["counts"]), (
            ours["name"])
        assert same_bits(ours["frequencies"], theirs["frequencies"])


def test_three_histograms_equal_the_host_path(cuda_device):
    from scvae_amd.analyses import distributions as D
    for label, values, discrete in small_sets():
        want = D.distribution_histograms(values, name="test",
                                         discrete=discrete, on_device=False)
        got = D.distribution_histograms(values, name="test",
                                        discrete=discrete, on_device=True)
        _same_histograms(got, want)


def _case_300_257(device):
    from scvae_amd.minibatch import DeviceCSR
    rng = numpy.random.default_rng(77)
    rows, features = 300, 257
    counts = (rng.poisson(2.0, (rows, features))
              * (rng.random((rows, features)) < 0.3)).astype(numpy.float32)
    rates = rng.gamma(0.7, 2.0, (rows, features)).astype(numpy.float32)
    rates[rng.random((rows, features)) < 0.9] *= 1e-3
    csr = DeviceCSR.from_scipy(scipy.sparse.csr_matrix(counts), device)
    return csr, torch.from_numpy(rates).to(device), counts, rates


def test_evaluation_distributions_equal_the_host_path(cuda_device):
    from scvae_amd.analyses.distributions import evaluation_distributions
    csr, reconstructed, counts, rates = _case_300_257(cuda_device)
    n = counts.size
    for extensive in (False, True):
        got = evaluation_distributions(csr, reconstructed, kind="test",
                                       extensive=extensive)
        want = evaluation_distributions(csr, reconstructed, kind="test",
                                        extensive=extensive, on_device=False)
        assert len(got) == (6 if extensive else 3)
        _same_histograms(got, want)
    assert [h["name"] for h in got] == [
        "histogram-normed-counts", "histogram-normed-counts-log_values",
        "histogram-normed-count_sum", "histogram-normed-counts-test",
        "histogram-normed-counts-test-log_values",
        "histogram-normed-count_sum-test"]
    assert [int(h["counts"].sum()) for h in got] == [n, n, 300, n, n, 300]
    # the discrete rule: one bin per count over (-0.5, max + 0.5)
    assert len(got[3]["counts"]) == int(counts.max()) + 1
    assert numpy.array_equal(
        got[3]["counts"],
        numpy.bincount(counts.astype(numpy.int64).reshape(-1)))
    # with preprocessing the set is not discrete
    preprocessed = evaluation_distributions(
        csr, reconstructed, extensive=True, preprocessed=True)
    assert len(preprocessed[3]["counts"]) != len(got[3]["counts"])


def _tiny_set():
    from scvae_amd.data import DataSet
    rng = numpy.random.default_rng(23)
    n, features = 90, 37
    x = (rng.poisson(2.0, (n, features))
         * (rng.random((n, features)) < 0.5)).astype(numpy.float32)
    return DataSet("tiny", values=scipy.sparse.csr_matrix(x),
                   example_names=numpy.arange(n).astype(str),
                   feature_names=numpy.arange(features).astype(str),
                   kind="test")


def test_through_the_model(tmp_path, cuda_device):
    from scvae_amd.models import VariationalAutoencoder
    data_set = _tiny_set()
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
    assert not hasattr(plain[1], "distributions")
    n, features = 90, 37
    extensive = model.evaluate(data_set, distributions="extensive",
                               **arguments)
    assert numpy.array_equal(extensive[1].values, plain[1].values)
    histograms = extensive[1].distributions
    assert len(histograms) == 6 and extensive[1].distributions_duration > 0
    assert [int(h["counts"].sum()) for h in histograms] == [
        n * features, n * features, n, n * features, n * features, n]
    # the reconstruction's, against NumPy on the values that came back
    values = numpy.asarray(extensive[1].values, dtype=numpy.float32)
    flat = values.reshape(-1)
    want, want_edges = numpy.histogram(
        flat, bins="auto", range=numpy.array((flat.min(), flat.max())))
    assert same_bits(histograms[0]["edges"], want_edges)
    assert numpy.array_equal(histograms[0]["counts"], want)
    # the evaluation set's: its non-zeros plus the excess zeros
    stored = data_set.values.data
    assert histograms[3]["counts"][0] == (
        n * features - stored.size + int((stored == 0).sum()))
    assert histograms[3]["name"] == "histogram-normed-counts-test"
    for level in (True, "normal"):
        normal = model.evaluate(data_set, distributions=level, **arguments)
        assert len(normal[1].distributions) == 3
        for ours, theirs in zip(normal[1].distributions, histograms):
            assert numpy.array_equal(ours["counts"], theirs["counts"])
    with pytest.raises(ValueError, match="reconstructed"):
        model.evaluate(data_set, distributions=True,
                       output_versions=["latent"], **arguments)
    with pytest.raises(ValueError, match="`all` not found"):
        model.evaluate(data_set, distributions="all", **arguments)


def _files(directory):
    return sorted(os.path.relpath(os.path.join(root, name), directory)
                  for root, _, names in os.walk(directory) for name in names)


def test_through_the_command_line(tmp_path, cuda_device, monkeypatch, capsys):
    from scvae_amd import cli
    data_set = _tiny_set()
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
    arguments = dict(latent_size=3, hidden_sizes=[12], minibatch_size=32,
                     reconstruction_distribution="poisson",
                     models_directory="models",
                     analyses_directory="analyses")
    cli.train("tiny", number_of_epochs=1, **arguments)
    capsys.readouterr()
    cli.evaluate("tiny", sample_size=0, **arguments)
    plain = capsys.readouterr().out
    files_before = _files(tmp_path)
    assert "distributions for" not in plain
    assert "distribution plotted" not in plain
    assert not analyses.exists()
    results = cli.evaluate("tiny", sample_size=0, distributions=True,
                           analysis_level="extensive", **arguments)
    text = capsys.readouterr().out
    lines = text.splitlines()
    # every line of the plain run, in order, and the new ones after them
    new = [line for line in lines if "distributions for" in line
           or "distribution plotted" in line]
    assert len(new) == 6
    at = lines.index("Plotting distributions for reconstructed test set.")
    assert re.fullmatch(
        r"    Count distribution plotted and saved \(.+\)\.", lines[at + 1])
    assert re.fullmatch(
        r"    Count sum distribution plotted and saved \(.+\)\.",
        lines[at + 2])
    assert lines[at + 3] == ""
    assert lines[at + 4] == "Plotting distributions for test set."
    assert lines[at + 5].startswith("    Count distribution plotted")
    assert lines[at + 6].startswith("    Count sum distribution plotted")
    assert lines[at + 7] == ""
    # (durations and the figures of a sampled evaluation differ run to run)
    numbers = re.compile(r"[-+]?\d[\d.e+-]*( [a-z]+)?")
    assert [numbers.sub("#", line) for line in lines[:at] + lines[at + 8:]
            ] == [numbers.sub("#", line) for line in plain.splitlines()]
    histograms = results["end_of_training"][1].distributions
    written = [name for name in _files(tmp_path) if name not in files_before
               and name.startswith("analyses")]
    assert sorted(os.path.basename(name) for name in written) == sorted(
        h["name"] + ".tsv" for h in histograms)
    assert len(written) == 6
    assert all(os.path.basename(os.path.dirname(name)) == "histograms"
               for name in written)
    table = (tmp_path / written[0]).read_text().splitlines()
    assert table[0] == "bin_left\tbin_right\tcount\tfrequency"
    by_name = {h["name"]: h for h in histograms}
    histogram = by_name[os.path.basename(written[0])[:-4]]
    assert len(table) == 1 + len(histogram["counts"])
    assert [int(row.split("\t")[2]) for row in table[1:]] == (
        histogram["counts"].tolist())
    # normal level: three files' worth of lines
    cli.evaluate("tiny", sample_size=0, distributions=True, **arguments)
    lines = capsys.readouterr().out.splitlines()
    assert sum("distributions for" in line or "distribution plotted" in line
               for line in lines) == 3
