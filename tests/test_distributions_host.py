"""The bin rules and the percentile formula that
``scvae_amd/analyses/distributions.py`` restates, against the installed
NumPy, and its host path against a straight transcription of
``plot_histogram`` (``scvae/analyses/figures/histograms.py:142-179``).  No
GPU: the order statistics come from ``numpy.sort`` here, from the radix
select on the device (``tests/test_gpu_distributions.py``)."""
import numpy
import pytest
import scipy.sparse

from scvae_amd.analyses import distributions as D

SIZES = (2, 3, 4, 5, 7, 64, 65, 257, 1000, 5000)
KINDS = ("gamma", "zero-heavy", "log-normal")


def series_of(kind, n, seed):
    rng = numpy.random.default_rng(seed)
    if kind == "gamma":
        x = rng.gamma(0.7, 2.0, n)
    elif kind == "zero-heavy":
        x = rng.gamma(0.5, 3.0, n) * (rng.random(n) < 0.05)
    else:
        x = rng.lognormal(1.0, 2.0, n)
    return x.astype(numpy.float32)


def all_series():
    for k, kind in enumerate(KINDS):
        for n in SIZES:
            for shift in (False, True):
                x = series_of(kind, n, 100 * k + n)
                yield kind, n, shift, x + numpy.float32(1) if shift else x


def same_bits(a, b):
    a, b = numpy.asarray(a), numpy.asarray(b)
    return (a.dtype == b.dtype and a.shape == b.shape
            and a.tobytes() == b.tobytes())


def restated_percentile(x, q):
    ordered = numpy.sort(x)
    lo, hi, g = D.percentile_ranks(x.size, q)
    return D.percentile_from_order_statistics(ordered[lo], ordered[hi], g)


def test_percentile_formula():
    for kind, n, shift, x in all_series():
        for q in (25, 75, 0, 100, 50, 12.5, 99.9):
            got = restated_percentile(x, q)
            # (q as an array, which is how ``_hist_bin_fd`` asks: fp64; a
            #  scalar q makes NumPy interpolate in fp32)
            want = numpy.percentile(x, [q])[0]
            assert same_bits(got, want), (kind, n, shift, q, got, want)
        got = [restated_percentile(x, q) for q in (75, 25)]
        assert same_bits(numpy.array(got), numpy.percentile(x, [75, 25]))


def test_percentile_with_ties_and_negative_values():
    rng = numpy.random.default_rng(3)
    for n in (2, 9, 1000):
        for x in (rng.poisson(1.0, n).astype(numpy.float32),
                  rng.normal(0, 3, n).astype(numpy.float32),
                  numpy.full(n, 2.5, dtype=numpy.float32)):
            for q in (25, 75, 33):
                assert same_bits(restated_percentile(x, q),
                                 numpy.percentile(x, [q])[0])


def restated_edges(x, bins, range=None):
    first, last = D.outer_edges(x.min(), x.max(), range)
    if bins == "auto":
        bins = D.automatic_number_of_bins(
            x.size, x.min(), x.max(), first, last,
            restated_percentile(x, 75), restated_percentile(x, 25))
    return D.bin_edges(bins, first, last)


def test_automatic_bins_and_edges():
    for kind, n, shift, x in all_series():
        want = numpy.histogram_bin_edges(x, bins="auto")
        assert same_bits(restated_edges(x, "auto"), want), (kind, n, shift)
        # with the range plot_histogram passes: an array of the extremes
        bin_range = numpy.array((x.min(), x.max()))
        want = numpy.histogram_bin_edges(x, bins="auto", range=bin_range)
        assert same_bits(restated_edges(x, "auto", bin_range), want)
        for bins in (1, 7, 20000):
            assert same_bits(restated_edges(x, bins),
                             numpy.histogram_bin_edges(x, bins=bins))


def test_outer_edges():
    x = numpy.full(5, 3.0, dtype=numpy.float32)
    assert same_bits(restated_edges(x, 4), numpy.histogram_bin_edges(x, 4))
    assert same_bits(restated_edges(x, "auto"),
                     numpy.histogram_bin_edges(x, "auto"))
    # the discrete rule's range: fp64 edges for fp32 values
    bin_range = numpy.array((-0.5, x.max() + 0.5))
    edges = restated_edges(x, 4, bin_range)
    assert same_bits(edges, numpy.histogram_bin_edges(x, 4, bin_range))
    assert edges.dtype == bin_range.dtype
    for bad in (numpy.array([1.0, numpy.nan], dtype=numpy.float32),
                numpy.array([1.0, numpy.inf], dtype=numpy.float32)):
        for call in (lambda: numpy.histogram_bin_edges(bad, 3),
                     lambda: restated_edges(bad, 3)):
            with pytest.raises(ValueError, match="is not finite"):
                call()
    with pytest.raises(ValueError) as ours:
        restated_edges(bad, 3)
    with pytest.raises(ValueError) as theirs:
        numpy.histogram_bin_edges(bad, 3)
    assert str(ours.value) == str(theirs.value)
    with pytest.raises(ValueError, match="max must be larger than min"):
        D.outer_edges(None, None, (2.0, 1.0))
    tiny = numpy.array([1.0, numpy.nextafter(numpy.float32(1), 2)],
                       dtype=numpy.float32)
    with pytest.raises(ValueError, match="Too many bins for data range"):
        restated_edges(tiny, 5)


def test_histogram_host_path_is_numpy():
    for kind, n, shift, _ in all_series():
        x = series_of(kind, n, 7)
        shifted = x + numpy.float32(1) if shift else x
        for bins in ("auto", 10):
            counts, edges = D.histogram(x, bins=bins, shift=shift,
                                        excess_zero_count=5, on_device=False)
            want, want_edges = numpy.histogram(shifted, bins=bins)
            want = want.astype(numpy.int64)
            want[0] += 5
            assert counts.dtype == numpy.int64
            assert numpy.array_equal(counts, want)
            assert same_bits(edges, want_edges)
    sparse = scipy.sparse.random(30, 40, density=0.2, format="csr",
                                 dtype=numpy.float32, random_state=1)
    counts, _ = D.histogram(sparse, bins=6, on_device=False)
    assert counts.sum() == sparse.data.size


# histograms.py:142-179, as it stands there but for the figure
MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS = 20000


def transcribed_plot_histogram(series, excess_zero_count=0, normed=False,
                               discrete=False, x_scale="linear"):
    series = series.copy()
    series_length = len(series) + excess_zero_count
    series_max = series.max()
    if discrete and series_max < MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS:
        number_of_bins = int(numpy.ceil(series_max)) + 1
        bin_range = numpy.array((-0.5, series_max + 0.5))
    else:
        if series_max < MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS:
            number_of_bins = "auto"
        else:
            number_of_bins = MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS
        bin_range = numpy.array((series.min(), series_max))
    if x_scale == "log":
        series += 1
        bin_range += 1
    histogram, bin_edges = numpy.histogram(
        series, bins=number_of_bins, range=bin_range)
    histogram[0] += excess_zero_count
    if normed:
        histogram = histogram / series_length
    return histogram, bin_edges


def transcribed_histograms(values, discrete):
    """``analyse_distributions`` (``subanalyses.py:119-146, 173-192``) with
    the count sums this build takes: fp64 row sums rounded to fp32."""
    if scipy.sparse.issparse(values):
        series = values.data
        excess_zero_count = values.shape[0] * values.shape[1] - series.size
    else:
        series = values.reshape(-1)
        excess_zero_count = 0
    results = [
        transcribed_plot_histogram(series, excess_zero_count, normed=True,
                                   discrete=discrete, x_scale=x_scale)
        for x_scale in ("linear", "log")]
    count_sum = numpy.asarray(values.sum(axis=1, dtype=numpy.float64)
                              ).reshape(-1).astype(numpy.float32)
    results.append(transcribed_plot_histogram(count_sum, normed=True))
    return results


def small_sets():
    rng = numpy.random.default_rng(41)
    counts = (rng.poisson(2.0, (90, 37))
              * (rng.random((90, 37)) < 0.4)).astype(numpy.float32)
    rates = rng.gamma(0.7, 2.0, (90, 37)).astype(numpy.float32)
    large = counts.copy()
    large[3, 5] = 25000.0          # at 20 000 and above: 20 000 bins
    return (("dense", rates, False), ("sparse", scipy.sparse.csr_matrix(counts),
                                      True),
            ("sparse, not discrete", scipy.sparse.csr_matrix(counts), False),
            ("dense counts", counts, True),
            ("large", scipy.sparse.csr_matrix(large), True))


def test_three_histograms_against_the_transcription():
    for label, values, discrete in small_sets():
        got = D.distribution_histograms(values, name="test",
                                        discrete=discrete, on_device=False)
        want = transcribed_histograms(values, discrete)
        assert len(got) == 3
        n = values.shape[0] * values.shape[1]
        for histogram, (frequencies, edges), length in zip(
                got, want, (n, n, values.shape[0])):
            assert same_bits(histogram["edges"], edges), label
            assert same_bits(histogram["frequencies"], frequencies), label
            assert histogram["counts"].dtype == numpy.int64
            assert histogram["counts"].sum() == length
            assert histogram["duration"] >= 0
    assert len(got[0]["counts"]) == 20000     # the last set: "large"


def test_names_and_files(tmp_path):
    _, values, discrete = small_sets()[1]
    reconstructed = D.distribution_histograms(
        numpy.asarray(values.todense()), on_device=False)
    assert [h["name"] for h in reconstructed] == [
        "histogram-normed-counts", "histogram-normed-counts-log_values",
        "histogram-normed-count_sum"]
    original = D.distribution_histograms(values, name="test",
                                         discrete=True, on_device=False)
    assert [h["name"] for h in original] == [
        "histogram-normed-counts-test",
        "histogram-normed-counts-test-log_values",
        "histogram-normed-count_sum-test"]
    assert D.figure_name(["counts", "training"], normed=False) == (
        "histogram-counts-training")
    path = tmp_path / "histograms" / (original[0]["name"] + ".tsv")
    D.write_histogram(str(path), original[0])
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["bin_left", "bin_right", "count",
                                    "frequency"]
    assert len(lines) == 1 + len(original[0]["counts"])
    for line, left, right, count, frequency in zip(
            lines[1:], original[0]["edges"][:-1], original[0]["edges"][1:],
            original[0]["counts"], original[0]["frequencies"]):
        fields = line.split("\t")
        assert float(fields[0]) == left and float(fields[1]) == right
        assert int(fields[2]) == count and float(fields[3]) == frequency


def test_fallback_line_without_a_device(capsys):
    """The reasons a call leaves the device path are decided before any
    kernel runs; without a GPU the host path is taken silently."""
    x = series_of("gamma", 100, 1)
    D.histogram(x, bins=5, on_device=False)
    assert capsys.readouterr().out == ""
