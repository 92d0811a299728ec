"""Distributions of data sets on the device: the histograms that
``analyse_distributions`` plots (``scvae/analyses/subanalyses.py:50-291``,
called for the reconstructed set at ``scvae/analyses/analyses.py:1226-1235``)
-- "counts", "counts, log values" and "count sum", each the
``numpy.histogram`` of ``plot_histogram``
(``scvae/analyses/figures/histograms.py:125-198``) -- as tables of edges,
counts and frequencies, from the kernels of ``csrc/histogram.hip``: an exact
histogram over NumPy's own edges, exact order statistics by radix select (for
the percentiles ``bins="auto"`` asks for) and fp64 row sums.  The values are
read where they lie; nothing of their size is allocated.

The bin rules are NumPy's (``numpy/lib/_histograms_impl.py`` of NumPy 2.2),
restated here so that they can be fed from the device's order statistics:

*   outer edges (``_get_outer_edges``, lines 303-330): ``range``, or the
    minimum and maximum of the values; both must be finite (314, 322); equal
    ones are widened by 0.5 either way (326-328).
*   ``bins="auto"`` (``_hist_bin_auto``, 229-269): the width is the smaller of
    the Freedman-Diaconis width ``2 IQR n**(-1/3)`` (199-226) and the Sturges
    width ``ptp / (log2 n + 1)`` (53-73), Sturges alone where the former
    is 0; ``ceil((last - first) / width)`` bins, one bin where the width is 0
    (410-418).  With a ``range`` NumPy first drops the values outside it
    (400-404): the device path takes such a call to the host.
*   IQR = ``percentile(75) - percentile(25)`` with the default "linear"
    method (``numpy/lib/_function_base_impl.py`` ``_quantile`` and
    ``_lerp``, 4639-4660): virtual index ``v = (n - 1) q / 100``,
    ``lo = floor(v)``, ``hi = min(lo + 1, n - 1)``, ``g = v - lo``; the
    difference ``d = x_hi - x_lo`` is formed in fp32 and the result in fp64,
    ``x_lo + d g``, replaced by ``x_hi - d (1 - g)`` where ``g >= 0.5``.
*   edges (440-456): ``numpy.linspace(first, last, bins + 1)`` in the result
    type of the outer edges and the values, taken from
    ``numpy.histogram_bin_edges`` itself, so that the bits are NumPy's.
*   counts (816-877): an element with ``e[0] <= x <= e[-1]`` belongs to the
    last bin ``i`` with ``e[i] <= x``, the last bin closed on the right.
    NumPy estimates the index and corrects it by one either way; the kernel
    corrects until the definition holds.

What differs from the reference on purpose: the count sums are fp64 sums of
each row rounded once to fp32 (the reference adds in fp32,
``data_set.py`` ``count_sum``); nothing is plotted; the histograms per class
(``subanalyses.py:194-289``: for a dense set every one of them is the
histogram of the whole set, ``subanalyses.py:234``), those with cut-offs
(``analyse_results`` passes no cut-offs) and the class histogram (a count of
labels on the host) are left out.
"""
import ctypes
import math
import operator
from time import time

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.kmeans import _ptr
from scvae_amd.utilities import normalise_string

#: ``histograms.py:27``
MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS = 20000
#: most bins of a histogram on the device (``scvae_histogram_accumulate``)
MAXIMUM_NUMBER_OF_BINS_ON_DEVICE = 1 << 20
#: most ranks of one ``scvae_order_statistics`` call
_MAXIMUM_RANKS = 4
_QUARTILES = (75, 25)          # in the order ``_hist_bin_fd`` asks for them


class _HostFallback(Exception):
    """The device path does not cover this call: the reason."""


# ---- the restated rules ----

def percentile_ranks(n, q):
    """``(lo, hi, g)`` of the "linear" percentile ``q`` of ``n`` values: the
    zero-based ranks of the two order statistics it interpolates between and
    the weight of the upper one."""
    virtual_index = (n - 1) * numpy.true_divide(q, 100)
    lo = int(math.floor(virtual_index))
    if lo >= n - 1:
        lo = hi = n - 1
    else:
        hi = lo + 1
    return lo, hi, numpy.float64(virtual_index - math.floor(virtual_index))


def percentile_from_order_statistics(x_lo, x_hi, g):
    """NumPy's ``_lerp`` for fp32 order statistics: the difference in fp32,
    the result in fp64."""
    x_lo, x_hi = numpy.float32(x_lo), numpy.float32(x_hi)
    g = numpy.float64(g)
    with numpy.errstate(invalid="ignore"):
        d = numpy.subtract(x_hi, x_lo)
        if d == 0:
            return numpy.float64(x_lo)
        if g >= 0.5:
            return numpy.float64(x_hi) - d * (1 - g)
        return numpy.float64(x_lo) + d * g


def outer_edges(minimum, maximum, range=None):
    """``_get_outer_edges``: NumPy scalars in, NumPy's errors out."""
    if range is not None:
        first_edge, last_edge = range
        if first_edge > last_edge:
            raise ValueError(
                "max must be larger than min in range parameter.")
        if not (numpy.isfinite(first_edge) and numpy.isfinite(last_edge)):
            raise ValueError(
                "supplied range of [{}, {}] is not finite".format(
                    first_edge, last_edge))
    else:
        first_edge, last_edge = minimum, maximum
        if not (numpy.isfinite(first_edge) and numpy.isfinite(last_edge)):
            raise ValueError(
                "autodetected range of [{}, {}] is not finite".format(
                    first_edge, last_edge))
    if first_edge == last_edge:
        first_edge = first_edge - 0.5
        last_edge = last_edge + 0.5
    return first_edge, last_edge


def _subtract(a, b):
    """``_unsigned_subtract`` for floating-point scalars."""
    return numpy.subtract(a, b, dtype=numpy.result_type(a, b))


def automatic_number_of_bins(n, minimum, maximum, first_edge, last_edge,
                             percentile_75, percentile_25):
    """``bins="auto"`` for ``n`` fp32 values, none of them outside the outer
    edges, from their extremes and quartiles."""
    peak_to_peak = _subtract(numpy.float32(maximum), numpy.float32(minimum))
    sturges_width = peak_to_peak / (numpy.log2(n) + 1.0)
    iqr = numpy.subtract(percentile_75, percentile_25)
    fd_width = 2.0 * iqr * n ** (-1.0 / 3.0)
    width = min(fd_width, sturges_width) if fd_width else sturges_width
    if width:
        return int(numpy.ceil(_subtract(last_edge, first_edge) / width))
    return 1


def bin_edges(number_of_bins, first_edge, last_edge, dtype=numpy.float32):
    """NumPy's own edges for ``number_of_bins`` equal bins of values of type
    ``dtype``."""
    return numpy.histogram_bin_edges(
        numpy.empty(0, dtype=dtype), bins=number_of_bins,
        range=(first_edge, last_edge))


def figure_name(names, normed=True, log_values=False):
    """``plot_histogram``'s figure name (``histograms.py:131-136, 163``
    through ``figures/saving.py:44-63``)."""
    name = "histogram" + ("-normed" if normed else "")
    names = [str(n) for n in names if n is not None]
    if names:
        name += "-" + "-".join(map(normalise_string, names))
    if log_values:
        name += "-log_values"
    return name


# ---- values ----

def _is_sparse(x):
    return hasattr(x, "tocsr") and not isinstance(x, numpy.ndarray)


def _is_device_csr(x):
    return hasattr(x, "indptr") and hasattr(x, "gather_dense")


def _device_of(device=None):
    device = torch.device(device if device is not None else "cuda:0")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _DeviceSeries:
    """fp32 values on the device as the kernels take them: ``[rows, F]`` with
    unit column stride and a row pitch, read in place."""

    def __init__(self, tensor):
        if tensor.dtype != torch.float32:
            raise ValueError("Distributions: float32 values expected, got "
                             "{}.".format(tensor.dtype))
        if tensor.dim() != 2:
            tensor = tensor.contiguous().view(1, -1)
        elif tensor.stride(1) != 1 and tensor.shape[1] > 1:
            tensor = tensor.contiguous()
        self.tensor = tensor
        self.rows, self.features = int(tensor.shape[0]), int(tensor.shape[1])
        self.pitch = (int(tensor.stride(0)) if self.rows > 1
                      else self.features)
        if self.rows > 1 and self.pitch < self.features:
            self.tensor = tensor = tensor.contiguous()
            self.pitch = self.features
        self.size = self.rows * self.features
        self.device = tensor.device
        self.lib = _lib.load()
        self._statistics = None

    def _stream(self):
        return ctypes.c_void_p(
            torch.cuda.current_stream(self.device).cuda_stream)

    def order_statistics(self, ranks, shift=False):
        """``(values fp32 [len(ranks)], minimum, maximum, NaN count)``."""
        ranks = [int(r) for r in ranks]
        values = []
        workspace = torch.empty(
            self.lib.scvae_order_statistics_workspace_bytes(),
            dtype=torch.uint8, device=self.device)
        extremes = torch.empty(2, dtype=torch.float32, device=self.device)
        counts = torch.empty(2, dtype=torch.int64, device=self.device)
        for first in range(0, max(len(ranks), 1), _MAXIMUM_RANKS):
            some = ranks[first:first + _MAXIMUM_RANKS] or [0]
            out = torch.empty(len(some), dtype=torch.float32,
                              device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.scvae_order_statistics(
                    _ptr(self.tensor), self.pitch, self.rows, self.features,
                    int(bool(shift)),
                    (ctypes.c_int64 * len(some))(*some), len(some),
                    _ptr(out), _ptr(extremes), _ptr(counts), _ptr(workspace),
                    workspace.numel(), self._stream()),
                    "scvae_order_statistics")
            values.append(out.cpu().numpy())
        values = numpy.concatenate(values)[:len(ranks)]
        minimum, maximum = extremes.cpu().numpy()
        return values, minimum, maximum, int(counts[1].item())

    def statistics(self):
        """``(minimum, maximum, the order statistics of the two quartiles)``
        of the unshifted values, from one radix select; the extremes are NaN
        where a value is, as NumPy's are."""
        if self._statistics is None:
            ranks = []
            for q in _QUARTILES:
                ranks.extend(percentile_ranks(self.size, q)[:2])
            values, minimum, maximum, nans = self.order_statistics(ranks)
            if nans:
                minimum = maximum = numpy.float32("nan")
            self._statistics = (minimum, maximum, values)
        return self._statistics

    def count(self, edges, shift=False, aggregate=True):
        """``(counts int64 [bins], below, above, NaN)`` over NumPy edges."""
        edges = numpy.ascontiguousarray(edges)
        if edges.dtype not in (numpy.float32, numpy.float64):
            edges = edges.astype(numpy.float64)
        number_of_bins = edges.size - 1
        device_edges = torch.from_numpy(edges).to(self.device)
        counts = torch.zeros(number_of_bins + 3, dtype=torch.int64,
                             device=self.device)
        flags = int(edges.dtype == numpy.float64) | (0 if aggregate else 2)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_histogram_accumulate(
                _ptr(self.tensor), self.pitch, self.rows, self.features,
                int(bool(shift)), _ptr(device_edges), flags, number_of_bins,
                _ptr(counts), _ptr(counts[number_of_bins:]), self._stream()),
                "scvae_histogram_accumulate")
        counts = counts.cpu().numpy()
        return (counts[:number_of_bins],) + tuple(
            int(c) for c in counts[number_of_bins:])

    def row_sums(self):
        out = torch.empty(self.rows, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_row_sums_f64(
                _ptr(self.tensor), self.pitch, self.rows, self.features, 0,
                _ptr(out), self._stream()), "scvae_row_sums_f64")
        return out


def _host_series(values):
    """The values as ``analyse_distributions`` takes them
    (``subanalyses.py:119-125``): the stored values of a sparse matrix, all
    values of a dense one, flat, fp32."""
    if isinstance(values, _DeviceSeries):
        values = values.tensor
    if _is_device_csr(values):
        values = values.values
    if isinstance(values, torch.Tensor):
        values = values.cpu().numpy()
    if _is_sparse(values):
        values = values.tocsr().data
    return numpy.asarray(values, dtype=numpy.float32).reshape(-1)


def _device_series(values, device=None):
    if isinstance(values, _DeviceSeries):
        return values
    if _is_device_csr(values):
        return _DeviceSeries(values.values)
    if isinstance(values, torch.Tensor):
        if not values.is_cuda:
            values = values.to(_device_of(device))
        return _DeviceSeries(values)
    return _DeviceSeries(torch.from_numpy(numpy.ascontiguousarray(
        _host_series(values))).to(_device_of(device)))


def _use_device(values, on_device):
    if on_device is None:
        return torch.cuda.is_available()
    if on_device and not torch.cuda.is_available():
        raise _lib.HipLibraryError(
            "No GPU visible: distributions on the device need one.")
    return bool(on_device)


def _size_of(values):
    if isinstance(values, _DeviceSeries):
        return values.size
    if _is_device_csr(values):
        return int(values.values.numel())
    if isinstance(values, torch.Tensor):
        return int(values.numel())
    if _is_sparse(values):
        return int(values.tocsr().data.size)
    return int(numpy.size(values))


# ---- public ----

def order_statistics(values, ranks, shift=False, device=None):
    """The ``ranks``-th smallest values (zero-based) of ``values`` (an fp32
    device tensor, read in place; a NumPy array; the stored values of a SciPy
    sparse matrix) as fp32, exact, by radix select on the device.  NaN orders
    last."""
    ranks = [operator.index(r) for r in numpy.atleast_1d(ranks)]
    series = _device_series(values, device)
    if series.size == 0:
        raise ValueError("Order statistics: no values.")
    for rank in ranks:
        if not 0 <= rank < series.size:
            raise ValueError("Rank {} outside [0, {}).".format(
                rank, series.size))
    return series.order_statistics(ranks, shift=shift)[0]


def percentile(values, q, shift=False, device=None):
    """``numpy.percentile(values, q)`` (the "linear" method) of fp32 values
    from the device's order statistics: fp64, bit for bit NumPy's."""
    series = _device_series(values, device)
    if series.size == 0:
        raise ValueError("Percentile: no values.")
    qs = numpy.atleast_1d(numpy.asarray(q, dtype=numpy.float64))
    if not numpy.all((qs >= 0) & (qs <= 100)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    ranks = []
    for one in qs:
        ranks.extend(percentile_ranks(series.size, one)[:2])
    found = series.order_statistics(ranks, shift=shift)[0]
    result = numpy.array([
        percentile_from_order_statistics(
            found[2 * i], found[2 * i + 1],
            percentile_ranks(series.size, one)[2])
        for i, one in enumerate(qs)], dtype=numpy.float64)
    return result[0] if numpy.ndim(q) == 0 else result


def _shifted(value):
    return numpy.float32(value) + numpy.float32(1)


def _device_histogram(values, bins, range, shift, device):
    series = _device_series(values, device)
    if series.size < 1:
        raise _HostFallback("no values")
    automatic = isinstance(bins, str)
    if automatic and bins != "auto":
        raise _HostFallback("only the estimator \"auto\" is built")
    minimum = maximum = None
    if automatic or range is None:
        minimum, maximum, quartile_values = series.statistics()
        if shift:
            minimum, maximum = _shifted(minimum), _shifted(maximum)
            quartile_values = quartile_values + numpy.float32(1)
    first_edge, last_edge = outer_edges(minimum, maximum, range)
    if automatic:
        if not (numpy.isfinite(minimum) and numpy.isfinite(maximum)):
            raise _HostFallback("values that are not finite")
        if range is not None and not (first_edge <= minimum
                                      and maximum <= last_edge):
            raise _HostFallback(
                "automatic bins with values outside the range")
        percentiles = [
            percentile_from_order_statistics(
                quartile_values[2 * i], quartile_values[2 * i + 1],
                percentile_ranks(series.size, q)[2])
            for i, q in enumerate(_QUARTILES)]
        number_of_bins = automatic_number_of_bins(
            series.size, minimum, maximum, first_edge, last_edge,
            *percentiles)
    else:
        number_of_bins = operator.index(bins)
        if number_of_bins < 1:
            raise ValueError("`bins` must be positive, when an integer")
    if number_of_bins > MAXIMUM_NUMBER_OF_BINS_ON_DEVICE:
        raise _HostFallback("{} bins, more than {}".format(
            number_of_bins, MAXIMUM_NUMBER_OF_BINS_ON_DEVICE))
    edges = bin_edges(number_of_bins, first_edge, last_edge)
    return series.count(edges, shift=shift)[0], edges


def histogram(values, bins=10, range=None, shift=False, excess_zero_count=0,
              on_device=None, device=None):
    """``numpy.histogram(values (+ 1 with shift), bins, range)`` as
    ``(counts int64, edges)``; ``excess_zero_count`` is added to the first
    bin (``histograms.py:173``).  ``values``: an fp32 device tensor (read in
    place, its row pitch honoured), a NumPy array, or a SciPy sparse matrix,
    which contributes its stored values.  ``bins``: an int or ``"auto"``.
    On the device the counts are exact over NumPy's own edges; without a GPU
    or with ``on_device=False`` the call is ``numpy.histogram`` itself."""
    if _use_device(values, on_device):
        try:
            counts, edges = _device_histogram(values, bins, range, shift,
                                              device)
        except _HostFallback as reason:
            print("distributions on the device not used: {}.".format(reason))
            counts = None
    else:
        counts = None
    if counts is None:
        series = _host_series(values)
        if shift:
            series = series + numpy.float32(1)
        counts, edges = numpy.histogram(series, bins=bins, range=range)
    counts = numpy.asarray(counts, dtype=numpy.int64).copy()
    counts[0] += int(excess_zero_count)
    return counts, edges


def _plot_histogram_bins(minimum, maximum, discrete):
    """``(bins, range)`` of ``plot_histogram`` (``histograms.py:144-154``)
    before any shift."""
    if discrete and maximum < MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS:
        return int(numpy.ceil(maximum)) + 1, numpy.array(
            (-0.5, maximum + 0.5))
    if maximum < MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS:
        bins = "auto"
    else:
        bins = MAXIMUM_NUMBER_OF_BINS_FOR_HISTOGRAMS
    return bins, numpy.array((minimum, maximum))


def _extremes(values, use_device, device):
    if use_device:
        series = _device_series(values, device)
        minimum, maximum, _ = series.statistics()
        return series, minimum, maximum
    series = _host_series(values)
    return series, series.min(), series.max()


def _plotted_histogram(values, names, excess_zero_count=0, discrete=False,
                       log_values=False, use_device=False, device=None,
                       extremes=None):
    """One ``plot_histogram(series, excess_zero_count, normed=True,
    discrete=discrete, x_scale="log" if log_values else "linear")`` as a
    dict."""
    time_start = time()
    series, minimum, maximum = extremes or _extremes(
        values, use_device, device)
    series_length = _size_of(series) + int(excess_zero_count)
    bins, bin_range = _plot_histogram_bins(minimum, maximum, discrete)
    if log_values:          # histograms.py:159-163
        bin_range += 1
    counts, edges = histogram(
        series, bins=bins, range=bin_range, shift=log_values,
        excess_zero_count=excess_zero_count, on_device=use_device,
        device=device)
    return {
        "name": figure_name(names, log_values=log_values),
        "edges": edges,
        "counts": counts,
        "frequencies": counts / series_length,
        "duration": time() - time_start,
    }


def _stored_values(values, use_device, device):
    """``(series, excess zero count, shape)`` of a set's values
    (``subanalyses.py:119-125``)."""
    if _is_device_csr(values):
        shape = tuple(int(s) for s in values.shape)
        stored = values.values
        excess = shape[0] * shape[1] - int(stored.numel())
    elif _is_sparse(values):
        values = values.tocsr()
        shape = tuple(int(s) for s in values.shape)
        stored = values.data
        excess = shape[0] * shape[1] - int(stored.size)
    else:
        shape = tuple(int(s) for s in values.shape)
        stored, excess = values, 0
    if _size_of(stored) == 0:
        raise ValueError("Distributions: no stored values.")
    return stored, excess, shape


def _count_sums(values, use_device, device):
    """The sums of the rows: fp64 sums rounded once to fp32."""
    if not use_device:
        if _is_device_csr(values) or isinstance(values, torch.Tensor):
            raise ValueError("Count sums on the host: host values expected.")
        sums = values.sum(axis=1, dtype=numpy.float64)
        return numpy.asarray(sums, dtype=numpy.float64).reshape(-1).astype(
            numpy.float32)
    if _is_sparse(values):
        from scvae_amd.minibatch import DeviceCSR
        values = DeviceCSR.from_scipy(values.tocsr(), _device_of(device))
    if _is_device_csr(values):
        from scvae_amd.analyses.summary import csr_blocks
        sums = torch.empty(values.shape[0], dtype=torch.float32,
                           device=values.device)
        first = 0
        for block in csr_blocks(values):
            last = first + block.shape[0]
            sums[first:last] = _DeviceSeries(block).row_sums()
            first = last
        return sums
    if not isinstance(values, torch.Tensor):
        values = torch.from_numpy(numpy.ascontiguousarray(
            values, dtype=numpy.float32)).to(_device_of(device))
    return _DeviceSeries(values).row_sums()


def distribution_histograms(values, name=None, discrete=False,
                            on_device=None, device=None):
    """The three histograms ``analyse_distributions`` plots for a set
    (``subanalyses.py:119-146, 173-192``): "counts" and "counts, log values"
    over its values (the stored ones of a sparse matrix, the rest as excess
    zeros of the first bin) and "count sum" over the sums of its rows.
    ``values``: ``[N, F]`` as an fp32 device tensor, a ``DeviceCSR``, a NumPy
    array or a SciPy sparse matrix; ``name``: the reference's
    ``data_set_name`` (the kind of an original set, None otherwise).  The bin
    rules are ``plot_histogram``'s (``histograms.py:142-171``): a discrete
    set with a maximum below 20 000 gets ``ceil(max) + 1`` bins over
    ``(-0.5, max + 0.5)``; otherwise ``"auto"`` below 20 000 and 20 000 bins
    from there on, over ``(min, max)``; the log variant adds 1 to values and
    range.  Returns a list of dicts: ``name``, ``edges``, ``counts``,
    ``frequencies`` (counts over the length of the series with its excess
    zeros, ``histograms.py:142, 178-179``) and ``duration``."""
    use_device = _use_device(values, on_device)
    if not use_device and (_is_device_csr(values)
                           or isinstance(values, torch.Tensor)):
        values = _to_host(values)
    stored, excess, _ = _stored_values(values, use_device, device)
    extremes = _extremes(stored, use_device, device)
    histograms = [
        _plotted_histogram(stored, ["counts", name], excess, discrete,
                           log_values, use_device, device, extremes)
        for log_values in (False, True)]
    time_start = time()
    sums = _count_sums(values, use_device, device)
    count_sum = _plotted_histogram(sums, ["count sum", name],
                                   use_device=use_device, device=device)
    count_sum["duration"] = time() - time_start
    histograms.append(count_sum)
    return histograms


def _to_host(values):
    """A device tensor or ``DeviceCSR`` as a NumPy array or SciPy matrix."""
    if _is_device_csr(values):
        import scipy.sparse
        return scipy.sparse.csr_matrix(
            (values.values.cpu().numpy(), values.indices.cpu().numpy(),
             values.indptr.cpu().numpy()),
            shape=tuple(int(s) for s in values.shape))
    return values.cpu().numpy()


def evaluation_distributions(csr, reconstructed, kind="test",
                             extensive=False, preprocessed=False,
                             on_device=None):
    """What ``ModelBase.evaluate`` attaches: the histograms of the
    reconstructed set (``analyses.py:1226-1235``; not discrete, version
    "reconstructed", so no name) from ``reconstructed`` (``[N, F]`` fp32 on
    the device, read in place), and with ``extensive`` those of the
    evaluation set as ``analyse_data`` treats it (``analyses.py:60-300``,
    ``subanalyses.py:119-146, 173-192``): the stored values of the
    ``DeviceCSR`` with the excess zero count, discrete where its values are
    integer counts and no preprocessing is applied, named after the kind."""
    histograms = distribution_histograms(reconstructed, on_device=on_device)
    if extensive:
        discrete = bool(getattr(csr, "integer_counts", False)
                        and not preprocessed)
        histograms += distribution_histograms(
            csr, name=kind, discrete=discrete, on_device=on_device)
    return histograms


def write_histogram(path, histogram_dict):
    """One histogram as a tab-separated table: ``bin_left``, ``bin_right``,
    ``count``, ``frequency``."""
    import os
    os.makedirs(os.path.dirname(path), exist_ok=True)
    edges = histogram_dict["edges"]
    with open(path, "w") as file:
        file.write("bin_left\tbin_right\tcount\tfrequency\n")
        for i, (count, frequency) in enumerate(zip(
                histogram_dict["counts"], histogram_dict["frequencies"])):
            file.write("{}\t{}\t{}\t{}\n".format(
                repr(float(edges[i])), repr(float(edges[i + 1])),
                int(count), repr(float(frequency))))
