"""The kernels of ``csrc/histogram.hip`` through the C ABI: exact integer
equality with NumPy oracles everywhere.

*   ``scvae_histogram_accumulate`` against ``numpy.searchsorted(edges, x,
    "right") - 1`` in fp64 with the last edge folded into the last bin, which
    is the entry's definition word for word.
*   ``scvae_order_statistics`` against ``numpy.sort``, and bit for bit against
    a sort of the order-preserving keys (-0.0 before +0.0).
*   ``scvae_row_sums_f64``: any order of F - 1 fp64 additions is within
    ``(F - 1) u sum |x|`` of the exact sum (u = 2^-53, first order; the bound
    below takes F + 1), so the fp32 result lies between the fp32 roundings of
    the two ends of that interval around ``math.fsum``: it is the rounding of
    the exact sum or its neighbour.
"""
import ctypes
import math

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu

#: csrc/histogram.hip: bins of a slab
S = 8192
ROWS = (1, 2, 63, 300)
FEATURES = (1, 3, 63, 64, 65, 257, 1031)
#: (pad of the pitch, offset of the base) in elements, the four layouts of
#: the reconstruction in tests/test_gpu_summary.py
LAYOUTS = ((0, 0), (3, 1), (1, 1), (5, 0))
BINS = (1, 2, 255, S - 1, S, S + 1, 2 * S + 3, 20000)
U = 2.0 ** -53


def placed(values, pad, offset, device):
    """``values`` on the device as a matrix of pitch F + pad whose base lies
    ``offset`` elements into a 256-byte aligned buffer; everything around the
    values is NaN, so a read outside them shows in every result."""
    rows, features = values.shape
    pitch = features + pad
    buffer = torch.full((offset + rows * pitch + 8,), float("nan"),
                        device=device)
    view = buffer[offset:offset + rows * pitch].view(rows, pitch)[:, :features]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() == buffer.data_ptr() + 4 * offset
    return view


def _pitch(view):
    return view.stride(0) if view.shape[0] > 1 else view.shape[1]


def _p(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


def device_histogram(view, edges, shift=0, into=None, aggregate=True):
    """``(counts [bins] int64, outside [3] int64)`` as NumPy, and the device
    tensor the call added to."""
    from scvae_amd import _lib
    lib = _lib.load()
    bins = edges.size - 1
    device_edges = torch.from_numpy(numpy.ascontiguousarray(edges)).to(
        view.device)
    cells = into if into is not None else torch.zeros(
        bins + 3, dtype=torch.int64, device=view.device)
    flags = int(edges.dtype == numpy.float64) | (0 if aggregate else 2)
    _lib.check(lib.scvae_histogram_accumulate(
        _p(view), _pitch(view), view.shape[0], view.shape[1], shift,
        _p(device_edges), flags, bins, _p(cells), _p(cells[bins:]), None),
        "scvae_histogram_accumulate")
    host = cells.cpu().numpy()
    return host[:bins], host[bins:], cells


def histogram_oracle(x, edges, shift=0):
    x = numpy.asarray(x, dtype=numpy.float32).reshape(-1)
    if shift:
        x = x + numpy.float32(1)
    x = x.astype(numpy.float64)
    e = edges.astype(numpy.float64)
    bins = e.size - 1
    nan = numpy.isnan(x)
    with numpy.errstate(invalid="ignore"):
        below, above = x < e[0], x > e[-1]
    inside = ~(nan | below | above)
    index = numpy.searchsorted(e, x[inside], "right") - 1
    index = numpy.minimum(index, bins - 1)
    return (numpy.bincount(index, minlength=bins).astype(numpy.int64),
            numpy.array([below.sum(), above.sum(), nan.sum()],
                        dtype=numpy.int64))


def uniform_edges(bins, first, last, dtype=numpy.float32):
    """NumPy's own edges, fp32 or (as for the discrete rule) fp64."""
    bin_range = numpy.array((first, last), dtype=dtype)
    edges = numpy.histogram_bin_edges(
        numpy.empty(0, dtype=numpy.float32), bins=bins, range=bin_range)
    assert edges.dtype == dtype
    return edges


def hard_values(edges, n, seed):
    """``n`` fp32 values: every edge itself (rounded to fp32) and the fp32
    neighbours on both sides of it, values below and above the range, NaN,
    and uniform values across the range -- as many of the first kinds as
    fit, in random places."""
    rng = numpy.random.default_rng(seed)
    at = edges.astype(numpy.float32)
    low, high = numpy.float32(-numpy.inf), numpy.float32(numpy.inf)
    span = float(edges[-1]) - float(edges[0])
    pool = numpy.concatenate([
        at, numpy.nextafter(at, low), numpy.nextafter(at, high),
        numpy.array([edges[0] - 1 - span, edges[-1] + 1 + span, numpy.nan,
                     -numpy.inf, numpy.inf], dtype=numpy.float32)])
    values = rng.uniform(float(edges[0]), float(edges[-1]), n).astype(
        numpy.float32)
    take = min(n, pool.size)
    where = rng.choice(n, take, replace=False)
    values[where] = rng.permutation(pool)[:take] if take < pool.size else pool
    return values


def check(view, host, edges, shift=0):
    counts, outside, _ = device_histogram(view, edges, shift)
    want_counts, want_outside = histogram_oracle(host, edges, shift)
    assert numpy.array_equal(outside, want_outside), (outside, want_outside)
    assert numpy.array_equal(counts, want_counts), numpy.flatnonzero(
        counts != want_counts)[:8]
    assert counts.sum() + outside.sum() == host.size


@pytest.mark.parametrize("features", FEATURES)
def test_histogram_shapes_and_pitches(cuda_device, features):
    for rows in ROWS:
        for k, (pad, offset) in enumerate(LAYOUTS):
            for bins, dtype in ((2, numpy.float32), (255, numpy.float64),
                                (S + 1, numpy.float32)):
                edges = uniform_edges(bins, -0.5, 37.5, dtype)
                host = hard_values(edges, rows * features,
                                   1000 * rows + features + k).reshape(
                                       rows, features)
                check(placed(host, pad, offset, cuda_device), host, edges)


@pytest.mark.parametrize("bins", BINS)
def test_histogram_every_edge_and_its_neighbours(cuda_device, bins):
    """300 x 1031 values hold every edge and the fp32 values next to it on
    both sides, for fp32 edges, fp64 edges (the discrete rule's), and edges
    whose width is a few ulp of their magnitude."""
    rows, features = 300, 1031
    cases = [uniform_edges(bins, 0.0, 11.75),
             uniform_edges(bins, -0.5, bins - 0.5, numpy.float64),
             uniform_edges(bins, -3.25, 1e4, numpy.float64),
             uniform_edges(bins, 1.0, 1.0 + bins * 2.0 ** -21)]
    for k, edges in enumerate(cases):
        assert 3 * edges.size + 5 <= rows * features
        host = hard_values(edges, rows * features, bins + k).reshape(
            rows, features)
        check(placed(host, 3, 1, cuda_device), host, edges)


def test_histogram_extremes_and_equal_values(cuda_device):
    rng = numpy.random.default_rng(2)
    host = rng.gamma(0.7, 2.0, (63, 257)).astype(numpy.float32)
    # edges from the extremes: the maximum lies on the last edge
    for bins in (1, 7, 255, S + 1):
        edges = numpy.histogram_bin_edges(host, bins=bins)
        counts, outside, _ = device_histogram(
            placed(host, 1, 1, cuda_device), edges)
        assert numpy.array_equal(counts, numpy.histogram(host, bins)[0])
        assert counts[-1] >= 1 and not outside.any()
    # all elements equal: NumPy widens the range by 0.5 either way
    equal = numpy.full((63, 65), 2.5, dtype=numpy.float32)
    for bins in (1, 2, 5, 255):
        want, edges = numpy.histogram(equal, bins)
        counts, outside, _ = device_histogram(
            placed(equal, 0, 0, cuda_device), edges)
        assert numpy.array_equal(counts, want) and not outside.any()


def test_histogram_one_bin_and_zero_heavy(cuda_device):
    """All elements in one bin, and 95 % zeros: what the aggregation inside a
    wave is for; with it switched off the counts are the same."""
    rng = numpy.random.default_rng(3)
    rows, features = 300, 257
    narrow = rng.uniform(5.0, 5.001, (rows, features)).astype(numpy.float32)
    zeros = (rng.gamma(0.5, 3.0, (rows, features))
             * (rng.random((rows, features)) < 0.05)).astype(numpy.float32)
    two = numpy.where(rng.random((rows, features)) < 0.6, 0.0, 1.0).astype(
        numpy.float32)
    for host in (narrow, zeros, two):
        for bins in (3, 255, S + 1, 20000):
            edges = uniform_edges(bins, 0.0, float(host.max()))
            view = placed(host, 3, 1, cuda_device)
            check(view, host, edges)
            with_aggregation = device_histogram(view, edges)[0]
            without = device_histogram(view, edges, aggregate=False)[0]
            assert numpy.array_equal(with_aggregation, without)


def test_histogram_repeated_edges(cuda_device):
    rng = numpy.random.default_rng(4)
    base = numpy.linspace(0.0, 8.0, 33)
    cases = [numpy.repeat(base, 2), numpy.repeat(base, 5)[2:],
             numpy.concatenate([[0.0] * 4, base, [8.0] * 3]),
             numpy.full(7, 2.0), numpy.full(S + 5, 2.0),
             numpy.concatenate([numpy.full(S - 1, 1.0), [1.0, 1.5, 2.0, 2.0]])]
    for k, edges in enumerate(cases):
        for dtype in (numpy.float32, numpy.float64):
            edges = numpy.ascontiguousarray(edges, dtype=dtype)
            host = hard_values(edges, 63 * 257, k).reshape(63, 257)
            check(placed(host, 1, 1, cuda_device), host, edges)


def test_histogram_shift(cuda_device):
    """``fl32(x + 1)``: values below 2^-24 round to 1, 3 x 2^-25 rounds up,
    2^24 + 1 is a tie, -1 gives 0, -0.0 gives +1."""
    special = numpy.array(
        [0.0, -0.0, 1e-9, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25,
         2.0 ** -23, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 24 - 1, -1.0, -2.0,
         0.5, numpy.nan], dtype=numpy.float32)
    rng = numpy.random.default_rng(5)
    host = rng.gamma(0.7, 2.0, (63, 257)).astype(numpy.float32)
    flat = host.reshape(-1)
    flat[rng.choice(flat.size, 20 * special.size, replace=False)] = (
        numpy.tile(special, 20))
    one = numpy.float32(1)
    up = numpy.nextafter(one, numpy.float32(2))
    cases = [numpy.array([0.0, 1.0, up, 2.0, 2.0 ** 24, 2.0 ** 25],
                         dtype=numpy.float32),
             numpy.array([1.0, up], dtype=numpy.float32),
             uniform_edges(255, 1.0, 20.0),
             uniform_edges(S + 1, 0.5, 2.0 ** 24 + 2, numpy.float64)]
    for edges in cases:
        view = placed(host, 3, 1, cuda_device)
        check(view, host, edges, shift=1)
        shifted = device_histogram(view, edges, shift=1)[0]
        plain = device_histogram(view, edges, shift=0)[0]
        assert not numpy.array_equal(shifted, plain)


def test_histogram_accumulates_and_is_the_same_for_every_geometry(
        cuda_device):
    """Two calls into one ``counts`` add up; the rows in one call, in pieces
    and in another layout give the same bits, run after run."""
    rows, features = 300, 257
    edges = uniform_edges(S + 1, 0.0, 30.0)
    host = hard_values(edges, rows * features, 6).reshape(rows, features)
    view = placed(host, 3, 1, cuda_device)
    counts, outside, cells = device_histogram(view, edges)
    twice = device_histogram(view, edges, into=cells)
    assert numpy.array_equal(twice[0], 2 * counts)
    assert numpy.array_equal(twice[1], 2 * outside)
    cells = None
    for first, last in ((0, 1), (1, 8), (8, 200), (200, rows)):
        pieces = device_histogram(view[first:last], edges, into=cells)
        cells = pieces[2]
    assert numpy.array_equal(pieces[0], counts)
    assert numpy.array_equal(pieces[1], outside)
    flat = placed(host.reshape(1, -1), 0, 1, cuda_device)
    for _ in range(2):
        again = device_histogram(flat, edges)
        assert numpy.array_equal(again[0], counts)
        assert numpy.array_equal(again[1], outside)


# ---- order statistics ----

def device_order_statistics(view, ranks, shift=0):
    """``(values fp32 [len(ranks)], minimum, maximum, n, NaN count)``."""
    from scvae_amd import _lib
    lib = _lib.load()
    device = view.device
    workspace = torch.empty(lib.scvae_order_statistics_workspace_bytes(),
                            dtype=torch.uint8, device=device)
    extremes = torch.empty(2, dtype=torch.float32, device=device)
    counts = torch.empty(2, dtype=torch.int64, device=device)
    values = []
    for first in range(0, len(ranks), 4):
        some = [int(r) for r in ranks[first:first + 4]]
        out = torch.empty(len(some), dtype=torch.float32, device=device)
        _lib.check(lib.scvae_order_statistics(
            _p(view), _pitch(view), view.shape[0], view.shape[1], shift,
            (ctypes.c_int64 * len(some))(*some), len(some), _p(out),
            _p(extremes), _p(counts), _p(workspace), workspace.numel(),
            None), "scvae_order_statistics")
        values.append(out.cpu().numpy())
    extremes, counts = extremes.cpu().numpy(), counts.cpu().numpy()
    return (numpy.concatenate(values), extremes[0], extremes[1],
            int(counts[0]), int(counts[1]))


def keys_of(x):
    bits = numpy.ascontiguousarray(x, dtype=numpy.float32).view(numpy.uint32)
    return numpy.where(bits & 0x80000000, ~bits, bits | 0x80000000).astype(
        numpy.uint32)


def values_of(keys):
    keys = numpy.asarray(keys, dtype=numpy.uint32)
    return numpy.where(keys & 0x80000000, keys ^ 0x80000000, ~keys).astype(
        numpy.uint32).view(numpy.float32)


def sorted_by_key(x):
    """The kernel's order: ``numpy.sort`` but for -0.0 before +0.0."""
    x = numpy.asarray(x, dtype=numpy.float32).reshape(-1)
    x = x[~numpy.isnan(x)]
    return values_of(numpy.sort(keys_of(x)))


def ranks_of(n):
    from scvae_amd.analyses.distributions import percentile_ranks
    ranks = [0, n - 1]
    for q in (25, 75):
        ranks.extend(percentile_ranks(n, q)[:2])
    return ranks


def check_order_statistics(view, host, ranks=None, shift=0):
    host = numpy.asarray(host, dtype=numpy.float32).reshape(-1)
    ranks = ranks_of(host.size) if ranks is None else ranks
    got, lo, hi, n, nans = device_order_statistics(view, ranks, shift)
    want = sorted_by_key(host)
    assert numpy.array_equal(want, numpy.sort(host[~numpy.isnan(host)]))
    if shift:
        want = want + numpy.float32(1)
    assert n == host.size and nans == int(numpy.isnan(host).sum())
    picked = want[ranks]
    assert numpy.array_equal(got.view(numpy.uint32),
                             picked.view(numpy.uint32)), (got, picked)
    assert numpy.array_equal(
        numpy.array([lo, hi]).view(numpy.uint32),
        numpy.array([want[0], want[-1]]).view(numpy.uint32))


def order_data(n, kind, seed):
    rng = numpy.random.default_rng(seed)
    if kind == "poisson":             # heavy ties
        return rng.poisson(1.3, n).astype(numpy.float32)
    if kind == "normal":              # negative values
        return rng.normal(0.0, 50.0, n).astype(numpy.float32)
    # zero-heavy rates
    return (rng.gamma(0.5, 3.0, n) * (rng.random(n) < 0.3)).astype(
        numpy.float32)


@pytest.mark.parametrize("n", (1, 2, 3, 64, 65, 4097))
def test_order_statistics_sizes(cuda_device, n):
    for k, kind in enumerate(("poisson", "normal", "rates")):
        host = order_data(n, kind, 10 * n + k).reshape(1, n)
        for pad, offset in LAYOUTS:
            check_order_statistics(placed(host, pad, offset, cuda_device),
                                   host)
        check_order_statistics(placed(host, 0, 1, cuda_device), host,
                               shift=1)


def test_order_statistics_matrix(cuda_device):
    rows, features = 300, 1031
    n = rows * features
    for k, kind in enumerate(("poisson", "normal", "rates")):
        host = order_data(n, kind, k).reshape(rows, features)
        for pad, offset in LAYOUTS:
            check_order_statistics(placed(host, pad, offset, cuda_device),
                                   host)
        spread = [n // 7, n // 3, n // 2, n - 2]
        check_order_statistics(placed(host, 3, 1, cuda_device), host, spread,
                               shift=1)
    for rows, features in ((2, 65), (63, 257), (63, 3)):
        host = order_data(rows * features, "normal", 9).reshape(
            rows, features)
        check_order_statistics(placed(host, 5, 0, cuda_device), host)


def test_order_statistics_zeros_and_nan(cuda_device):
    """-0.0 orders before +0.0; NaN orders last and is counted apart."""
    host = numpy.array([[0.0, -0.0, 1.0, -0.0, -1.0, 0.0, numpy.nan, 2.0,
                         numpy.nan, -numpy.inf, numpy.inf]],
                       dtype=numpy.float32)
    view = placed(host, 0, 1, cuda_device)
    got, lo, hi, n, nans = device_order_statistics(
        view, list(range(host.size)))
    assert n == 11 and nans == 2
    assert lo == -numpy.inf and hi == numpy.inf
    want = numpy.array([-numpy.inf, -1.0, -0.0, -0.0, 0.0, 0.0, 1.0, 2.0,
                        numpy.inf, numpy.nan, numpy.nan],
                       dtype=numpy.float32)
    assert numpy.array_equal(got[:9].view(numpy.uint32),
                             want[:9].view(numpy.uint32))
    assert numpy.isnan(got[9:]).all()
    # a -0.0 among many zeros: rank 0 is it, every other rank a +0.0 or more
    rates = order_data(4097, "rates", 1)
    zeros = numpy.flatnonzero(rates == 0)
    rates[zeros[len(zeros) // 2]] = -0.0
    check_order_statistics(placed(rates.reshape(1, -1), 0, 0, cuda_device),
                           rates)
    only_nan = numpy.full((1, 70), numpy.nan, dtype=numpy.float32)
    got, lo, hi, n, nans = device_order_statistics(
        placed(only_nan, 0, 0, cuda_device), [0, 69])
    assert numpy.isnan(got).all() and numpy.isnan(lo) and numpy.isnan(hi)
    assert n == 70 and nans == 70


def test_order_statistics_keys_that_differ_in_one_digit(cuda_device):
    """Keys that differ only in the digit of one radix pass (bits 31-21,
    20-10, 9-0), every value once, in random order."""
    rng = numpy.random.default_rng(8)
    base = int(keys_of(numpy.array([3.1415927]))[0])
    sets = [
        (base & ~0x3FF) | numpy.arange(1 << 10, dtype=numpy.uint32),
        (base & ~(0x7FF << 10)) | (numpy.arange(1 << 11, dtype=numpy.uint32)
                                   << 10),
        (base & 0x1FFFFF) | (numpy.arange(1 << 11, dtype=numpy.uint32)
                             << 21)]
    for keys in sets:
        host = values_of(keys.astype(numpy.uint32))
        host = rng.permutation(host[numpy.isfinite(host)]).reshape(1, -1)
        n = host.size
        assert n >= 1000 and numpy.unique(host).size == n
        ranks = [0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1, 511]
        check_order_statistics(placed(host, 0, 1, cuda_device), host, ranks)
        # ... and each of them many times: ties inside every digit
        many = numpy.repeat(host, 3, axis=0)
        check_order_statistics(placed(many, 1, 0, cuda_device), many)


# ---- row sums ----

def device_row_sums(view, shift=0):
    from scvae_amd import _lib
    lib = _lib.load()
    out = torch.full((view.shape[0] + 2,), float("nan"), device=view.device)
    _lib.check(lib.scvae_row_sums_f64(
        _p(view), _pitch(view), view.shape[0], view.shape[1], shift,
        _p(out[1:]), None), "scvae_row_sums_f64")
    out = out.cpu().numpy()
    assert numpy.isnan(out[0]) and numpy.isnan(out[-1])
    return out[1:-1]


def check_row_sums(view, host, shift=0):
    got = device_row_sums(view, shift)
    elements = host + numpy.float32(1) if shift else host
    features = host.shape[1]
    for row, value in zip(elements.astype(numpy.float64), got):
        exact = math.fsum(row)
        bound = (features + 1) * U * math.fsum(numpy.abs(row))
        low, high = numpy.float32(exact - bound), numpy.float32(exact + bound)
        assert low <= value <= high, (value, exact, bound)


@pytest.mark.parametrize("features", FEATURES)
def test_row_sums(cuda_device, features):
    rng = numpy.random.default_rng(features)
    for rows in ROWS:
        positive = rng.gamma(0.7, 2.0, (rows, features)).astype(numpy.float32)
        mixed = rng.normal(0.0, 100.0, (rows, features)).astype(numpy.float32)
        for pad, offset in LAYOUTS:
            check_row_sums(placed(positive, pad, offset, cuda_device),
                           positive)
            check_row_sums(placed(mixed, pad, offset, cuda_device), mixed)
        check_row_sums(placed(mixed, 3, 1, cuda_device), mixed, shift=1)
    counts = rng.poisson(3.0, (63, features)).astype(numpy.float32)
    got = device_row_sums(placed(counts, 1, 1, cuda_device))
    assert numpy.array_equal(got, counts.sum(axis=1, dtype=numpy.float64))


def test_row_sums_of_long_rows_run_to_run(cuda_device):
    rng = numpy.random.default_rng(12)
    host = rng.gamma(0.7, 2.0, (5, 40000)).astype(numpy.float32)
    view = placed(host, 1, 1, cuda_device)
    check_row_sums(view, host)
    first = device_row_sums(view).view(numpy.uint32)
    assert numpy.array_equal(first, device_row_sums(view).view(numpy.uint32))
    # the same rows among others: the order of a row's sum is its own
    alone = device_row_sums(view[2:3]).view(numpy.uint32)
    assert alone[0] == first[2]


# ---- offsets past 2^31, bad arguments ----

def test_element_offsets_past_two_to_the_31(cuda_device):
    """Three rows at a pitch of 2^30 elements: the last row starts 2^31
    elements (8 GiB) into a buffer of NaN, which a 32-bit offset does not
    reach; and a flat array of 2^31 + 1031 zeros with a few values placed
    past element 2^31."""
    rows, features, pitch = 3, 1031, 2 ** 30
    edges = uniform_edges(255, 0.0, 30.0)
    host = hard_values(edges, rows * features, 31).reshape(rows, features)
    host[~numpy.isfinite(host)] = 1.0
    buffer = torch.full((1 + (rows - 1) * pitch + features,), float("nan"),
                        device=cuda_device)
    view = buffer[1:].as_strided((rows, features), (pitch, 1))
    view.copy_(torch.from_numpy(host))
    check(view, host, edges)
    check_order_statistics(view, host)
    check_row_sums(view, host)
    del view, buffer
    n = 2 ** 31 + 1031
    flat = torch.zeros(n, device=cuda_device)
    placed_values = {2 ** 31 + 7: 5.0, 2 ** 31 + 1030: 29.5, n - 3: -1.0,
                     12345: 3.0}
    for index, value in placed_values.items():
        flat[index] = value
    view = flat.view(1, n)
    counts, outside, _ = device_histogram(view, edges)
    want = numpy.zeros(255, dtype=numpy.int64)
    for value in (5.0, 29.5, 3.0):
        want[numpy.searchsorted(edges, value, "right") - 1] += 1
    want[0] += n - 4
    assert numpy.array_equal(counts, want)
    assert outside.tolist() == [1, 0, 0]
    got, lo, hi, size, nans = device_order_statistics(
        view, [0, 1, n - 4, n - 3, n - 2, n - 1, n // 2])
    assert got.tolist() == [-1.0, 0.0, 0.0, 3.0, 5.0, 29.5, 0.0]
    assert (lo, hi, size, nans) == (-1.0, 29.5, n, 0)


def test_bad_arguments_launch_nothing(cuda_device):
    from scvae_amd import _lib
    lib = _lib.load()
    host = numpy.arange(63 * 65, dtype=numpy.float32).reshape(63, 65)
    view = placed(host, 0, 0, cuda_device)
    edges = torch.from_numpy(uniform_edges(4, 0.0, 100.0)).to(cuda_device)
    cells = torch.zeros(7, dtype=torch.int64, device=cuda_device)

    def accumulate(x=view.data_ptr(), ld=65, rows=63, features=65, flags=0,
                   bins=4, e=edges.data_ptr(), c=cells.data_ptr()):
        return lib.scvae_histogram_accumulate(
            ctypes.c_void_p(x), ld, rows, features, 0, ctypes.c_void_p(e),
            flags, bins, ctypes.c_void_p(c),
            ctypes.c_void_p(c + 32 if c else None), None)
    for arguments in ({"rows": 0}, {"features": 0}, {"ld": 64}, {"bins": 0},
                      {"bins": 2 ** 20 + 1}, {"x": view.data_ptr() + 2},
                      {"x": None}, {"e": None}, {"c": None}, {"flags": 4},
                      {"flags": 1, "e": edges.data_ptr() + 4},
                      {"rows": 2, "features": 2 ** 31, "ld": 2 ** 31},
                      {"rows": 1, "features": 2 ** 40 + 1,
                       "ld": 2 ** 40 + 1}):
        assert accumulate(**arguments) == -1, arguments
        assert "bad argument" in lib.scvae_last_error().decode()
    torch.cuda.synchronize(cuda_device)
    assert not cells.cpu().numpy().any()
    workspace = torch.empty(lib.scvae_order_statistics_workspace_bytes(),
                            dtype=torch.uint8, device=cuda_device)
    out = torch.full((8,), -7.0, device=cuda_device)
    counts = torch.full((2,), -7, dtype=torch.int64, device=cuda_device)

    def select(ranks=(0,), n_ranks=None, nbytes=workspace.numel(),
               w=workspace.data_ptr(), ld=65):
        return lib.scvae_order_statistics(
            _p(view), ld, 63, 65, 0, (ctypes.c_int64 * len(ranks))(*ranks),
            len(ranks) if n_ranks is None else n_ranks, _p(out), _p(out[4:]),
            _p(counts), ctypes.c_void_p(w), nbytes, None)
    for arguments in ({"ranks": (63 * 65,)}, {"ranks": (-1,)},
                      {"ranks": (0, 1, 2, 3, 4)}, {"n_ranks": 0},
                      {"nbytes": workspace.numel() - 1}, {"w": None},
                      {"ld": 64}):
        assert select(**arguments) == -1, arguments
        assert "bad argument" in lib.scvae_last_error().decode()
    assert lib.scvae_row_sums_f64(_p(view), 64, 63, 65, 0, _p(out),
                                  None) == -1
    assert lib.scvae_row_sums_f64(_p(view), 65, 63, 65, 0, None, None) == -1
    torch.cuda.synchronize(cuda_device)
    assert (out.cpu().numpy() == -7.0).all()
    assert (counts.cpu().numpy() == -7).all()
