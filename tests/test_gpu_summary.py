"""The device summary statistics (``csrc/summary.hip``,
``analyses/summary.py``) against an fp64 oracle on the same fp32 inputs.

How the bounds are derived (u = 2^-53, the fp64 unit roundoff; first order
in u).  The kernel joins partial results (n, S, M2) by

    S = Sa + Sb,   M2 = M2a + M2b + T,   T = (nb Sa - na Sb)^2 / (na nb n)

starting from the two-pass partials of at most 16 elements a thread holds in
registers (m = S / n, M2 = sum (x - m)^2).

*   A sum S is the result of at most ``A`` additions in a fixed order: 15
    inside a chunk, one per further chunk of the thread, 6 over the lanes, 3
    over the waves, at most 4 + 6 + 3 over the workgroups' partials, one per
    call.  Any order of A additions is within A u sum |x| of the exact sum, so
    with the division |mean - mean*| <= (A + 1) u mean|x|.
*   M2 is a sum of non-negative terms, each formed with at most 8 roundings
    and then passed through at most A additions: (A + 8) u M2 of relative
    error from these.
*   The rounded chunk mean m' costs n_c (m - m')^2 <= 16 (17 u X)^2 per chunk,
    X = max |x|: relative (17 u X / sd)^2 in all, sd^2 = M2 / n.
*   A join sees Sa and Sb with errors of at most A u na X and A u nb X, so
    d = nb Sa - na Sb = na nb delta carries 2 (A + 1) u na nb X + u |d|, and T
    an error of 4 (A + 1) u X w |delta| + 6 u T with w = na nb / n.  Over all
    joins, by Cauchy-Schwarz, sum w |delta| <= sqrt(sum w) sqrt(sum T), and
    sum T <= M2.  sum w: w <= nb, and in each of the five in-order stages
    (a thread's chunks, the waves, a thread's workgroup partials, the waves
    again, the calls) every partial is the b of one join, n per stage; in each
    of the 12 tree levels w <= n_ab / 2, n / 2 per level: sum w <= 11 n.
    Relative to M2: 4 (A + 1) sqrt(11) u X / sd.  This is the term that sees
    the condition number X / sd; the one-pass formula sees its square.
*   Where the oracle forms an element differently (the log-ratios: two
    ``log1p`` of different libraries), a per-element error e moves the mean
    by at most e and M2 by at most 2 e sqrt(n M2) + n e^2.

The standard deviation carries half the relative error of M2; the asserts
allow all of it.
"""
import ctypes
import math
import re
from fractions import Fraction

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
#: csrc/summary.hip: virtual columns of a tile, most workgroups of a launch
TILE_COLUMNS, MAX_WORKGROUPS = 4096, 1024
TOLERANCE = 0.5
ROWS = (1, 2, 63, 300)
FEATURES = (1, 3, 63, 64, 65, 257, 1031)
#: (pad of recon's pitch, pad of orig's pitch, offset of recon's base, offset
#: of orig's base), in elements: aligned and dense; both one element off (the
#: same phase); and two with different phases and pitches
LAYOUTS = ((0, 0, 0, 0), (3, 3, 1, 1), (1, 2, 1, 0), (5, 0, 0, 1))


def additions(rows, features, calls=1):
    """A of the module docstring for a call of this shape."""
    tiles = rows * -(-(features + 3) // TILE_COLUMNS)
    chunks = -(-tiles // min(tiles, MAX_WORKGROUPS))
    return 15 + chunks + 6 + 3 + 4 + 6 + 3 + calls


def oracle(e, count=True):
    """(n, count, mean, sd, min, max, M2, mean |x|, max |x|) of the fp64
    elements e, sums by ``math.fsum``."""
    e = numpy.asarray(e, dtype=numpy.float64).reshape(-1)
    n = e.size
    mean = math.fsum(e) / n
    m2 = math.fsum((e - mean) ** 2)
    sd = math.sqrt(m2 / (n - 1)) if n > 1 else float("nan")
    return {"n": n, "count": int((e >= TOLERANCE).sum()) if count else 0,
            "mean": mean, "sd": sd, "min": float(e.min()),
            "max": float(e.max()), "m2": m2,
            "mean_abs": math.fsum(numpy.abs(e)) / n,
            "max_abs": float(numpy.abs(e).max())}


def streams_oracle(recon, orig):
    recon64 = numpy.asarray(recon, dtype=numpy.float64)
    orig64 = numpy.asarray(orig, dtype=numpy.float64)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        log_ratios = numpy.abs(numpy.log1p(recon64) - numpy.log1p(orig64))
    streams = [oracle(orig64), oracle(recon64),
               oracle(numpy.abs(recon64 - orig64), count=False),
               oracle(log_ratios, count=False)]
    # where some x~ equals its x, both sides' log-ratio there is exactly 0
    streams[3]["equal_pair"] = bool((recon64 == orig64).any())
    return streams


def log1p_element_error(recon, orig):
    """e for the log-ratios: the device's ``log1p`` is within 2 ulp (the
    OpenCL bound its library keeps), the host's within 1 ulp, an ulp of L is
    at most 2 u L, and each side rounds its subtraction once."""
    largest = float(numpy.log1p(numpy.float64(max(
        numpy.abs(recon).max(), numpy.abs(orig).max()))))
    return 2 * (4 * U + 2 * U) * largest + 2 * U * largest


def mean_bound(want, a, element_error=0.0):
    return (a + 1) * U * want["mean_abs"] + element_error


def m2_relative_bound(want, a, element_error=0.0):
    sd = math.sqrt(want["m2"] / want["n"])
    x = want["max_abs"]
    return ((a + 8) * U + (17 * U * x / sd) ** 2
            + 4 * (a + 1) * math.sqrt(11.0) * U * x / sd
            + 2 * element_error / sd + (element_error / sd) ** 2)


def check_stream(got, want, a, element_error=0.0, exact_extremes=True):
    n, count, mean, sd, lo, hi = got
    assert n == want["n"] and count == want["count"]
    if exact_extremes:
        assert lo == want["min"] and hi == want["max"]
    else:
        assert abs(lo - want["min"]) <= element_error
        if want.get("equal_pair"):
            assert lo == 0.0 and want["min"] == 0.0
        assert abs(hi - want["max"]) <= element_error
    bound = mean_bound(want, a, element_error)
    print("mean {:.17g} want {:.17g} bound {:.3g}".format(
        mean, want["mean"], bound))
    assert abs(mean - want["mean"]) <= bound
    if n == 1:
        assert math.isnan(sd)
    elif want["m2"] == 0.0:
        assert sd == 0.0
    else:
        relative = m2_relative_bound(want, a, element_error)
        print("sd {:.17g} want {:.17g} relative bound {:.3g}".format(
            sd, want["sd"], relative))
        assert abs(sd - want["sd"]) <= relative * want["sd"]


def placed(values, pad, offset, device):
    """``values`` on the device as a matrix of pitch F + pad whose base lies
    ``offset`` elements into a 256-byte aligned buffer; everything around the
    values is NaN, so a read outside them shows in every statistic."""
    rows, features = values.shape
    pitch = features + pad
    buffer = torch.full((offset + rows * pitch + 8,), float("nan"),
                        device=device)
    view = buffer[offset:offset + rows * pitch].view(rows, pitch)[:, :features]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() == buffer.data_ptr() + 4 * offset
    return view


def count_like(rows, features, seed):
    """(recon, orig): counts with many zeros against positive rates, with
    values exactly at the tolerance, the next value below it, and negative
    values of a magnitude above it in both."""
    rng = numpy.random.default_rng(seed)
    orig = (rng.poisson(1.5, (rows, features))
            * (rng.random((rows, features)) < 0.4)).astype(numpy.float32)
    recon = rng.gamma(0.7, 2.0, (rows, features)).astype(numpy.float32)
    below = numpy.nextafter(numpy.float32(TOLERANCE), numpy.float32(0))
    special = numpy.array([TOLERANCE, below, -0.75, 0.0], dtype=numpy.float32)
    n = rows * features
    for matrix, shift in ((orig, 0), (recon, 1)):
        flat = matrix.reshape(-1)
        for k in range(min(n, 8)):
            flat[(k * 7919 + shift) % n] = special[(k + shift) % 4]
    if n > 2:       # one pair of equal values: a log-ratio of exactly 0
        recon.reshape(-1)[n // 2] = orig.reshape(-1)[n // 2] = 3.0
    return recon, orig


_CASES = {}


def case(rows, features):
    """One pair of matrices and its oracle per shape, shared by the tests."""
    key = (rows, features)
    if key not in _CASES:
        recon, orig = count_like(rows, features, 1000 * rows + features)
        _CASES[key] = (recon, orig, streams_oracle(recon, orig),
                       log1p_element_error(recon, orig))
    return _CASES[key]


def run(device, recon=None, orig=None, comparisons=True, blocks=None,
        summary=None):
    """The finished streams after feeding the row blocks ``blocks`` (bounds,
    default all rows in one call)."""
    from scvae_amd.analyses.summary import DeviceSummary
    if summary is None:
        summary = DeviceSummary(TOLERANCE, comparisons=comparisons,
                                device=device)
    rows = (recon if recon is not None else orig).shape[0]
    bounds = [0, rows] if blocks is None else blocks
    for first, last in zip(bounds[:-1], bounds[1:]):
        summary.add(
            reconstructed=None if recon is None else recon[first:last],
            original=None if orig is None else orig[first:last])
    return summary.finish()


@pytest.mark.parametrize("features", FEATURES)
def test_shapes_and_pitches(cuda_device, features):
    """Every stream against the oracle for every row count, with dense and
    padded pitches (NaN in the pad), aligned and offset bases, equal and
    different phases of the two inputs; n, minimum, maximum and the count are
    equal.  The log-ratios' extremes are held to the element bound: their
    elements come from another ``log1p`` than the oracle's; their minimum is
    exactly 0 where a pair of equal values makes it so."""
    for rows in ROWS:
        recon, orig, want, element_error = case(rows, features)
        a = additions(rows, features)
        for pad_r, pad_o, off_r, off_o in LAYOUTS:
            got = run(cuda_device, placed(recon, pad_r, off_r, cuda_device),
                      placed(orig, pad_o, off_o, cuda_device))
            for s in range(3):
                check_stream(got[s], want[s], a)
            check_stream(got[3], want[3], a, element_error,
                         exact_extremes=False)
        # one input alone: its stream as before, the others empty
        alone = run(cuda_device, recon=placed(recon, 3, 1, cuda_device),
                    comparisons=False)
        check_stream(alone[1], want[1], a)
        alone = run(cuda_device, orig=placed(orig, 0, 1, cuda_device),
                    comparisons=False)
        check_stream(alone[0], want[0], a)
        for s in (1, 2, 3):
            assert alone[s][:2] == (0, 0) and math.isnan(alone[s][2])


def test_several_workgroups_a_tile(cuda_device):
    """1024 x 1031: as many tiles as a launch has workgroups; 2048 and 2049:
    two tiles each, and with one more row a third for the first of them."""
    for rows in (1024, 2048, 2049):
        recon, orig, want, element_error = case(rows, 1031)
        a = additions(rows, 1031)
        got = run(cuda_device, placed(recon, 1, 1, cuda_device),
                  placed(orig, 0, 0, cuda_device))
        for s in range(3):
            check_stream(got[s], want[s], a)
        check_stream(got[3], want[3], a, element_error, exact_extremes=False)


def test_element_offsets_past_two_to_the_31(cuda_device):
    """Three rows at a pitch of 2^30 elements: the last row starts 2^31
    elements (8 GiB) into the buffer, which a 32-bit offset does not reach.
    The buffer is NaN throughout, so rows read at a wrapped offset show."""
    rows, features, pitch = 3, 1031, 2 ** 30
    recon, orig = count_like(rows, features, 31)
    want = streams_oracle(recon, orig)
    element_error = log1p_element_error(recon, orig)
    views = []
    for values, offset in ((recon, 1), (orig, 0)):
        buffer = torch.full((offset + (rows - 1) * pitch + features,),
                            float("nan"), device=cuda_device)
        view = buffer[offset:].as_strided((rows, features), (pitch, 1))
        view.copy_(torch.from_numpy(values))
        views.append(view)
    got = run(cuda_device, views[0], views[1])
    a = additions(rows, features)
    for s in range(3):
        check_stream(got[s], want[s], a)
    check_stream(got[3], want[3], a, element_error, exact_extremes=False)


def test_exact_sums(cuda_device):
    """Integer counts with sum x^2 < 2^53: every S is an integer below 2^53,
    so the mean is float(sum x) / n bit for bit, and the variance meets its
    bound against the exact rational value."""
    rng = numpy.random.default_rng(5)
    for rows, features in ((63, 65), (300, 1031)):
        counts = rng.poisson(3.0, (rows, features))
        counts[rng.random((rows, features)) < 0.01] = 60000
        total, squares, n = int(counts.sum()), int((counts ** 2).sum()), \
            counts.size
        assert squares < 2 ** 53
        got = run(cuda_device,
                  orig=placed(counts.astype(numpy.float32), 1, 1, cuda_device),
                  comparisons=False)[0]
        assert got[0] == n and got[2] == float(total) / n
        m2 = Fraction(squares) - Fraction(total * total, n)
        want = dict(oracle(counts), m2=float(m2),
                    sd=math.sqrt(float(m2 / (n - 1))))
        relative = m2_relative_bound(want, additions(rows, features))
        print("sd {:.17g} want {:.17g} relative bound {:.3g}".format(
            got[3], want["sd"], relative))
        assert abs(got[3] - want["sd"]) <= relative * want["sd"]
        assert got[4] == counts.min() and got[5] == counts.max()


def test_cancellation(cuda_device):
    """fp32 values around 10 000 with a spread of about 0.01: mean^2 /
    variance is near 1e12.  The values are integers times 2^-10, so the exact
    variance is a rational number.  The bound of the module docstring is
    linear in X / sd and comes out below 1e-6.  The one-pass formula
    sum x^2 - (sum x)^2 / n cannot reach that in fp64: a correctly rounded
    sum x^2 alone is off by up to u sum x^2 = u n (mean^2 + var), which
    against M2 = n var is u (mean / sd)^2 -- above 1e-6 here, whatever the
    order of the additions."""
    rows, features = 300, 1031
    rng = numpy.random.default_rng(11)
    values = (10000.0 + rng.uniform(-0.02, 0.02, (rows, features))).astype(
        numpy.float32)
    scaled = numpy.asarray(values, dtype=numpy.float64) * 1024.0
    integers = scaled.astype(numpy.int64)
    assert numpy.array_equal(integers.astype(numpy.float64), scaled)
    n = values.size
    total = sum(int(k) for k in integers.reshape(-1))
    squares = sum(int(k) * int(k) for k in integers.reshape(-1))
    m2 = (Fraction(squares) - Fraction(total * total, n)) / (1024 * 1024)
    want = dict(oracle(values), m2=float(m2),
                sd=math.sqrt(float(m2 / (n - 1))))
    condition = (want["mean"] / want["sd"]) ** 2
    assert 1e11 < condition < 1e13
    assert U * condition > 1e-6          # the one-pass formula's floor
    relative = m2_relative_bound(want, additions(rows, features))
    assert relative < 1e-6
    for pad, offset in ((0, 0), (1, 1)):
        got = run(cuda_device, recon=placed(values, pad, offset, cuda_device),
                  comparisons=False)[1]
        error = abs(got[3] - want["sd"]) / want["sd"]
        print("sd {:.17g} want {:.17g} relative error {:.3g} bound {:.3g}"
              .format(got[3], want["sd"], error, relative))
        assert error <= relative
        assert abs(got[2] - float(Fraction(total, n) / 1024)) <= mean_bound(
            want, additions(rows, features))


def _bits(streams):
    return [(n, count) + tuple(numpy.array(rest).view(numpy.int64).tolist())
            for n, count, *rest in streams]


def test_accumulation(cuda_device):
    """All rows in one call against the same rows in blocks of 1, 7 and the
    rest: both are within their bounds of the exact values, so of each other
    by the sum of the two; counts and extremes are equal.  The same sequence
    twice gives the same bits, and a reset empties the state."""
    from scvae_amd.analyses.summary import DeviceSummary
    rows, features = 300, 257
    recon, orig, want, element_error = case(rows, features)
    r, o = (placed(recon, 3, 1, cuda_device),
            placed(orig, 0, 0, cuda_device))
    whole = run(cuda_device, r, o)
    blocks = [0, 1, 8, rows]
    pieces = run(cuda_device, r, o, blocks=blocks)
    a_whole, a_pieces = additions(rows, features), additions(
        rows, features, calls=3)
    for s in range(4):
        error = element_error if s == 3 else 0.0
        check_stream(pieces[s], want[s], a_pieces, error,
                     exact_extremes=s < 3)
        assert pieces[s][:2] == whole[s][:2]
        assert pieces[s][4:] == whole[s][4:]
        assert abs(pieces[s][2] - whole[s][2]) <= (
            mean_bound(want[s], a_whole) + mean_bound(want[s], a_pieces))
        assert abs(pieces[s][3] - whole[s][3]) <= want[s]["sd"] * (
            m2_relative_bound(want[s], a_whole)
            + m2_relative_bound(want[s], a_pieces))
    assert _bits(run(cuda_device, r, o, blocks=blocks)) == _bits(pieces)
    assert _bits(run(cuda_device, r, o)) == _bits(whole)
    # one state: fed, reset, fed again -- as if fresh; without the reset the
    # second feed adds to the first
    summary = DeviceSummary(TOLERANCE, comparisons=True, device=cuda_device)
    run(cuda_device, r, o, blocks=blocks, summary=summary)
    summary.reset()
    empty = summary.finish()
    assert all(stream[:2] == (0, 0) and math.isnan(stream[2])
               for stream in empty)
    assert _bits(run(cuda_device, r, o, summary=summary)) == _bits(whole)
    doubled = run(cuda_device, r, o, summary=summary)
    assert [s[0] for s in doubled] == [2 * s[0] for s in whole]
    assert [s[1] for s in doubled] == [2 * s[1] for s in whole]


def test_special_values(cuda_device):
    from scvae_amd.analyses import summary_statistics
    rows, features = 63, 257
    recon, orig, want, _ = case(rows, features)
    clean = run(cuda_device, placed(recon, 1, 1, cuda_device),
                placed(orig, 1, 1, cuda_device))
    # a NaN in recon: its stream and the two comparisons are NaN, orig is
    # untouched to the bit; NaN is not counted as >= tolerance
    spoiled = recon.copy()
    spoiled[40, 129] = numpy.nan
    got = run(cuda_device, placed(spoiled, 1, 1, cuda_device),
              placed(orig, 1, 1, cuda_device))
    assert _bits([got[0]]) == _bits([clean[0]])
    for s in (1, 2, 3):
        assert got[s][0] == rows * features
        assert all(math.isnan(v) for v in got[s][2:]), got[s]
    assert got[1][1] == int((spoiled >= TOLERANCE).sum())
    # ... and in orig: recon is untouched
    spoiled = orig.copy()
    spoiled[0, 0] = numpy.nan
    got = run(cuda_device, placed(recon, 1, 1, cuda_device),
              placed(spoiled, 1, 1, cuda_device))
    assert _bits([got[1]]) == _bits([clean[1]])
    assert all(math.isnan(v) for v in got[0][2:])
    # + inf in recon
    spoiled = recon.copy()
    spoiled[62, 256] = numpy.inf
    got = run(cuda_device, placed(spoiled, 0, 0, cuda_device),
              placed(orig, 0, 0, cuda_device))
    assert got[1][5] == math.inf and got[1][2] == math.inf
    assert got[1][4] == want[1]["min"]
    assert got[1][1] == want[1]["count"] + (recon[62, 256] < TOLERANCE)
    assert _bits([got[0]]) == _bits([clean[0]])
    # one element: no standard deviation
    one = summary_statistics(numpy.array([[2.5]], dtype=numpy.float32),
                             name="one", tolerance=TOLERANCE)
    assert one["mean"] == 2.5 and one["minimum"] == one["maximum"] == 2.5
    assert math.isnan(one["standard deviation"]) and one["sparsity"] == 0.0
    # all zeros
    zeros = summary_statistics(numpy.zeros((5, 70), dtype=numpy.float32),
                               name="zeros")
    assert zeros["name"] == "zeros"
    assert zeros["mean"] == 0.0 and zeros["standard deviation"] == 0.0
    assert math.isnan(zeros["dispersion"]) and zeros["sparsity"] == 1.0
    assert math.isnan(summary_statistics(
        numpy.zeros(7, dtype=numpy.float32), skip_sparsity=True)["sparsity"])


def test_log1p_range(cuda_device):
    """x~ and x from 0 and 1e-8 up to 6e4: the log-ratios against fp64
    ``log1p``.  The element bound is 14 u log1p(6e4), about 1.7e-14; fp32
    ``log1pf`` is off by 6e-8 of a value of up to 11 per element, which the
    bounds of the mean and of the extremes below do not admit."""
    rows, features = 63, 65
    rng = numpy.random.default_rng(17)
    grid = numpy.concatenate([[0.0], numpy.geomspace(1e-8, 6e4, 200)])
    recon = rng.choice(grid, (rows, features)).astype(numpy.float32)
    orig = rng.choice(grid, (rows, features)).astype(numpy.float32)
    want = streams_oracle(recon, orig)
    element_error = log1p_element_error(recon, orig)
    assert element_error < 2e-14
    got = run(cuda_device, placed(recon, 2, 1, cuda_device),
              placed(orig, 0, 0, cuda_device))
    a = additions(rows, features)
    for s in range(3):
        check_stream(got[s], want[s], a)
    check_stream(got[3], want[3], a, element_error, exact_extremes=False)
    assert mean_bound(want[3], a, element_error) < 1e-12


def test_public_functions_take_every_kind_of_input(cuda_device):
    """NumPy of any shape (flattened), SciPy sparse (densified on the device
    in row blocks), and a device tensor read in place; blocks of rows that do
    not divide the set."""
    import scipy.sparse
    from scvae_amd.analyses import comparison_statistics, summary_statistics
    rows, features = 300, 65
    recon, orig, want, element_error = case(rows, features)
    a = additions(rows, features, calls=5)

    def as_stream(row, n):
        count = round((1 - row["sparsity"]) * n) if not math.isnan(
            row["sparsity"]) else 0
        return (n, count, row["mean"], row["standard deviation"],
                row["minimum"], row["maximum"])
    n = rows * features
    for x in (orig, orig.reshape(-1), orig.reshape(4, 75, 65),
              scipy.sparse.csr_matrix(orig),
              torch.from_numpy(orig).to(cuda_device),
              torch.from_numpy(orig).to(cuda_device).reshape(-1)):
        row = summary_statistics(x, name="x", tolerance=TOLERANCE)
        check_stream(as_stream(row, n), want[0], a)
        assert row["sparsity"] == 1 - want[0]["count"] / n
        assert row["dispersion"] == row["standard deviation"] ** 2 / row[
            "mean"]
    for original in (orig, scipy.sparse.csr_matrix(orig),
                     torch.from_numpy(orig).to(cuda_device)):
        table = comparison_statistics(
            original, torch.from_numpy(recon).to(cuda_device),
            tolerance=TOLERANCE, extensive=True, row_block=64)
        assert [r["name"] for r in table] == [
            "original", "reconstructed", "differences", "log-ratios"]
        for s in range(3):
            check_stream(as_stream(table[s], n)[:1] + (want[s]["count"],)
                         + as_stream(table[s], n)[2:], want[s], a)
        check_stream((n, 0) + as_stream(table[3], n)[2:], want[3], a,
                     element_error, exact_extremes=False)
        assert math.isnan(table[2]["sparsity"])
        assert table[1]["sparsity"] == 1 - want[1]["count"] / n
    assert len(comparison_statistics(orig, recon, tolerance=TOLERANCE)) == 2


def _tiny_set():
    import scipy.sparse
    from scvae_amd.data import DataSet
    rng = numpy.random.default_rng(23)
    n, features = 90, 37
    x = (rng.poisson(2.0, (n, features))
         * (rng.random((n, features)) < 0.5)).astype(numpy.float32)
    return DataSet("tiny", values=scipy.sparse.csr_matrix(x),
                   example_names=numpy.arange(n).astype(str),
                   feature_names=numpy.arange(features).astype(str),
                   kind="test")


def _dense(values):
    return numpy.asarray(values.todense() if hasattr(values, "todense")
                         else values, dtype=numpy.float32)


def _check_attached(rows, reconstructed, data_set, first_name="original"):
    values = _dense(data_set.values)
    recon = numpy.asarray(reconstructed.values, dtype=numpy.float32)
    want = streams_oracle(recon, values)
    element_error = log1p_element_error(recon, values)
    n = values.size
    a = additions(*values.shape)
    assert [r["name"] for r in rows] == [
        first_name, "reconstructed", "differences", "log-ratios"]
    for s, row in enumerate(rows):
        stream = (n, want[s]["count"], row["mean"],
                  row["standard deviation"], row["minimum"], row["maximum"])
        check_stream(stream, want[s], a, element_error if s == 3 else 0.0,
                     exact_extremes=s < 3)
        if s < 2:
            assert row["sparsity"] == 1 - want[s]["count"] / n
        else:
            assert math.isnan(row["sparsity"])
        assert row["dispersion"] == row["standard deviation"] ** 2 / row[
            "mean"]


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
    assert not hasattr(plain[1], "summary_statistics")
    extensive = model.evaluate(data_set, summary_statistics="extensive",
                               **arguments)
    assert len(extensive) == 3 and extensive[0] is data_set
    assert numpy.array_equal(extensive[1].values, plain[1].values)
    assert numpy.array_equal(extensive[2]["z"].values, plain[2]["z"].values)
    assert len(extensive[1].summary_statistics) == 4
    _check_attached(extensive[1].summary_statistics, extensive[1], data_set)
    for level in (True, "normal"):
        normal = model.evaluate(data_set, summary_statistics=level,
                                **arguments)
        assert normal[1].summary_statistics == extensive[
            1].summary_statistics[:2]
    reconstructed = model.evaluate(
        data_set, summary_statistics=True, output_versions="reconstructed",
        **arguments)
    assert reconstructed.summary_statistics == normal[1].summary_statistics
    with pytest.raises(ValueError, match="reconstructed"):
        model.evaluate(data_set, summary_statistics=True,
                       output_versions=["latent"], **arguments)
    with pytest.raises(ValueError, match="`all` not found"):
        model.evaluate(data_set, summary_statistics="all", **arguments)


def test_transformed_set_through_the_model(tmp_path, cuda_device):
    """A Bernoulli model's likelihood sees the binarised values: the first
    row is named after the transformed set the evaluation returns and holds
    the statistics of its values, not of the counts."""
    from scvae_amd.models import VariationalAutoencoder
    data_set = _tiny_set()
    state = numpy.random.get_state()
    numpy.random.seed(7)
    try:
        model = VariationalAutoencoder(
            feature_size=37, latent_size=3, hidden_sizes=[12],
            reconstruction_distribution="bernoulli",
            log_directory=str(tmp_path))
        model.train(data_set, number_of_epochs=1, minibatch_size=32)
    finally:
        numpy.random.set_state(state)
    transformed, reconstructed, _ = model.evaluate(
        data_set, summary_statistics="extensive", minibatch_size=32,
        use_deterministic_z=True, log_results=False)
    assert transformed.version == "transformed"
    binarised = _dense(transformed.values)
    assert numpy.array_equal(binarised,
                             (_dense(data_set.values) > 0.5).astype("f4"))
    rows = reconstructed.summary_statistics
    _check_attached(rows, reconstructed, transformed, "transformed")
    assert rows[0]["maximum"] == 1.0 and rows[0]["minimum"] == 0.0
    assert rows[0]["mean"] == float(binarised.sum()) / binarised.size
    assert rows[0]["mean"] != _dense(data_set.values).mean()


def _two_rank_worker(rank, port, directory):
    """Rank body: both ranks share cuda:0 (gloo carries the collectives), as
    in test_gpu_dataparallel.py.  ``cli.train`` and ``cli.evaluate`` with the
    switch, this rank's printed text kept."""
    import contextlib
    import io
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        from scvae_amd import cli
        data_set = _tiny_set()
        cli._load_data = lambda *a, **kw: (
            data_set, (data_set, None, data_set), None, None)
        cli.build_directory_path = lambda *a, **kw: directory
        cli.indices_for_evaluation_subset = lambda data_set: set()
        arguments = dict(latent_size=3, hidden_sizes=[12], minibatch_size=32,
                         reconstruction_distribution="poisson")
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            numpy.random.seed(7)
            cli.train("tiny", number_of_epochs=1, **arguments)
            results = cli.evaluate(
                "tiny", sample_size=0, summary_statistics=True,
                analysis_level="extensive", **arguments)
        text = text.getvalue()
        reconstructed = results["end_of_training"][1]
        if rank == 0:
            # over the assembled reconstruction: the other rank's rows too
            _check_attached(reconstructed.summary_statistics, reconstructed,
                            data_set)
            assert text.count("Calculating metrics for results.") == 1
            assert text.count("Metrics calculated (") == 1
            assert text.count("sparsity") == 1
            assert text.count("\nlog-ratios ") == 1
        else:
            assert not hasattr(reconstructed, "summary_statistics")
            assert "metrics" not in text.lower() and "sparsity" not in text
        with open(os.path.join(directory, "rank{}".format(rank)), "w") as f:
            f.write("done")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_through_the_command_line(tmp_path, cuda_device):
    """Several ranks: rank 0 computes, attaches and prints the table once,
    over the reconstruction the all-reduce assembled; the other rank has no
    rows, prints nothing of it and finishes."""
    import os
    import torch.multiprocessing as mp
    port = 29650 + (os.getpid() % 100)
    mp.spawn(_two_rank_worker, args=(port, str(tmp_path)), nprocs=2,
             join=True)
    assert sorted(p.name for p in tmp_path.glob("rank*")) == [
        "rank0", "rank1"]


def test_through_the_command_line(tmp_path, cuda_device, monkeypatch, capsys):
    from scvae_amd import cli
    data_set = _tiny_set()
    monkeypatch.setattr(
        cli, "_load_data",
        lambda *a, **kw: (data_set, (data_set, None, data_set), None, None))
    monkeypatch.setattr(cli, "build_directory_path",
                        lambda *a, **kw: str(tmp_path))
    monkeypatch.setattr(cli, "indices_for_evaluation_subset",
                        lambda data_set: set())
    arguments = dict(latent_size=3, hidden_sizes=[12], minibatch_size=32,
                     reconstruction_distribution="poisson")
    cli.train("tiny", number_of_epochs=1, **arguments)
    capsys.readouterr()
    cli.evaluate("tiny", sample_size=0, **arguments)
    plain = capsys.readouterr().out
    assert "metrics" not in plain.lower() and "sparsity" not in plain
    results = cli.evaluate("tiny", sample_size=0, summary_statistics=True,
                           analysis_level="extensive", **arguments)
    lines = capsys.readouterr().out.splitlines()
    reconstructed = results["end_of_training"][1]
    _check_attached(reconstructed.summary_statistics, reconstructed, data_set)
    at = lines.index("Calculating metrics for results.")
    assert lines[at - 1].startswith("    Test set (")
    assert re.fullmatch(r"Metrics calculated \(.+\)\.", lines[at + 1])
    assert lines[at + 2] == ""
    assert lines[at + 3].split() == [
        "Data", "set", "mean", "std.", "dev.", "dispersion", "minimum",
        "maximum", "sparsity"]
    for line, row in zip(lines[at + 4:at + 8],
                         reconstructed.summary_statistics):
        fields = line.split()
        assert fields[0] == row["name"] and len(fields) == 7
        for field, key in zip(fields[1:], (
                "mean", "standard deviation", "dispersion", "minimum",
                "maximum", "sparsity")):
            shown = float("{:.5g}".format(row[key]))
            assert float(field) == shown or (
                math.isnan(float(field)) and math.isnan(shown))
    assert lines[at + 8] == ""


def test_bad_arguments_through_the_entries(cuda_device):
    """-1 with a message, and the state is as it was: nothing was launched."""
    from scvae_amd import _lib
    from scvae_amd.analyses.summary import DeviceSummary
    lib = _lib.load()
    recon, orig, _, _ = case(63, 65)
    r, o = placed(recon, 0, 0, cuda_device), placed(orig, 0, 0, cuda_device)
    summary = DeviceSummary(TOLERANCE, comparisons=True, device=cuda_device)
    summary.add(reconstructed=r, original=o)
    before = _bits(summary.finish())
    workspace = ctypes.c_void_p(summary.workspace.data_ptr())
    need = summary.workspace.numel()
    rp, op = ctypes.c_void_p(r.data_ptr()), ctypes.c_void_p(o.data_ptr())

    def accumulate(recon=rp, ldr=65, orig=op, ldo=65, rows=63, features=65,
                   comparisons=1, workspace=workspace, nbytes=need):
        return lib.scvae_summary_accumulate(
            recon, ldr, orig, ldo, rows, features, TOLERANCE, comparisons,
            workspace, nbytes, None)
    for arguments in ({"rows": 0}, {"features": 0}, {"ldr": 64}, {"ldo": 64},
                      {"recon": None, "orig": None, "comparisons": 0},
                      {"orig": None}, {"workspace": None},
                      {"nbytes": need - 1},
                      {"recon": ctypes.c_void_p(r.data_ptr() + 2)}):
        assert accumulate(**arguments) == -1, arguments
        assert "bad argument" in lib.scvae_last_error().decode()
    assert lib.scvae_summary_reset(workspace, need - 1, None) == -1
    assert lib.scvae_summary_finish(workspace, need, None, None, None) == -1
    torch.cuda.synchronize(cuda_device)
    assert _bits(summary.finish()) == before
