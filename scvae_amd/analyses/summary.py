"""Summary statistics of data sets on the device: the metrics table that
``analyse_results`` prints first (``scvae/analyses/analyses.py:873-895, 1040``,
built by ``scvae/analyses/metrics/summary.py:27-93``) -- mean, standard
deviation (ddof 1), dispersion, minimum, maximum and sparsity of the
evaluation set and of the reconstructed set, and with the analysis level
``extensive`` of ``differences`` |x~ - x| and ``log-ratios``
|log1p x~ - log1p x| (``analyses.py:796-802, 882-892``) -- from one streaming
pass of the kernel of ``csrc/summary.hip`` over blocks of rows.

What differs from the reference on purpose: every sum is taken in fp64, the
variance from two-pass partials of 16 elements joined pairwise with Chan's
formula (the reference takes fp32 ``mean()`` / ``std()`` for small sets and
the cancelling ``E[x^2] - E[x]^2`` above 5e8 values); and the elements of the
two comparison rows are formed in fp64 from the fp32 values (the reference
rounds the difference and both ``log1p`` to fp32 per element).  The tolerance
of the sparsity is rounded to fp32, which is what NumPy compares fp32 values
with.  Every sum has one fixed order, so the same input gives the same bits
on every run.
"""
import ctypes
import math

import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses.kmeans import _ptr

#: rows of a block handed to the kernel where a set is fed in pieces: a
#: multiple of 4, so that every block of a contiguous fp32 matrix starts at the
#: alignment of the matrix itself
ROW_BLOCK = 2048
#: elements of a piece of a flattened array
_FLAT_BLOCK = 1 << 26


def _check_tolerance(tolerance):
    tolerance = float(tolerance)
    if math.isnan(tolerance):
        raise ValueError("The tolerance of the sparsity must be a number.")
    return float(numpy.float32(tolerance))


def _is_sparse(x):
    return hasattr(x, "tocsr") and not isinstance(x, numpy.ndarray)


def _check_values(x, what):
    """Shape of ``x`` as a matrix ([1, size] for what is not 2-D)."""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise ValueError("{}: a float32 tensor expected, got {}.".format(
                what, x.dtype))
        shape = tuple(x.shape)
    elif _is_sparse(x):
        shape = tuple(x.shape)
    else:
        shape = numpy.shape(x)
    size = 1
    for extent in shape:
        size *= int(extent)
    if size == 0:
        raise ValueError("{}: no values.".format(what))
    if len(shape) != 2:
        shape = (1, size)
    return int(shape[0]), int(shape[1])


def statistics_dictionary(name, n, count, mean, standard_deviation, minimum,
                          maximum, skip_sparsity=False):
    """The reference's result dict (``summary.py:47-57``) from a stream's
    numbers."""
    with numpy.errstate(divide="ignore", invalid="ignore"):
        dispersion = float(numpy.float64(standard_deviation) ** 2
                           / numpy.float64(mean))
    sparsity = float("nan") if skip_sparsity or n == 0 else 1 - count / n
    return {
        "name": name,
        "mean": mean,
        "standard deviation": standard_deviation,
        "minimum": minimum,
        "maximum": maximum,
        "dispersion": dispersion,
        "sparsity": sparsity,
    }


class DeviceSummary:
    """The state the kernel's calls add to.  ``add`` takes blocks of rows
    (fp32 device tensors ``[rows, F]`` with unit column stride; a row pitch is
    taken as it is), ``finish`` returns per stream
    ``(n, count, mean, standard deviation, minimum, maximum)``."""

    def __init__(self, tolerance=0.5, comparisons=False, device=None):
        tolerance = _check_tolerance(tolerance)
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(
                "No GPU visible: the device summary statistics have no CPU "
                "path.")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tolerance = tolerance
        self.comparisons = bool(comparisons)
        self.workspace = torch.empty(
            self.lib.scvae_summary_workspace_bytes(), dtype=torch.uint8,
            device=self.device)
        self.reset()

    def _stream(self):
        return ctypes.c_void_p(
            torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_summary_reset(
                _ptr(self.workspace), self.workspace.numel(), self._stream()),
                "scvae_summary_reset")

    def add(self, reconstructed=None, original=None):
        present = [t for t in (reconstructed, original) if t is not None]
        if not present:
            raise ValueError("Summary statistics: no values.")
        for tensor in present:
            if (tensor.dtype != torch.float32 or tensor.dim() != 2
                    or tensor.stride(1) != 1 or tensor.device != self.device
                    or tensor.shape != present[0].shape):
                raise ValueError(
                    "Summary statistics: fp32 matrices of one shape with "
                    "unit column stride on {} expected.".format(self.device))
        rows, features = present[0].shape

        def pitch(tensor):
            return 0 if tensor is None else (
                tensor.stride(0) if rows > 1 else features)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_summary_accumulate(
                _ptr(reconstructed), pitch(reconstructed), _ptr(original),
                pitch(original), rows, features, self.tolerance,
                int(self.comparisons and len(present) == 2),
                _ptr(self.workspace), self.workspace.numel(), self._stream()),
                "scvae_summary_accumulate")

    def finish(self):
        stats = torch.empty(4, 4, dtype=torch.float64, device=self.device)
        counts = torch.empty(4, 2, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.scvae_summary_finish(
                _ptr(self.workspace), self.workspace.numel(), _ptr(stats),
                _ptr(counts), self._stream()), "scvae_summary_finish")
        stats, counts = stats.cpu().tolist(), counts.cpu().tolist()
        return [(counts[s][0], counts[s][1]) + tuple(stats[s])
                for s in range(4)]


def _row_provider(x, device):
    """``take(first, last)``: the rows ``first .. last - 1`` of the matrix
    ``x`` as an fp32 device matrix (valid until the next call)."""
    if isinstance(x, torch.Tensor):
        x = x.to(device)
        if x.stride(1) != 1:
            x = x.contiguous()
        return lambda first, last: x[first:last]     # read where it lies
    if _is_sparse(x):
        from scvae_amd.minibatch import DeviceCSR
        csr = DeviceCSR.from_scipy(x, device)
        held = {}

        def take(first, last):
            if "buffer" not in held or held["buffer"].shape[0] < last - first:
                held["buffer"] = torch.empty(
                    last - first, csr.shape[1], dtype=torch.float32,
                    device=csr.device)
            index = torch.arange(first, last, dtype=torch.int64,
                                 device=csr.device)
            return csr.gather_dense(index,
                                    out=held["buffer"][:last - first])
        return take
    x = numpy.asarray(x)
    return lambda first, last: torch.from_numpy(numpy.ascontiguousarray(
        x[first:last], dtype=numpy.float32)).to(device)


def _blocks(x, shape, device, row_block):
    """``x`` as fp32 device matrices of at most ``row_block`` rows (pieces of
    ``_FLAT_BLOCK`` elements for what is not a matrix), in order."""
    rows, features = shape
    is_matrix = (len(x.shape) if hasattr(x, "shape")
                 else numpy.ndim(x)) == 2
    if is_matrix:
        take = _row_provider(x, device)
        for first in range(0, rows, row_block):
            yield take(first, min(first + row_block, rows))
    elif isinstance(x, torch.Tensor):
        flat = x.to(device).contiguous().view(-1)
        for first in range(0, features, _FLAT_BLOCK):
            yield flat[first:first + _FLAT_BLOCK].view(1, -1)
    else:
        flat = numpy.asarray(x).reshape(-1)
        for first in range(0, features, _FLAT_BLOCK):
            yield torch.from_numpy(numpy.ascontiguousarray(
                flat[first:first + _FLAT_BLOCK], dtype=numpy.float32)
            ).to(device).view(1, -1)


def csr_blocks(csr, row_block=ROW_BLOCK, first_row=0, last_row=None):
    """The rows of a ``DeviceCSR`` as dense fp32 blocks of at most
    ``row_block`` rows, through ``gather_dense`` into one buffer that every
    block reuses (a block is valid until the next one is asked for)."""
    rows, features = csr.shape
    last_row = rows if last_row is None else last_row
    buffer = torch.empty(min(row_block, max(last_row - first_row, 1)),
                         features, dtype=torch.float32, device=csr.device)
    for first in range(first_row, last_row, row_block):
        last = min(first + row_block, last_row)
        index = torch.arange(first, last, dtype=torch.int64,
                             device=csr.device)
        yield csr.gather_dense(index, out=buffer[:last - first])


def summary_statistics(x, name="", tolerance=1e-3, skip_sparsity=False,
                       device=None):
    """The reference's ``summary_statistics`` (``summary.py:27-57``) of ``x``:
    a NumPy array (any shape, all its values as with ``axis=None``; taken as
    fp32), a SciPy sparse matrix (densified on the device in row blocks) or
    an fp32 torch tensor on the device, which is read where it lies."""
    shape = _check_values(x, "Summary statistics")
    summary = DeviceSummary(tolerance, device=device)
    for block in _blocks(x, shape, summary.device, ROW_BLOCK):
        summary.add(original=block)
    return statistics_dictionary(name, *summary.finish()[0],
                                 skip_sparsity=skip_sparsity)


def comparison_statistics(original, reconstructed, tolerance=0.5,
                          extensive=False, names=("original", "reconstructed"),
                          device=None, row_block=ROW_BLOCK):
    """The rows of the metrics table of ``analyse_results``
    (``analyses.py:876-892``) from one pass: the statistics of ``original``
    and of ``reconstructed`` (two matrices of one shape: NumPy, fp32 device
    tensor or, for ``original``, SciPy sparse), and with ``extensive`` those
    of ``differences`` and ``log-ratios`` (no sparsity, as in the
    reference)."""
    shapes = [tuple(x.shape) if hasattr(x, "shape") else numpy.shape(x)
              for x in (original, reconstructed)]
    if len(shapes[0]) != 2 or shapes[0] != shapes[1]:
        raise ValueError(
            "Two matrices of one shape expected, got original values of "
            "shape {} and reconstructed values of shape {}.".format(*shapes))
    rows, _ = _check_values(original, "Original values")
    _check_values(reconstructed, "Reconstructed values")
    if _is_sparse(reconstructed):
        raise ValueError("Reconstructed values: a dense matrix expected.")
    if len(names) != 2:
        raise ValueError("Two names expected, got {}.".format(len(names)))
    row_block = int(row_block)
    if row_block < 1:
        raise ValueError("Row blocks of at least one row expected.")
    summary = DeviceSummary(tolerance, comparisons=extensive, device=device)
    take_original = _row_provider(original, summary.device)
    take_reconstructed = _row_provider(reconstructed, summary.device)
    for first in range(0, rows, row_block):
        last = min(first + row_block, rows)
        summary.add(reconstructed=take_reconstructed(first, last),
                    original=take_original(first, last))
    return _comparison_rows(summary.finish(), names, extensive)


def _comparison_rows(finished, names, extensive):
    rows = [statistics_dictionary(names[0], *finished[0]),
            statistics_dictionary(names[1], *finished[1])]
    if extensive:
        rows.append(statistics_dictionary(
            "differences", *finished[2], skip_sparsity=True))
        rows.append(statistics_dictionary(
            "log-ratios", *finished[3], skip_sparsity=True))
    return rows


def evaluation_statistics(csr, reconstructed, names, extensive=False,
                          tolerance=0.5, row_block=ROW_BLOCK):
    """What ``ModelBase.evaluate`` attaches: ``reconstructed`` (``[N, F]``
    fp32 on the device, read in place) against the rows of the ``DeviceCSR``
    the evaluation pass read, gathered block by block into one buffer."""
    summary = DeviceSummary(tolerance, comparisons=extensive,
                            device=reconstructed.device)
    first = 0
    for block in csr_blocks(csr, row_block):
        summary.add(reconstructed=reconstructed[first:first + block.shape[0]],
                    original=block)
        first += block.shape[0]
    return _comparison_rows(summary.finish(), names, extensive)


def format_summary_statistics(statistics_sets, name="Data set"):
    """The reference's table (``summary.py:60-93``), character for
    character."""
    if not isinstance(statistics_sets, list):
        statistics_sets = [statistics_sets]
    name_width = max([len(name)] + [len(s["name"]) for s in statistics_sets])
    rows = ["  ".join([
        "{:{}}".format(name, name_width), " mean ", "std. dev. ",
        "dispersion", " minimum ", " maximum ", "sparsity"])]
    for s in statistics_sets:
        rows.append("  ".join([
            "{:{}}".format(s["name"], name_width),
            "{:<9.5g}".format(s["mean"]),
            "{:<9.5g}".format(s["standard deviation"]),
            "{:<9.5g}".format(s["dispersion"]),
            "{:<11.5g}".format(s["minimum"]),
            "{:<11.5g}".format(s["maximum"]),
            "{:<7.5g}".format(s["sparsity"]),
        ]))
    return "\n".join(rows)
