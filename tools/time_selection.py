"""Time the feature selection on the device beside the host path of this
build and the reference's formulation, on a synthetic sparse count matrix:
    python tools/time_selection.py [--shapes NxF ...] [--keep K] [--out FILE]
One JSON line per shape (default 68 579 x 32 738, about 5 % non-zero,
``keep_highest_variances 5000``):

moments_ms    ``scvae_csr_feature_moments`` alone between two device events
              (mean of --launches launches); moments_floor_ms = the 8 bytes of
              every stored entry (column index and value) read once, over the
              HBM rate a float4 copy reaches, 6.29 TB/s; moments_read_ms = the
              bytes the kernel does read (the column indices once per slab of
              8192 genes, the values once) over the same rate
count_ms,     ``scvae_csr_submatrix_count`` and ``_fill`` alone for the column
fill_ms       map of the selection; submatrix_floor_ms = indices read twice,
              values once, the kept entries written, over the same rate
device_s      ``select_features(..., on_device=True)``: upload of the CSR,
              kernels, the selection rule on the host, download of the result
              (wall clock, best of --calls)
host_s        ``select_features(..., on_device=False)``: this build's host path
reference_s   the reference's formulation written out here: fp32
              ``E[x^2] - E[x]^2`` over the CSR (``SparseRowMatrix.var(axis=0)``),
              ``numpy.argsort`` and SciPy's ``values[:, indices]``
reference_differs  genes that the reference's formulation selects and the
              exact rule does not
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import scipy.sparse
import torch

from scvae_amd import _lib
from scvae_amd.data import processing
from scvae_amd.data.sparse import SparseRowMatrix

HBM_BYTES_PER_SECOND = 6.29e12
DEFAULT_SHAPES = ["68579x32738"]
SLAB = 8192


def synthetic(n, features, density=0.05, seed=0):
    """A canonical CSR count matrix with ``density`` of its values stored: the
    same columns shifted row by row, counts whose spread differs from gene to
    gene."""
    generator = numpy.random.default_rng(seed)
    per_row = max(1, int(features * density))
    stride = features // per_row
    columns = numpy.arange(per_row, dtype=numpy.int32) * stride
    shift = (numpy.arange(n, dtype=numpy.int32) % stride)
    indices = (columns[None, :] + shift[:, None]).reshape(-1)
    top = 2 + (indices % 23).astype(numpy.float32)
    values = numpy.floor(
        1 + generator.random(indices.size, dtype=numpy.float32) * top)
    indptr = numpy.arange(n + 1, dtype=numpy.int64) * per_row
    matrix = scipy.sparse.csr_matrix(
        (values.astype(numpy.float32), indices, indptr), shape=(n, features))
    matrix.has_sorted_indices = True
    matrix.has_canonical_format = True
    return matrix


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr() if tensor is not None else None)


def events(function, launches):
    function()
    start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(launches):
        function()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def time_kernels(matrix, selected, launches, device):
    lib = _lib.load()
    n, features = matrix.shape
    uploaded = processing._DeviceMatrix(matrix, device)
    results = torch.empty(3, features, dtype=torch.int64, device=device)
    bad = torch.zeros(1, dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def moments():
        _lib.check(lib.scvae_csr_feature_moments(
            _ptr(uploaded.indptr), _ptr(uploaded.indices),
            _ptr(uploaded.values), n, features, _ptr(results[0]),
            _ptr(results[1]), _ptr(results[2]), _ptr(bad), stream), "moments")
    out = {"moments_ms": events(moments, launches)}

    host_map = numpy.full(features, -1, dtype=numpy.int32)
    host_map[selected] = numpy.arange(len(selected), dtype=numpy.int32)
    column_map = torch.from_numpy(host_map).to(device)
    counts = torch.empty(n, dtype=torch.int64, device=device)
    out_indptr = torch.zeros(n + 1, dtype=torch.int64, device=device)

    def count():
        _lib.check(lib.scvae_csr_submatrix_count(
            _ptr(uploaded.indptr), _ptr(uploaded.indices), n, features, None,
            n, _ptr(column_map), _ptr(counts), _ptr(bad), stream), "count")
    out["count_ms"] = events(count, launches)
    torch.cumsum(counts, dim=0, out=out_indptr[1:])
    kept = int(out_indptr[-1].item())
    out_indices = torch.empty(kept, dtype=torch.int32, device=device)
    out_values = torch.empty(kept, dtype=torch.float32, device=device)

    def fill():
        _lib.check(lib.scvae_csr_submatrix_fill(
            _ptr(uploaded.indptr), _ptr(uploaded.indices),
            _ptr(uploaded.values), n, features, None, n, _ptr(column_map),
            _ptr(out_indptr), _ptr(out_indices), _ptr(out_values), _ptr(bad),
            stream), "fill")
    out["fill_ms"] = events(fill, launches)
    assert int(bad.item()) == 0
    stored = matrix.nnz
    slabs = (features + SLAB - 1) // SLAB
    out["stored_entries"] = stored
    out["kept_entries"] = kept
    out["moments_floor_ms"] = 8 * stored / HBM_BYTES_PER_SECOND * 1e3
    out["moments_read_ms"] = (
        (4 * slabs + 4) * stored / HBM_BYTES_PER_SECOND * 1e3)
    out["submatrix_floor_ms"] = (
        (12 * stored + 8 * kept) / HBM_BYTES_PER_SECOND * 1e3)
    return out


def wall(function, calls):
    best = None
    for _ in range(calls):
        torch.cuda.synchronize()
        start = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            result = function()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - start
        best = elapsed if best is None else min(best, elapsed)
    return best, result


def reference_formulation(matrix, keep):
    """``processing.py:124-133, 151`` of the reference with the ``var`` of its
    ``SparseRowMatrix`` (``sparse.py:51-62``)."""
    values = SparseRowMatrix(matrix)
    variances = values.var(axis=0)
    if isinstance(variances, numpy.matrix):
        variances = variances.A.squeeze()
    indices = numpy.sort(numpy.argsort(variances)[-keep:])
    return values[:, indices], indices


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+")
    parser.add_argument("--keep", type=int, default=5000)
    parser.add_argument("--launches", type=int, default=5)
    parser.add_argument("--calls", type=int, default=2)
    parser.add_argument("--out")
    arguments = parser.parse_args()
    device = torch.device("cuda:0")
    lines = []
    warm = synthetic(300, 900)
    processing.feature_moments(warm, on_device=True)
    for shape in arguments.shapes or DEFAULT_SHAPES:
        n, features = (int(v) for v in shape.split("x"))
        keep = min(arguments.keep, features - 1)
        matrix = synthetic(n, features)
        names = numpy.arange(features)
        result = {"cells": n, "features": features, "keep": keep}

        def select(on_device):
            return processing.select_features(
                {"original": matrix}, names, method="keep_highest_variances",
                parameters=[keep], on_device=on_device)
        result["device_s"], on_device = wall(lambda: select(True),
                                             arguments.calls)
        result["host_s"], on_host = wall(lambda: select(False),
                                         arguments.calls)
        result["device_equals_host"] = bool(
            on_device[1].tolist() == on_host[1].tolist()
            and all(numpy.array_equal(getattr(on_device[0]["original"], a),
                                      getattr(on_host[0]["original"], a))
                    for a in ("indptr", "indices", "data")))
        result["reference_s"], reference = wall(
            lambda: reference_formulation(matrix, keep), arguments.calls)
        result["reference_differs"] = int(
            len(set(reference[1].tolist()) - set(on_host[1].tolist())))
        result.update(time_kernels(matrix, on_host[1], arguments.launches,
                                   device))
        result["moments_over_floor"] = (
            result["moments_ms"] / result["moments_floor_ms"])
        result["host_over_device"] = result["host_s"] / result["device_s"]
        line = json.dumps(result)
        print(line, flush=True)
        lines.append(line)
        if arguments.out:
            with open(arguments.out, "w") as sink:
                sink.write("\n".join(lines) + "\n")
        del matrix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
