"""Time the count-space silhouette on the device beside what the reference
computes on the host, on synthetic counts (about 5 % non-zeros, K = 20):
    python tools/time_count_silhouette.py [--skip-host | --host-only]
        [--shapes NxF ...] [--limit SECONDS] [--out FILE]
One JSON line per shape:
  distance_ms    every strip of scvae_count_distances_u16 (device events
                 around the launches; the strips of the whole entry)
  bf16_roof_share / i8_roof_share
                 the matrix products issued, 4 byte products x 2 N^2 Fp
                 operations (Fp: the genes rounded up to 64), against the
                 dense bf16 rate of the chip, 2.5e15 a second, and against
                 the rate of the int8 instruction that issues them, twice
                 that
  entry_ms       scvae_count_silhouette_samples_u16 between two events
  reduction_ms   entry_ms - distance_ms: the strip reductions and the mean,
                 as the difference of two measurements that each spread by
                 about 1 % (the distance loop also repeats the row moments
                 once per strip): where the reductions are below that, the
                 difference is noise of either sign
  wrapper_s      count_silhouette_score from the scipy matrix to the float
  host_s         sklearn.metrics.silhouette_score on the same rows with 16
                 threads, once
Every shape runs in a child process of its own under --limit seconds; the
first one that fails or runs out of time ends the run: nothing is tried
again."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import scipy.sparse

DENSE_BF16_OPERATIONS_PER_SECOND = 2.5e15
CLUSTERS = 20
DEFAULT_SHAPES = ["20000x32738", "5000x32738", "20000x2000"]


def counts(n, features, k=CLUSTERS, density=0.05, seed=0):
    """(scipy CSR fp32 [n, features] of integer counts, labels): every cell
    draws half of its genes from the block of its cluster."""
    rng = numpy.random.default_rng(seed)
    labels = rng.integers(k, size=n)
    labels[:k] = numpy.arange(k)
    per_row = max(1, int(features * density))
    block = max(1, features // k)
    genes = rng.integers(features, size=(n, per_row))
    own = (labels[:, None] * block
           + rng.integers(block, size=(n, per_row // 2))) % features
    genes[:, :per_row // 2] = own
    data = (1 + rng.poisson(1.0, size=n * per_row)).astype(numpy.float32)
    matrix = scipy.sparse.csr_matrix(
        (data, genes.reshape(-1), numpy.arange(n + 1) * per_row),
        shape=(n, features))
    matrix.sum_duplicates()
    matrix.sort_indices()
    return matrix, labels


def time_device(matrix, labels, launches):
    import torch
    from scvae_amd import _lib
    from scvae_amd.analyses import count_silhouette
    lib = _lib.load()
    device = torch.device("cuda:0")
    n, features = matrix.shape
    k = CLUSTERS
    order = numpy.argsort(labels, kind="stable")
    offsets = torch.from_numpy(numpy.concatenate(
        [[0], numpy.cumsum(numpy.bincount(labels, minlength=k))]).astype(
            numpy.int64)).to(device)
    pitch = count_silhouette.row_pitch(features)
    xd = torch.zeros((n, pitch), dtype=torch.int16, device=device)
    for first in range(0, n, 2048):      # (counts far below 2^15)
        rows = matrix[order[first:first + 2048]].toarray().astype(numpy.int16)
        xd[first:first + len(rows), :features] = torch.from_numpy(rows).to(
            device)
    nbytes = lib.scvae_count_silhouette_workspace_bytes(n, features, k)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    fixed = 8 * n + (4 * n + 7) // 8 * 8
    ldd = (n + 15) // 16 * 16
    strip = min(n, (nbytes - fixed) // (4 * ldd))
    d = torch.empty((strip, ldd), dtype=torch.float32, device=device)
    s = torch.empty(n, dtype=torch.float32, device=device)
    score = torch.zeros(1, dtype=torch.float64, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def distances():
        for i0 in range(0, n, strip):
            _lib.check(lib.scvae_count_distances_u16(
                xd.data_ptr(), pitch, n, features, i0, min(strip, n - i0),
                d.data_ptr(), ldd, workspace.data_ptr(), nbytes, stream),
                "scvae_count_distances_u16")

    def entry():
        _lib.check(lib.scvae_count_silhouette_samples_u16(
            xd.data_ptr(), pitch, n, features, offsets.data_ptr(), k, None,
            None, s.data_ptr(), score.data_ptr(), workspace.data_ptr(),
            nbytes, stream), "scvae_count_silhouette_samples_u16")

    def timed(function):
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        start.record()
        for _ in range(launches):
            function()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / launches
    # (the first launches of a process pay for loading the code object and
    # for the clocks coming up)
    entry()
    torch.cuda.synchronize()
    entry_ms = timed(entry)
    distance_ms = timed(distances)
    padded = (features + 63) // 64 * 64
    operations = 4 * 2.0 * n * n * padded
    result = {
        "distance_ms": distance_ms, "entry_ms": entry_ms,
        "reduction_ms": entry_ms - distance_ms, "launches": launches,
        "strip_rows": int(strip), "score": float(score.item()),
        "matrix_operations": operations,
        "bf16_roof_share": operations / DENSE_BF16_OPERATIONS_PER_SECOND
        / (distance_ms * 1e-3),
        "i8_roof_share": operations / (2 * DENSE_BF16_OPERATIONS_PER_SECOND)
        / (distance_ms * 1e-3)}
    del xd, d, workspace
    torch.cuda.synchronize()
    start = time.perf_counter()
    wrapped = count_silhouette.count_silhouette_score(
        matrix, labels, device=device)
    result["wrapper_s"] = time.perf_counter() - start
    assert wrapped == result["score"], (wrapped, result["score"])
    return result


def one_shape(shape, skip_host, host_only, launches):
    n, features = (int(v) for v in shape.split("x"))
    matrix, labels = counts(n, features)
    result = {"cells": n, "genes": features, "clusters": CLUSTERS,
              "non_zeros": int(matrix.nnz)}
    if not host_only:
        result.update(time_device(matrix, labels, launches))
    if not skip_host:
        import sklearn.metrics
        start = time.perf_counter()
        host = sklearn.metrics.silhouette_score(X=matrix, labels=labels)
        result["host_s"] = time.perf_counter() - start
        result["host_score"] = float(host)
        if "entry_ms" in result:
            result["host_over_wrapper"] = (
                result["host_s"] / result["wrapper_s"])
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES)
    parser.add_argument("--launches", type=int, default=2)
    parser.add_argument("--limit", type=float, default=420.0)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--host-only", action="store_true")
    parser.add_argument("--out")
    parser.add_argument("--one", help=argparse.SUPPRESS)
    arguments = parser.parse_args()
    if arguments.one:
        print(json.dumps(one_shape(arguments.one, arguments.skip_host,
                                   arguments.host_only, arguments.launches)),
              flush=True)
        return 0
    lines = []
    for shape in arguments.shapes:
        command = [sys.executable, os.path.abspath(__file__), "--one", shape,
                   "--launches", str(arguments.launches)]
        command += ["--skip-host"] if arguments.skip_host else []
        command += ["--host-only"] if arguments.host_only else []
        try:
            done = subprocess.run(command, stdout=subprocess.PIPE, text=True,
                                  timeout=arguments.limit)
        except subprocess.TimeoutExpired:
            print("{}: not done within {} s; stopping.".format(
                shape, arguments.limit), flush=True)
            return 1
        if done.returncode != 0:
            print("{}: exit status {}; stopping.".format(
                shape, done.returncode), flush=True)
            return 1
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if arguments.out:
            with open(arguments.out, "w") as sink:
                sink.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
