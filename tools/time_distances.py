"""Time the device distances (``csrc/distances.hip``,
``analyses/distances.py``) beside scikit-learn on the host:
    python tools/time_distances.py [--skip-host] [--cases ...] [--out FILE]
One JSON line per case ``ROWSofNxF`` (ROWS rows drawn through an index from a
resident N x F matrix; default: 1000 and 10000 of 68579x32738, 10000 of
10000x25) and metric:

kernel_ms         one ``scvae_pairwise_distances`` call, both passes (device
                  events, mean of --launches calls after one warm-up)
peak_ms           the time the fp64 matrix peak would need for the FLOPs of the
                  tiles on or above the diagonal, 2 F n (n + 1) / 2, at
                  78.6 TFLOP/s (AMD's specification of the MI355X, "peak
                  double precision matrix (FP64) performance")
kernel_over_peak  their ratio
call_s            the whole ``pairwise_distances`` call on the resident matrix
                  through the index, to the fp32 matrix on the device (wall
                  clock, synchronised)
host_s            ``sklearn.metrics.pairwise_distances`` on the host for the
                  first ``host_rows`` rows of the sample (all of them where
                  --host-rows allows); ``host_s_extrapolated`` scales that by
                  (n / host_rows)^2 and is an extrapolation, not a measurement
"""
import argparse
import ctypes
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch

from scvae_amd import _lib
from scvae_amd.analyses import distances

FP64_MATRIX_PEAK_FLOPS = 78.6e12
DEFAULT_CASES = ["1000of68579x32738", "10000of68579x32738", "10000of10000x25"]


def synthetic(n, features, device, seed=0):
    """A reconstruction-like matrix: positive rates, 93 % of them a thousand
    times smaller than the rest."""
    generator = torch.Generator(device=device).manual_seed(seed)
    values = torch.empty(n, features, device=device)
    for first in range(0, n, 4096):
        block = values[first:first + 4096]
        block.exponential_(2.0, generator=generator)
        keep = torch.rand(block.shape, device=device, generator=generator)
        block.mul_(torch.where(keep < 0.07, 1.0, 1e-3))
    return values


def _p(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


def kernel_ms(values, index, metric, launches):
    lib = _lib.load()
    total_rows, features = values.shape
    n = index.numel()
    out = torch.empty(n, n, dtype=torch.float32, device=values.device)
    size = lib.scvae_pairwise_distances_workspace_bytes(n, features)
    workspace = torch.empty(size, dtype=torch.uint8, device=values.device)

    def call():
        _lib.check(lib.scvae_pairwise_distances(
            _p(values), values.stride(0), total_rows, features, _p(index), n,
            metric, _p(out), n, _p(workspace), size,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "scvae_pairwise_distances")

    call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(launches):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cases", nargs="+")
    parser.add_argument("--launches", type=int, default=3)
    parser.add_argument("--host-rows", type=int, default=2000)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--out")
    arguments = parser.parse_args()
    import sklearn.metrics
    device = torch.device("cuda:0")
    lines, values, shape = [], None, None
    for case in arguments.cases or DEFAULT_CASES:
        rows, of = case.split("of")
        rows = int(rows)
        n, features = (int(v) for v in of.split("x"))
        if shape != (n, features):
            del values
            torch.cuda.empty_cache()
            values, shape = synthetic(n, features, device), (n, features)
        sample = numpy.random.RandomState(57).permutation(n)[:rows]
        index = torch.from_numpy(sample).to(device)
        for metric in distances.DISTANCE_METRICS:
            flag = distances._metric_flag(metric)
            result = {"rows": rows, "of_cells": n, "features": features,
                      "metric": metric}
            result["kernel_ms"] = kernel_ms(values, index, flag,
                                            arguments.launches)
            result["peak_ms"] = (features * rows * (rows + 1.0)
                                 / FP64_MATRIX_PEAK_FLOPS * 1e3)
            result["kernel_over_peak"] = (result["kernel_ms"]
                                          / result["peak_ms"])
            torch.cuda.synchronize()
            start = time.perf_counter()
            got = distances.pairwise_distances(values, metric, rows=sample)
            torch.cuda.synchronize()
            result["call_s"] = time.perf_counter() - start
            del got
            if not arguments.skip_host:
                host_rows = min(rows, arguments.host_rows)
                host_values = values[index[:host_rows]].cpu().numpy()
                start = time.perf_counter()
                sklearn.metrics.pairwise_distances(
                    host_values, metric=metric.lower())
                result["host_rows"] = host_rows
                result["host_s"] = time.perf_counter() - start
                result["host_s_extrapolated"] = (
                    result["host_s"] * (rows / host_rows) ** 2)
                result["host_threads"] = int(os.environ["OMP_NUM_THREADS"])
            line = json.dumps(result)
            print(line, flush=True)
            lines.append(line)
            if arguments.out:
                with open(arguments.out, "w") as sink:
                    sink.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
