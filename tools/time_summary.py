"""Time the device summary statistics beside what the reference computes on
the host, on a synthetic reconstruction and a synthetic sparse count matrix:
    python tools/time_summary.py [--skip-host] [--shapes NxF ...] [--out FILE]
One JSON line per shape and level (normal: two rows; extensive: four):

kernel_ms     the accumulate launches alone between two device events, over
              the reconstruction where it lies and ONE dense block of original
              rows used again for every block (mean of --launches passes);
              kernel_floor_ms = the bytes those launches read, 2 x 4 N F,
              over the HBM rate a float4 copy reaches, 6.29 TB/s
pass_ms       what ``evaluate`` runs: every block of original rows gathered
              out of the CSR matrix into one buffer, then the launch (wall
              clock around ``evaluation_statistics``); pass_floor_ms = its
              4 N F read of the reconstruction, 4 N F written and 4 N F read
              again of the original rows, over the same rate
host_s        NumPy as ``analyses/metrics/summary.py`` does it on the
              reconstruction copied to the host (fp32 ``mean``, the batched
              ``E[x^2] - E[x]^2`` above 5e8 values, ``min``, ``max``, the
              batched sparsity) and, for extensive, on the two dense
              comparison arrays of ``analyses.py:796-802``; only where the
              host has the memory for it, and the extensive rows only up to
              5e8 values (--host-above lifts both checks)
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch

from scvae_amd.analyses import summary
from scvae_amd.minibatch import DeviceCSR

HBM_BYTES_PER_SECOND = 6.29e12
DEFAULT_SHAPES = ["4096x2000", "68579x32738"]
MAXIMUM_NUMBER_OF_VALUES_FOR_NORMAL_STATISTICS_COMPUTATION = 5e8


def synthetic(n, features, device, density=0.07, seed=0):
    """(reconstruction [N, F] fp32 on the device, DeviceCSR of counts with
    ``density`` of its values non-zero, the same columns shifted row by
    row)."""
    generator = torch.Generator(device=device).manual_seed(seed)
    recon = torch.empty(n, features, device=device)
    for first in range(0, n, 4096):
        block = recon[first:first + 4096]
        block.exponential_(2.0, generator=generator)
    per_row = max(1, int(features * density))
    stride = features // per_row
    columns = torch.arange(per_row, device=device, dtype=torch.int32) * stride
    shift = (torch.arange(n, device=device, dtype=torch.int32) % stride)
    indices = (columns[None, :] + shift[:, None]).reshape(-1)
    values = torch.randint(1, 9, (n * per_row,), device=device,
                           generator=generator).to(torch.float32)
    indptr = torch.arange(n + 1, device=device, dtype=torch.int64) * per_row
    return recon, DeviceCSR(indptr, indices, values, (n, features), device)


def time_kernel(recon, block, extensive, launches):
    device = recon.device
    state = summary.DeviceSummary(0.5, comparisons=extensive, device=device)
    n = recon.shape[0]
    rows = block.shape[0]

    def one_pass():
        state.reset()
        for first in range(0, n, rows):
            piece = recon[first:first + rows]
            state.add(reconstructed=piece, original=block[:piece.shape[0]])
    one_pass()
    start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(launches):
        one_pass()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def host_available_bytes():
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return 0


def reference_statistics(x, tolerance, skip_sparsity=False):
    """``summary_statistics`` of the reference on a dense array, with its
    batched variance and sparsity above 5e8 values."""
    batch = (1000 if x.size
             > MAXIMUM_NUMBER_OF_VALUES_FOR_NORMAL_STATISTICS_COMPUTATION
             else None)
    mean = x.mean()
    if batch is None:
        std = numpy.sqrt(x.var(ddof=1))
    else:
        squared_sum = 0
        for i in range(0, x.shape[0], batch):
            squared_sum += numpy.power(x[i:i + batch], 2).sum()
        variance = squared_sum / x.size - numpy.power(x.mean(), 2)
        std = numpy.sqrt(variance * x.size / (x.size - 1))
    lowest, highest = x.min(), x.max()
    if skip_sparsity:
        return mean, std, lowest, highest, numpy.nan
    if batch is None:
        nonzero = (x >= tolerance).sum()
    else:
        nonzero = 0
        for i in range(0, x.shape[0], batch):
            nonzero += (x[i:i + batch] >= tolerance).sum()
    return mean, std, lowest, highest, 1 - nonzero / x.size


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+")
    parser.add_argument("--launches", type=int, default=3)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--host-above", action="store_true",
                        help="run the host column whatever memory is free")
    parser.add_argument("--out")
    arguments = parser.parse_args()
    device = torch.device("cuda:0")
    lines = []
    warm = synthetic(512, 300, device)
    summary.evaluation_statistics(warm[1], warm[0], ("o", "r"), True)
    for shape in arguments.shapes or DEFAULT_SHAPES:
        n, features = (int(v) for v in shape.split("x"))
        recon, csr = synthetic(n, features, device)
        block = next(summary.csr_blocks(csr)).clone()
        values = float(n) * features
        host_recon = host_orig = None
        need = 3 * 4 * values
        if not arguments.skip_host and (
                arguments.host_above or host_available_bytes() > need * 1.5):
            host_recon = recon.cpu().numpy()
        for extensive in (False, True):
            result = {"cells": n, "features": features,
                      "level": "extensive" if extensive else "normal"}
            result["kernel_ms"] = time_kernel(recon, block, extensive,
                                              arguments.launches)
            result["kernel_floor_ms"] = (
                2 * 4 * values / HBM_BYTES_PER_SECOND * 1e3)
            result["kernel_over_floor"] = (
                result["kernel_ms"] / result["kernel_floor_ms"])
            torch.cuda.synchronize()
            start = time.perf_counter()
            rows = summary.evaluation_statistics(
                csr, recon, ("original", "reconstructed"), extensive)
            result["pass_ms"] = (time.perf_counter() - start) * 1e3
            result["pass_floor_ms"] = (
                3 * 4 * values / HBM_BYTES_PER_SECOND * 1e3)
            result["pass_over_floor"] = (
                result["pass_ms"] / result["pass_floor_ms"])
            result["reconstructed"] = {
                k: rows[1][k] for k in ("mean", "standard deviation",
                                        "sparsity")}
            host_extensive = extensive and (
                arguments.host_above or values
                <= MAXIMUM_NUMBER_OF_VALUES_FOR_NORMAL_STATISTICS_COMPUTATION)
            if host_recon is not None and (host_extensive or not extensive):
                if extensive and host_orig is None:
                    host_orig = numpy.empty_like(host_recon)
                    for first in range(0, n, summary.ROW_BLOCK):
                        last = min(first + summary.ROW_BLOCK, n)
                        host_orig[first:last] = next(summary.csr_blocks(
                            csr, first_row=first, last_row=last)).cpu().numpy()
                start = time.perf_counter()
                host = reference_statistics(host_recon, 0.5)
                if extensive:
                    x_diff = host_recon - host_orig
                    x_log_ratio = (numpy.log1p(host_recon)
                                   - numpy.log1p(host_orig))
                    reference_statistics(numpy.abs(x_diff), 1e-3, True)
                    reference_statistics(numpy.abs(x_log_ratio), 1e-3, True)
                    del x_diff, x_log_ratio
                result["host_s"] = time.perf_counter() - start
                result["host_rows"] = "reconstructed" + (
                    ", differences, log-ratios" if extensive else "")
                result["host_reconstructed"] = {
                    "mean": float(host[0]), "standard deviation":
                    float(host[1]), "sparsity": float(host[4])}
                result["host_over_pass"] = (
                    result["host_s"] / (result["pass_ms"] * 1e-3))
            line = json.dumps(result)
            print(line, flush=True)
            lines.append(line)
            if arguments.out:
                with open(arguments.out, "w") as sink:
                    sink.write("\n".join(lines) + "\n")
        del recon, csr, block, host_recon, host_orig
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
