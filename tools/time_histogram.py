"""Time the device distributions (``csrc/histogram.hip``,
``analyses/distributions.py``) beside the reference's formulation on the host:
    python tools/time_histogram.py [--skip-host] [--shapes NxF ...] [--out FILE]
One JSON line per shape and value pattern (``uniform``; ``reconstruction``:
93 % of the rates a thousand times smaller than the rest; ``one-bin``: 95 %
exact zeros):

floor_ms          the time to read the matrix once, 4 N F bytes over the HBM
                  rate a float4 copy reaches, 6.29 TB/s
select_ms         one ``scvae_order_statistics`` call for the four ranks of
                  the two quartiles: the three radix passes and the picks
                  between them (device events, mean of --launches calls)
histogram_ms      one ``scvae_histogram_accumulate`` call at 20 000 bins and at
                  the bins ``"auto"`` chooses, with their slab counts (a slab
                  is one pass over the matrix); ``*_plain_ms`` the same with the
                  aggregation of equal bins inside a wave switched off
row_sums_ms       one ``scvae_row_sums_f64`` call
evaluation_s      the whole ``evaluation_distributions`` call at the normal
                  level (wall clock to the results on the host); left out
                  where ``"auto"`` asks for more bins than the device takes:
                  the call then goes to the host like the reference
                  (--allow-host runs it all the same)
host_s            the reference's formulation on the first --host-rows rows on
                  the host: the copy of the flattened series, ``min`` / ``max``,
                  ``numpy.histogram(bins="auto")``, the same on ``series + 1``,
                  and the fp32 row sums with their histogram
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

from scvae_amd.analyses import distributions

HBM_BYTES_PER_SECOND = 6.29e12
DEFAULT_SHAPES = ["4096x2000", "68579x32738"]
PATTERNS = ("uniform", "reconstruction", "one-bin")
SLAB = 8192


def synthetic(pattern, n, features, device, seed=0):
    generator = torch.Generator(device=device).manual_seed(seed)
    values = torch.empty(n, features, device=device)
    for first in range(0, n, 4096):
        block = values[first:first + 4096]
        if pattern == "uniform":
            block.uniform_(0.0, 30.0, generator=generator)
            continue
        block.exponential_(2.0, generator=generator)
        keep = torch.rand(block.shape, device=device, generator=generator)
        if pattern == "reconstruction":
            block.mul_(torch.where(keep < 0.07, 1.0, 1e-3))
        else:
            block.mul_(keep < 0.05)
    return values


def timed(call, launches):
    call()
    start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(launches):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def automatic_bins(series):
    minimum, maximum, quartile_values = series.statistics()
    first, last = distributions.outer_edges(minimum, maximum)
    percentiles = [
        distributions.percentile_from_order_statistics(
            quartile_values[2 * i], quartile_values[2 * i + 1],
            distributions.percentile_ranks(series.size, q)[2])
        for i, q in enumerate((75, 25))]
    return distributions.automatic_number_of_bins(
        series.size, minimum, maximum, first, last, *percentiles), first, last


def host_reference(values):
    """``plot_histogram`` twice and the count sums, as the reference runs
    them (``histograms.py:129-171``, ``subanalyses.py:119-192``)."""
    start = time.perf_counter()
    for log_values in (False, True):
        series = values.reshape(-1).copy()
        bin_range = numpy.array((series.min(), series.max()))
        if log_values:
            series += 1
            bin_range += 1
        numpy.histogram(series, bins="auto", range=bin_range)
    count_sum = values.sum(axis=1).reshape(-1).copy()
    numpy.histogram(count_sum, bins="auto",
                    range=numpy.array((count_sum.min(), count_sum.max())))
    return time.perf_counter() - start


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+")
    parser.add_argument("--patterns", nargs="+", default=list(PATTERNS))
    parser.add_argument("--launches", type=int, default=3)
    parser.add_argument("--host-rows", type=int, default=4000)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--allow-host", action="store_true")
    parser.add_argument("--out")
    arguments = parser.parse_args()
    device = torch.device("cuda:0")
    lines = []
    distributions.distribution_histograms(
        synthetic("uniform", 512, 300, device))
    for shape in arguments.shapes or DEFAULT_SHAPES:
        n, features = (int(v) for v in shape.split("x"))
        for pattern in arguments.patterns:
            values = synthetic(pattern, n, features, device)
            series = distributions._DeviceSeries(values)
            floor_ms = 4.0 * n * features / HBM_BYTES_PER_SECOND * 1e3
            result = {"cells": n, "features": features, "pattern": pattern,
                      "floor_ms": floor_ms}
            ranks = []
            for q in (75, 25):
                ranks.extend(distributions.percentile_ranks(series.size, q)[:2])
            result["select_ms"] = timed(
                lambda: series.order_statistics(ranks), arguments.launches)
            result["select_over_floor"] = result["select_ms"] / floor_ms
            bins, first, last = automatic_bins(series)
            result["auto_bins"] = bins
            cases = [("20000", 20000)]
            if bins <= distributions.MAXIMUM_NUMBER_OF_BINS_ON_DEVICE:
                cases.append(("auto", bins))
            for label, number in cases:
                edges = distributions.bin_edges(number, first, last)
                slabs = -(-number // SLAB)
                for aggregate, suffix in ((True, ""), (False, "_plain")):
                    key = "histogram_{}{}".format(label, suffix)
                    result[key + "_ms"] = timed(
                        lambda: series.count(edges, aggregate=aggregate),
                        arguments.launches)
                    result[key + "_over_floor"] = result[key + "_ms"] / floor_ms
                result["histogram_{}_slabs".format(label)] = slabs
            result["row_sums_ms"] = timed(series.row_sums, arguments.launches)
            result["row_sums_over_floor"] = result["row_sums_ms"] / floor_ms
            if (bins <= distributions.MAXIMUM_NUMBER_OF_BINS_ON_DEVICE
                    or arguments.allow_host):
                torch.cuda.synchronize()
                start = time.perf_counter()
                histograms = distributions.evaluation_distributions(
                    None, values)
                result["evaluation_s"] = time.perf_counter() - start
                result["evaluation_over_floor"] = (
                    result["evaluation_s"] * 1e3 / floor_ms)
                result["evaluation_bins"] = [
                    int(h["counts"].size) for h in histograms]
            if not arguments.skip_host:
                rows = min(n, arguments.host_rows)
                host_values = values[:rows].cpu().numpy()
                result["host_rows"] = rows
                result["host_s"] = host_reference(host_values)
                result["host_s_extrapolated_to_all_rows"] = (
                    result["host_s"] * n / rows)
            line = json.dumps(result)
            print(line, flush=True)
            lines.append(line)
            if arguments.out:
                with open(arguments.out, "w") as sink:
                    sink.write("\n".join(lines) + "\n")
            del values, series
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
