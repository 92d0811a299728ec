"""Time the device k-means beside the scikit-learn path `-P k-means` takes
without --prediction-on-device, on synthetic latent values:
    python tools/time_kmeans.py [--skip-host] [--shapes NxLxK ...] [--out FILE]
One JSON line per shape: the device fit + predict (n_init=10, k-means++), one
Lloyd iteration (assign and update kernels, mean of --launches launches) and
that time as a multiple of reading X once at 6.3 TB/s, and the host fit +
predict with 16 threads (KMeans up to 10 000 cells, MiniBatchKMeans above)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch

from scvae_amd.analyses.kmeans import DeviceKMeans
from scvae_amd.analyses.prediction import _predict_using_kmeans

HBM_BYTES_PER_SECOND = 6.3e12
DEFAULT_SHAPES = ["68579x25x20", "1306127x100x20", "8192x32x256"]


class LatentSet:
    def __init__(self, values):
        self.values = values
        self.number_of_examples = values.shape[0]


def latents(n, latent_size, k, seed=0):
    rng = numpy.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((k, latent_size))
    labels = rng.integers(k, size=n)
    x = centres[labels].astype(numpy.float32)
    x += rng.standard_normal((n, latent_size), dtype=numpy.float32)
    return x


def time_kernels(model, x, launches):
    k = model.n_clusters
    device = x.device
    centres = torch.from_numpy(model.cluster_centers_).to(device)
    new = torch.empty_like(centres)
    labels = torch.empty(x.shape[0], dtype=torch.int32, device=device)
    counts = torch.empty(k, dtype=torch.int32, device=device)
    scalars = torch.zeros(2, dtype=torch.float64, device=device)
    workspace = model._workspace(x.shape[0], x.shape[1])

    def assign():
        model._assign(x, centres, labels, scalars[0:1], workspace)

    def update():
        model._update(x, labels, centres, new, counts, scalars[1:2],
                      workspace)
    out = {}
    for name, call in (("assign", assign), ("update", update)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        start.record()
        for _ in range(launches):
            call()
        stop.record()
        torch.cuda.synchronize()
        out[name + "_us"] = start.elapsed_time(stop) / launches * 1e3
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES)
    parser.add_argument("--launches", type=int, default=20)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--out")
    arguments = parser.parse_args()
    lines = []
    for shape in arguments.shapes:
        n, latent_size, k = (int(v) for v in shape.split("x"))
        x = latents(n, latent_size, k)
        result = {"cells": n, "latent_size": latent_size, "clusters": k}
        DeviceKMeans(k, n_init=1, max_iter=2, seed=0).fit(x[:max(k, 1000)])
        torch.cuda.synchronize()
        start = time.perf_counter()
        model = DeviceKMeans(k, seed=0).fit(x)
        fitted = time.perf_counter()
        model.predict(x)
        result["device_fit_s"] = fitted - start
        result["device_predict_s"] = time.perf_counter() - fitted
        result["device_winning_run_iterations"] = model.n_iter_
        result["device_inertia"] = model.inertia_
        xd = torch.from_numpy(x).to(model._device)
        result.update(time_kernels(model, xd, arguments.launches))
        read_us = 4.0 * n * latent_size / HBM_BYTES_PER_SECOND * 1e6
        result["read_x_once_us"] = read_us
        result["iteration_us"] = result["assign_us"] + result["update_us"]
        result["iteration_over_two_reads"] = (
            result["iteration_us"] / (2 * read_us))
        result["assign_over_one_read"] = result["assign_us"] / read_us
        result["update_over_one_read"] = result["update_us"] / read_us
        del xd
        if not arguments.skip_host:
            sets = LatentSet(x), LatentSet(x)
            start = time.perf_counter()
            _predict_using_kmeans(*sets, number_of_clusters=k)
            result["host_fit_predict_s"] = time.perf_counter() - start
            result["host_method"] = (
                "KMeans(n_init=10)" if n <= 10000
                else "MiniBatchKMeans(batch_size=100, n_init=3)")
        line = json.dumps(result)
        print(line, flush=True)
        lines.append(line)
        if arguments.out:
            with open(arguments.out, "w") as sink:
                sink.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
