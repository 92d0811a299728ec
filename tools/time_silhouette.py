"""Time the device silhouette beside what the reference computes on the host,
on synthetic latent values:
    python tools/time_silhouette.py [--skip-host] [--shapes NxLxK ...] [--out FILE]
One JSON line per shape: the kernel launch (device events around
scvae_silhouette_samples, mean of --launches launches), its pair rate, the
bound it is judged by -- N^2 pairs x L coordinates x 2 fp32 vector
instructions (subtract, fused multiply-add) at the chip's fp32 vector rate,
157.3 TFLOPS = 78.65e12 lane-instructions a second, which takes the packed
two-wide instructions -- the whole wrapper call, and the host column:
scikit-learn's silhouette_score with 16 threads as the reference calls it,
sampled down to 20 000 cells above 20 000.  The last default shape runs only
if the pair rate measured before it says it ends within --largest-within
seconds."""
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
from scvae_amd.analyses import silhouette

FP32_VECTOR_LANE_INSTRUCTIONS_PER_SECOND = 157.3e12 / 2
HOST_SAMPLE = 20000
DEFAULT_SHAPES = ["68579x25x20", "20000x25x20", "262144x100x20"]
LARGEST_SHAPE = "1306127x100x20"


def latents(n, latent_size, k, seed=0):
    rng = numpy.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((k, latent_size))
    labels = rng.integers(k, size=n)
    labels[:k] = numpy.arange(k)
    x = centres[labels].astype(numpy.float32)
    x += rng.standard_normal((n, latent_size), dtype=numpy.float32)
    return x, labels


def time_kernel(x, labels, k, launches, device):
    """(milliseconds a launch, the score): rows grouped by cluster on the
    device, then the entry alone between two events."""
    lib = _lib.load()
    n, latent_size = x.shape
    order = torch.sort(torch.from_numpy(labels).to(device), stable=True)[1]
    xd = torch.from_numpy(x).to(device)[order].contiguous()
    counts = numpy.bincount(labels, minlength=k)
    offsets = torch.from_numpy(numpy.concatenate(
        [[0], numpy.cumsum(counts)]).astype(numpy.int64)).to(device)
    nbytes = lib.scvae_silhouette_workspace_bytes(n, latent_size, k)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    s = torch.empty(n, dtype=torch.float32, device=device)
    score = torch.zeros(1, dtype=torch.float64, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def launch():
        _lib.check(lib.scvae_silhouette_samples(
            xd.data_ptr(), xd.stride(0), n, latent_size, offsets.data_ptr(),
            k, None, None, s.data_ptr(), score.data_ptr(),
            workspace.data_ptr(), nbytes, stream), "scvae_silhouette_samples")
    start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(launches):
        launch()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches, float(score.item())


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+")
    parser.add_argument("--launches", type=int, default=3)
    parser.add_argument("--largest-within", type=float, default=60.0)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--out")
    arguments = parser.parse_args()
    device = torch.device("cuda:0")
    shapes = arguments.shapes or DEFAULT_SHAPES + [LARGEST_SHAPE]
    # the first launch of a process pays for loading the code object
    warm = latents(4096, 25, 20)
    time_kernel(warm[0], warm[1], 20, 1, device)
    lines = []
    slowest_pair_lane_rate = None
    for shape in shapes:
        n, latent_size, k = (int(v) for v in shape.split("x"))
        work = float(n) * n * latent_size * 2
        result = {"cells": n, "latent_size": latent_size, "clusters": k}
        if not arguments.shapes and shape == LARGEST_SHAPE:
            expected = work / slowest_pair_lane_rate
            result["expected_s"] = expected
            if expected > arguments.largest_within:
                result["skipped"] = "expected above {} s".format(
                    arguments.largest_within)
                print(json.dumps(result), flush=True)
                continue
        x, labels = latents(n, latent_size, k)
        launches = arguments.launches if work < 1e13 else 1
        ms, score = time_kernel(x, labels, k, launches, device)
        bound_ms = work / FP32_VECTOR_LANE_INSTRUCTIONS_PER_SECOND * 1e3
        rate = work / (ms * 1e-3)
        if slowest_pair_lane_rate is None or rate < slowest_pair_lane_rate:
            slowest_pair_lane_rate = rate
        result.update({
            "kernel_ms": ms, "launches": launches, "score": score,
            "pairs_per_second": float(n) * n / (ms * 1e-3),
            "bound_ms": bound_ms, "kernel_over_bound": ms / bound_ms})
        torch.cuda.synchronize()
        start = time.perf_counter()
        wrapped = silhouette.silhouette_score(x, labels, device=device)
        result["wrapper_s"] = time.perf_counter() - start
        assert wrapped == score, (wrapped, score)
        if not arguments.skip_host:
            import sklearn.metrics
            sample = HOST_SAMPLE if n > HOST_SAMPLE else None
            start = time.perf_counter()
            host = sklearn.metrics.silhouette_score(
                X=x, labels=labels, sample_size=sample, random_state=0)
            result["host_s"] = time.perf_counter() - start
            result["host_score"] = float(host)
            result["host_cells"] = sample or n
            result["host_over_kernel"] = result["host_s"] / (ms * 1e-3)
        line = json.dumps(result)
        print(line, flush=True)
        lines.append(line)
        if arguments.out:
            with open(arguments.out, "w") as sink:
                sink.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
