"""Time the exact t-SNE on the device, on synthetic latent values:
    python tools/time_tsne.py [--skip-host] [--shapes NxL ...] [--out FILE]
One JSON line per shape: the perplexity search (device events around
scvae_tsne_perplexity), one pass over all pairs (scvae_tsne_gradient without
and with the KL divergence, mean of --launches launches) beside the estimate
it is judged by -- N^2 pairs x 85 fp32 lane-operations (25 latent values in
the direct form, two exponentials, the two-dimensional kernel) at the chip's
fp32 vector rate, 157.3 TFLOPS = 78.65e12 lane-instructions a second -- and a
whole fit with the default schedule where the pass time says it ends within
--fit-within seconds.  The host column, for context: scikit-learn's
Barnes-Hut TSNE(n_components=2, random_state=42) as the reference calls it,
on the first --host-cells cells of the first shape."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch

from scvae_amd.analyses import tsne

FP32_VECTOR_LANE_INSTRUCTIONS_PER_SECOND = 157.3e12 / 2
LANE_OPERATIONS_PER_PAIR = 85
DEFAULT_SHAPES = ["68579x25", "200000x25"]


def latents(n, latent_size, k=20, seed=0):
    rng = numpy.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((k, latent_size))
    x = centres[rng.integers(k, size=n)].astype(numpy.float32)
    x += rng.standard_normal((n, latent_size), dtype=numpy.float32)
    return x


def timed(call, launches):
    start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(launches):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES)
    parser.add_argument("--launches", type=int, default=3)
    parser.add_argument("--fit-within", type=float, default=120.0)
    parser.add_argument("--host-cells", type=int, default=5000)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--out")
    arguments = parser.parse_args()
    device = torch.device("cuda:0")
    # the first launch of a process pays for loading the code object
    tsne.DeviceTSNE(max_iter=2, exploration_iterations=1,
                    device=device).fit_transform(latents(512, 25))
    lines = []
    for shape in arguments.shapes:
        n, latent_size = (int(v) for v in shape.split("x"))
        x = tsne.centre(latents(n, latent_size))
        passes = tsne.TSNEPasses(x, device=device)
        result = {"cells": n, "latent_size": latent_size,
                  "workspace_bytes": passes.workspace.numel()}
        torch.cuda.synchronize()
        start = time.perf_counter()
        passes.search(30.0)
        result["search_s"] = time.perf_counter() - start
        steps = passes.steps.cpu().numpy()
        result["search_steps_mean"] = float(steps.mean())
        result["search_steps_max"] = int(steps.max())
        y = torch.from_numpy(tsne.initial_embedding(x).astype(
            numpy.float32)).to(device)
        grad = torch.empty_like(y)
        kl = torch.zeros(1, dtype=torch.float64, device=device)
        norm = torch.zeros(1, dtype=torch.float64, device=device)
        launches = arguments.launches
        pass_ms = timed(lambda: passes.gradient(y, 12.0, grad), launches)
        check_ms = timed(
            lambda: passes.gradient(y, 12.0, grad, kl, norm), launches)
        bound_ms = (float(n) * n * LANE_OPERATIONS_PER_PAIR
                    / FP32_VECTOR_LANE_INSTRUCTIONS_PER_SECOND * 1e3)
        result.update({
            "pass_ms": pass_ms, "pass_with_kl_ms": check_ms,
            "launches": launches, "estimate_ms": bound_ms,
            "pass_over_estimate": pass_ms / bound_ms,
            "pairs_per_second": float(n) * n / (pass_ms * 1e-3)})
        expected = (1000 * pass_ms + 20 * (check_ms - pass_ms)) * 1e-3
        result["fit_expected_s"] = expected + result["search_s"]
        del passes
        if result["fit_expected_s"] <= arguments.fit_within:
            model = tsne.DeviceTSNE(device=device)
            torch.cuda.synchronize()
            start = time.perf_counter()
            model.fit_transform(x)
            result["fit_s"] = time.perf_counter() - start
            result["fit_iterations"] = model.n_iter_ + 1
            result["fit_kl_divergence"] = model.kl_divergence_
        else:
            result["fit_skipped"] = "expected above {} s".format(
                arguments.fit_within)
        if not arguments.skip_host and not lines:   # once: the first shape
            from sklearn.manifold import TSNE
            cells = min(n, arguments.host_cells)
            start = time.perf_counter()
            host = TSNE(n_components=2, random_state=42)
            host.fit_transform(x[:cells])
            result["host_barnes_hut_s"] = time.perf_counter() - start
            result["host_cells"] = cells
            result["host_kl_divergence"] = float(host.kl_divergence_)
        line = json.dumps(result)
        print(line, flush=True)
        lines.append(line)
        if arguments.out:
            with open(arguments.out, "w") as sink:
                sink.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
