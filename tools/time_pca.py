"""Time the device PCA beside what the reference fits on the host, on a
synthetic reconstruction (smooth rates of four groups of cells) and the
Poisson counts drawn from it:
    python tools/time_pca.py [--skip-host] [--shapes NxF ...] [--out FILE]
One JSON line per shape:

moments_ms    the two passes of ``scvae_pca_moments`` between device events
iteration_ms  one iteration's kernels, ``scvae_pca_project`` and
              ``scvae_pca_back_project`` with a block of 16, between device
              events (mean of --launches iterations), and each on its own;
              iteration_floor_ms = the matrix read twice, 2 x 4 N F bytes,
              over the HBM rate a float4 copy reaches, 6.29 TB/s
fit_s         what ``evaluate`` runs for a set: ``evaluation_decomposition``
              (moments, the iterations with their host algebra, the final
              projection, the copies), wall clock, with the iterations it took
              -- on the reconstruction and on the counts
host_s        scikit-learn's ``IncrementalPCA(n_components=2, batch_size=100)``
              -- what ``decomposition.py:66-73`` fits -- on the first
              ``host_rows`` rows of the reconstruction copied to the host
              (--host-rows; 0 = all of them), with 16 threads
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

from scvae_amd.analyses import decomposition

HBM_BYTES_PER_SECOND = 6.29e12
DEFAULT_SHAPES = ["4096x2101", "68579x32738"]


def synthetic(n, features, device, seed=0):
    """(rates [N, F] fp32 on the device: depth_i base_j programme_{g_i j},
    Poisson counts of them)."""
    generator = torch.Generator(device=device).manual_seed(seed)
    rng = numpy.random.default_rng(seed)
    base = torch.from_numpy(rng.gamma(0.3, 2.0, features)).float().to(device)
    programme = torch.from_numpy(numpy.exp(
        rng.normal(0, 1, (4, features))
        * (rng.random((4, features)) < 0.15))).float().to(device)
    group = torch.from_numpy(rng.integers(0, 4, n)).to(device)
    depth = torch.from_numpy(rng.gamma(8, 1 / 8, n)).float().to(device)
    rates = torch.empty(n, features, device=device)
    counts = torch.empty(n, features, device=device)
    for first in range(0, n, 4096):
        rows = slice(first, min(first + 4096, n))
        rates[rows] = depth[rows, None] * base * programme[group[rows]]
        counts[rows] = torch.poisson(rates[rows], generator=generator)
    return rates, counts


def device_ms(run, launches):
    run()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        run()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES)
    parser.add_argument("--launches", type=int, default=5)
    parser.add_argument("--skip-host", action="store_true")
    parser.add_argument("--host-rows", type=int, default=4000)
    parser.add_argument("--out")
    arguments = parser.parse_args()
    device = torch.device("cuda:0")
    lines = []
    for shape in arguments.shapes:
        n, features = (int(v) for v in shape.lower().split("x"))
        rates, counts = synthetic(n, features, device)
        operator = decomposition.DeviceOperator(rates)
        record = {"shape": [n, features], "block": 16}
        record["moments_ms"] = device_ms(operator.moments, arguments.launches)
        q, _ = numpy.linalg.qr(numpy.random.default_rng(42).standard_normal(
            (features, 16)))
        q_device = operator._block(q, features)
        y = operator.project(q)

        def project():
            decomposition._lib.check(operator.lib.scvae_pca_project(
                decomposition._ptr(rates), rates.stride(0), n, features,
                decomposition._ptr(operator.mean),
                decomposition._ptr(q_device), 16, decomposition._ptr(y),
                operator._stream()))
        z = torch.empty(features, 16, dtype=torch.float64, device=device)
        workspace = operator._workspace(n, 16)

        def back_project():
            decomposition._lib.check(operator.lib.scvae_pca_back_project(
                decomposition._ptr(rates), rates.stride(0), n, features,
                decomposition._ptr(operator.mean), decomposition._ptr(y), 16,
                decomposition._ptr(z), decomposition._ptr(workspace),
                workspace.numel(), operator._stream()))
        record["project_ms"] = device_ms(project, arguments.launches)
        record["back_project_ms"] = device_ms(back_project, arguments.launches)
        record["iteration_ms"] = device_ms(
            lambda: (project(), back_project()), arguments.launches)
        record["iteration_floor_ms"] = (
            2 * 4 * n * features / HBM_BYTES_PER_SECOND * 1e3)
        del operator, workspace
        for name, values in (("reconstruction", rates), ("counts", counts)):
            torch.cuda.synchronize()
            start = time.perf_counter()
            fit = decomposition.evaluation_decomposition(values)
            torch.cuda.synchronize()
            record["fit_s_" + name] = time.perf_counter() - start
            record["iterations_" + name] = fit["iterations"]
            record["converged_" + name] = bool(fit["converged"])
            record["explained_variance_ratio_" + name] = [
                float(r) for r in fit["explained_variance_ratio"]]
        if not arguments.skip_host:
            from sklearn.decomposition import IncrementalPCA
            rows = n if arguments.host_rows <= 0 else min(
                n, arguments.host_rows)
            host = rates[:rows].cpu().numpy()
            start = time.perf_counter()
            IncrementalPCA(n_components=2, batch_size=100).fit_transform(host)
            record["host_s"] = time.perf_counter() - start
            record["host_rows"] = rows
            del host
        del rates, counts
        torch.cuda.empty_cache()
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)
    if arguments.out:
        os.makedirs(os.path.dirname(os.path.abspath(arguments.out)),
                    exist_ok=True)
        with open(arguments.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
