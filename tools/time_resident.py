#!/usr/bin/env python3
"""Time the training step of the headline workload (68 579 x 32 738 synthetic counts, NB VAE
100-100-25, 4096 cells, clip + Adam carried by the step) with its minibatch taken three ways, in
ONE process and in interleaved blocks of steps:

  fetched   the CSR rows of the next minibatch densified to uint16 by the step before (the default
            of model.train: scvae_side_work);
  gathered  the rows copied out of the resident uint16 matrix (scvae_gather_rows_u16) in front of
            the step;
  direct    the resident matrix + the row index handed to the step (scvae_step_args.counts_rows).

Prints one JSON line: ms per step of each (median and min / max over the blocks), the stage
probes of the input layer's two products (event pairs inside the step, microseconds) and the head
kernel's time (ms) for fetched and direct, and whether the three leave identical parameters after
the same six steps from the same state (taken with the bit-repeatable decoder gradient).
Usage: python tools/time_resident.py [--cells 68579] [--batch 4096] [--blocks 5] [--steps 40]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=68579)
    ap.add_argument("--features", type=int, default=32738)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    from scvae_amd.engine import Engine
    from scvae_amd.minibatch import synthetic_count_matrix
    dev = torch.device("cuda:0")
    B, L = args.batch, 25
    matrix, _ = synthetic_count_matrix(args.cells, args.features, density=0.05, seed=60,
                                       device=dev)
    dense = matrix.resident_counts_u16()
    eng = Engine(args.features, L, (100, 100), "negative binomial", batch_norm=True, device=dev,
                 seed=0)
    eng.reserve(B, 1)
    assert eng.accepts_counts_u16(B, True, n_iw=1) and eng.accepts_counts_rows(B, True, n_iw=1)
    g = torch.Generator(device=dev).manual_seed(1)
    perm = torch.randperm(args.cells, device=dev, generator=g)
    n_batches = args.cells // B
    x = [torch.empty(B, matrix.u16_pitch, dtype=torch.uint16, device=dev) for _ in range(2)]
    rc = [torch.empty(B, device=dev) for _ in range(2)]
    eps = [torch.empty(1, B, L, device=dev) for _ in range(2)]
    counter = [0]

    def rows_of(i):
        return perm[(i % n_batches) * B:(i % n_batches + 1) * B]

    def noise(i, slot):
        return dict(out=eps[slot], block_stride=B, row_offset=0, seed=3, stream_id=i)

    def run(mode, steps):
        """``steps`` training steps; the first minibatch and noise are issued in line."""
        from scvae_amd.minibatch import philox_normal_blocks
        i0 = counter[0]
        philox_normal_blocks(**noise(i0, 0))
        if mode == "fetched":
            matrix._gather_from_resident = False      # (this one fetch: the CSR rows)
            matrix.request(rows_of(i0), x[0], rc[0]).issue()
            matrix._gather_from_resident = True
        for k in range(steps):
            i, slot = i0 + k, k & 1
            rows = rows_of(i)
            nxt = noise(i + 1, slot ^ 1)
            if mode == "fetched":
                eng.step(x[slot], x[slot], eps=eps[slot], row_const=rc[slot], training=True,
                         x_counts=True, learning_rate=1e-4, next_noise=nxt,
                         next_minibatch=matrix.request(rows_of(i + 1), x[slot ^ 1],
                                                       rc[slot ^ 1]))
            elif mode == "gathered":
                matrix.gather_counts_u16(rows, out=x[slot], row_const_out=rc[slot])
                eng.step(x[slot], x[slot], eps=eps[slot], row_const=rc[slot], training=True,
                         x_counts=True, learning_rate=1e-4, next_noise=nxt)
            else:
                matrix.gather_row_constants(rows, rc[slot])
                eng.step(dense, dense, eps=eps[slot], row_const=rc[slot], training=True,
                         x_counts=True, learning_rate=1e-4, next_noise=nxt, counts_rows=rows)
        counter[0] = i0 + steps

    modes = ("fetched", "gathered", "direct")
    # the same steps from the same state three ways: identical parameters?
    # (under the fixed-order decoder gradient: with the default atomics no two runs agree)
    eng.set_dd_atomics(False)
    state = eng.state_dict()
    finals = []
    for mode in modes:
        eng.load_state_dict(state)
        counter[0] = 0
        run(mode, 6)
        torch.cuda.synchronize()
        finals.append(eng.params.clone())
    identical = all(torch.equal(finals[0], f) for f in finals[1:])
    eng.set_dd_atomics(True)
    eng.load_state_dict(state)
    for mode in modes:      # warm-up of every shape
        run(mode, 10)
    torch.cuda.synchronize()
    times = {mode: [] for mode in modes}
    for _ in range(args.blocks):
        for mode in modes:
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            run(mode, args.steps)
            e1.record()
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1) / args.steps)
    # per kernel, inside the step: the input layer's products and the head kernel
    kernels = {}
    for mode in ("fetched", "direct"):
        eng.probe_stages(10)
        eng.probe_heads(10)
        run(mode, 10)
        torch.cuda.synchronize()
        stages = eng.probe_stages_us()
        heads = eng.probe_heads_ms()
        eng.probe_stages(0)
        eng.probe_heads(0)
        kernels[mode] = {
            "count_gemm_fwd_us": round(statistics.median(stages["count_gemm_fwd"]), 1),
            "count_gemm_dw_us": round(statistics.median(stages["count_gemm_dw"]), 1),
            "fetch_us": (round(statistics.median(stages["fetch"]), 1)
                         if stages["fetch"] else None),
            "head_kernel_ms": round(statistics.median(heads), 4) if heads else None}
    line = {"workload": "{} x {} NB VAE 100-100-25, {} cells per step".format(
                args.cells, args.features, B),
            "blocks": args.blocks, "steps_per_block": args.steps,
            "resident_bytes": dense.numel() * 2,
            "identical_parameters_after_6_steps": identical, "in_step": kernels}
    for mode in modes:
        line[mode + "_ms"] = {"median": round(statistics.median(times[mode]), 4),
                              "min": round(min(times[mode]), 4),
                              "max": round(max(times[mode]), 4)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
