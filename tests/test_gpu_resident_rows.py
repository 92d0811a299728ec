"""The resident training set on the device: a step that takes "resident uint16
matrix + row index" as its minibatch (``scvae_step_args.counts_rows``), the
row-gather entry for the plans without indexed kernels, and
``model.train(resident_training_set=True)``.

The yardstick is BIT-IDENTITY with the path that exists -- the same step given
the same rows as an ordinary uint16 minibatch, fetched from the CSR matrix --
under ``set_dd_atomics(False)`` (the bit-repeatable mode), plus one comparison
with the fp64 oracle so that the indexed path is not only held to its sibling.

Count kernels: by the plan's own rule they run (and a uint16 minibatch is
accepted) from cells x genes of 768 x 32 768 upwards, i.e. of the grid below
only at 4096 x 32 738; every other size takes
``Engine.set_count_gemm(True, always=True)`` -- as the evaluation-pass tests
do at small gene counts -- and then accepts the index as well, 100 and 128
cells (the all-in-one-phase head kernel, the mid chain) included.

``python tests/test_gpu_resident_rows.py guard`` runs a cut of the grid in
this process: the body of the ``SCVAE_WS_GUARD=1`` test (the switch is read
once per process).
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from oracle import models as om  # noqa: E402

from _parity import (LL_ATOL, LL_RTOL, close_elementwise,  # noqa: E402
                     close_maxnorm, close_per_tensor, close_scalar)

pytestmark = pytest.mark.gpu

H, L = (100, 100), 25
LIKELIHOODS = ["poisson", "negative binomial", "zero-inflated poisson",
               "zero-inflated negative binomial"]
SHAPES = ([(cells, F) for cells in (100, 128, 130, 700, 1536, 4096)
           for F in (1000, 2050)] + [(4096, 32738)])
INDEX_KINDS = ("permutation slice", "repeats", "descending")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    """uint16 as int16: the same bits in a dtype every torch op takes."""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _stream(device):
    from scvae_amd.engine import current_stream_handle
    return current_stream_handle(torch.device(device))


# ---------------------------------------------------------------- 3: the gather
def _random_u16(rows, ld, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-32768, 32768, (rows, ld), dtype=torch.int16,
                         device=device, generator=g).view(torch.uint16)


def _gather(src, rows, cols, out):
    from scvae_amd import _lib
    lib = _lib.load()
    _lib.check(lib.scvae_gather_rows_u16(
        _ptr(src), src.stride(0), _ptr(rows), rows.numel(), cols, _ptr(out),
        out.stride(0), _stream(src.device)), "scvae_gather_rows_u16")
    return out


@pytest.mark.parametrize("n_src,ld_src,cols,ld_out,n,kind", [
    (500, 1024, 1024, 1024, 300, "repeats"),
    (500, 1024, 1024, 1024, 257, "unsorted"),
    (300, 2112, 2050, 2176, 37, "unsorted"),        # cols % 64 != 0, ld_out > cols
    (300, 1024, 1000, 1088, 1, "unsorted"),         # one row
    (64, 32768, 32738, 32768, 131, "repeats"),      # the headline row: 64 KB
    (200, 1001, 999, 1003, 77, "unsorted"),         # pitches off 16 bytes
    (50, 16, 5, 8, 13, "repeats"),                  # less than one 16-byte piece
])
def test_gather_rows_u16_equals_index_select(cuda_device, n_src, ld_src, cols,
                                             ld_out, n, kind):
    src = _random_u16(n_src, ld_src, cuda_device, seed=n_src + cols)
    g = torch.Generator().manual_seed(n)
    if kind == "repeats":
        rows = torch.randint(0, max(n_src // 4, 1), (n,), generator=g)
    else:
        rows = torch.randperm(n_src, generator=g)[:n]
        if n > 1:
            assert not bool((rows[1:] > rows[:-1]).all())
    rows = rows.to(device=cuda_device, dtype=torch.int64)
    out = torch.full((n, ld_out), 0x5A5A, dtype=torch.int16,
                     device=cuda_device).view(torch.uint16)
    _gather(src, rows, cols, out)
    want = torch.index_select(_bits(src), 0, rows)[:, :cols]
    assert torch.equal(_bits(out)[:, :cols], want)
    # the columns beyond cols are the caller's
    assert bool((_bits(out)[:, cols:] == 0x5A5A).all())


def test_gather_rows_u16_as_fp32_equals_index_select(cuda_device):
    """The same rows converted to fp32 (``scvae_gather_rows_u16_f32``: the
    minibatch of a step that takes no uint16 batch)."""
    from scvae_amd import _lib
    lib = _lib.load()
    n_src, ld, cols, n = 300, 1088, 1000, 141
    src = _random_u16(n_src, ld, cuda_device, seed=9)
    rows = torch.randint(0, n_src, (n,)).to(device=cuda_device,
                                            dtype=torch.int64)
    out = torch.full((n, cols + 3), -1.0, device=cuda_device)
    _lib.check(lib.scvae_gather_rows_u16_f32(
        _ptr(src), ld, _ptr(rows), n, cols, _ptr(out), out.stride(0),
        _stream(cuda_device)), "scvae_gather_rows_u16_f32")
    want = torch.index_select(_bits(src), 0, rows)[:, :cols].to(torch.int32)
    want = torch.where(want < 0, want + 65536, want).to(torch.float32)
    assert torch.equal(out[:, :cols], want)
    assert bool((out[:, cols:] == -1.0).all())


def test_gather_rows_u16_from_the_far_end_of_a_large_matrix(cuda_device):
    """A source of more than 2^31 elements (70 000 x 32 768: the headline
    set's size), rows from its far end: 64-bit row offsets."""
    n_src, ld, far = 70000, 32768, 2048
    assert n_src * ld > 2 ** 31 and (n_src - far) * ld > 2 ** 31
    src = torch.empty(n_src, ld, dtype=torch.int16,
                      device=cuda_device).view(torch.uint16)
    _bits(src)[n_src - far:] = _bits(_random_u16(far, ld, cuda_device, 5))
    g = torch.Generator().manual_seed(3)
    rows = (n_src - far + torch.randint(0, far, (515,), generator=g)).to(
        device=cuda_device, dtype=torch.int64)
    out = torch.empty(515, ld, dtype=torch.int16,
                      device=cuda_device).view(torch.uint16)
    _gather(src, rows, ld, out)
    assert torch.equal(_bits(out), torch.index_select(_bits(src), 0, rows))


# ------------------------------------------------------- 4: the indexed step
@functools.lru_cache(maxsize=2)
def _resident(device, rows, F):
    """(DeviceCSR, its resident uint16 matrix [rows, pitch])."""
    from scvae_amd.minibatch import synthetic_count_matrix
    matrix, _ = synthetic_count_matrix(rows, F, density=0.05, seed=60 + F % 7,
                                       device=device)
    assert matrix.integer_counts
    dense = matrix.resident_counts_u16(chunk=1000)
    assert dense.shape == (rows, matrix.u16_pitch)
    assert matrix.resident_u16 is dense
    return matrix, dense


def _fetched(matrix, idx, rc):
    """The rows ``idx`` through the CSR fetch: the path that exists."""
    matrix._gather_from_resident = False
    try:
        return matrix.gather_counts_u16(idx, row_const_out=rc)
    finally:
        matrix._gather_from_resident = True


def _engine(F, likelihood, device, always, model_type="VAE", K=1):
    from scvae_amd.engine import Engine
    eng = Engine(F, L, H, likelihood, batch_norm=True, device=device, seed=0,
                 model_type=model_type, n_clusters=K)
    g = torch.Generator().manual_seed(1)
    for name, p in eng.named_parameters().items():
        if not name.endswith("weights"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    for name, m in eng.named_moving_statistics().items():
        if name.endswith("moving_mean"):
            m.copy_(torch.randn(m.shape, generator=g) * 0.2)
        else:
            m.copy_(torch.rand(m.shape, generator=g) + 0.5)
    eng.set_dd_atomics(False)        # the bit-repeatable mode
    if always:
        eng.set_count_gemm(True, always=True)
    return eng


def _indices(kind, n_src, cells, device):
    g = torch.Generator().manual_seed(cells + len(kind))
    if kind == "permutation slice":
        idx = torch.randperm(n_src, generator=g)[cells:2 * cells]
    elif kind == "repeats":
        idx = torch.randint(0, n_src, (cells,), generator=g)
        idx[1::3] = idx[0::3][:idx[1::3].numel()]
        assert idx.unique().numel() < cells
    else:
        idx = torch.arange(n_src - 1, n_src - 1 - cells, -1)
    return idx.to(device=device, dtype=torch.int64).contiguous()


def _noise(cells, device, seed):
    from scvae_amd.minibatch import philox_normal
    eps = torch.empty(1, cells, L, device=device)
    philox_normal(eps[0], row_offset=0, seed=seed, stream_id=0)
    return eps


def _step(eng, x, rc, eps, training, counts_rows=None):
    cells = rc.numel()
    ll = torch.zeros(cells, device=rc.device)
    qz = torch.zeros(cells, L, device=rc.device)
    scalars = eng.step(x, x, eps=eps, row_const=rc, training=training,
                       x_counts=True, counts_rows=counts_rows,
                       outputs={"log_p_x_given_z": ll, "q_z_mean": qz}).clone()
    return [scalars, ll, qz, eng.grads.clone(), eng.moving.clone()]


def _check_indexed_step(device, likelihood, cells, F):
    """Training and evaluation steps of one plan from the same parameters:
    (resident matrix, index) against the same rows fetched -- every output
    bit for bit, for three kinds of index."""
    always = (cells, F) != (4096, 32738)
    matrix, dense = _resident(device, 3 * cells + 11, F)
    direct = _engine(F, likelihood, device, always)
    fetched = _engine(F, likelihood, device, always)
    for training in (True, False):
        assert direct.accepts_counts_u16(cells, training, n_iw=1)
        assert direct.accepts_counts_rows(cells, training, n_iw=1), (
            likelihood, cells, F, training)
    for number, kind in enumerate(INDEX_KINDS):
        idx = _indices(kind, dense.shape[0], cells, device)
        rc = matrix.gather_row_constants(
            idx, torch.empty(cells, device=device))
        rc_fetched = torch.empty(cells, device=device)
        rows = _fetched(matrix, idx, rc_fetched)
        assert torch.equal(rc, rc_fetched)
        assert torch.equal(_bits(rows),
                           torch.index_select(_bits(dense), 0, idx))
        eps = _noise(cells, device, seed=7 + number)
        for training in (True, False):
            got = _step(direct, dense, rc, eps, training, counts_rows=idx)
            want = _step(fetched, rows, rc, eps, training)
            torch.cuda.synchronize()
            for name, a, b in zip(("scalars", "log_p_x_given_z", "q_z_mean",
                                   "gradients", "moving statistics"),
                                  got, want):
                assert torch.equal(a, b), (likelihood, cells, F, kind,
                                           training, name)
            assert bool(torch.isfinite(got[0][:4]).all())


@pytest.mark.parametrize("cells,F", SHAPES)
@pytest.mark.parametrize("likelihood", LIKELIHOODS)
def test_indexed_step_is_the_step_on_the_gathered_rows(cuda_device, likelihood,
                                                       cells, F):
    _check_indexed_step(cuda_device, likelihood, cells, F)


def test_indexed_step_with_atomics_at_the_parity_tolerances(cuda_device):
    """The plan's default -- the decoder gradient through fp32 atomics, not
    bit-repeatable from run to run -- at the tolerances of ``_parity``."""
    cells, F = 1536, 2050
    matrix, dense = _resident(cuda_device, 3 * cells + 11, F)
    results = []
    idx = _indices("permutation slice", dense.shape[0], cells, cuda_device)
    rc = matrix.gather_row_constants(idx, torch.empty(cells,
                                                      device=cuda_device))
    eps = _noise(cells, cuda_device, seed=2)
    for is_direct in (True, False):
        eng = _engine(F, "negative binomial", cuda_device, True)
        eng.set_dd_atomics(True)
        x = dense if is_direct else _fetched(
            matrix, idx, torch.empty(cells, device=cuda_device))
        results.append((eng, _step(eng, x, rc, eps, True,
                                   counts_rows=idx if is_direct else None)))
    (eng, got), (_, want) = results
    torch.cuda.synchronize()
    for i in range(4):
        close_scalar(got[0][i], want[0][i], what="scalar %d" % i)
    close_elementwise(got[1], want[1], rtol=LL_RTOL, atol=LL_ATOL, what="ll")
    close_maxnorm(got[2], want[2], rtol=1e-4, what="q_z_mean")
    close_per_tensor(got[3], want[3], eng.param_table, rtol=2e-4,
                     what="gradient")
    close_per_tensor(got[4], want[4], eng.moving_table, rtol=1e-5,
                     what="moving")


# ------------------------------------------------------------ 5: the oracle
def test_indexed_training_step_against_the_oracle(cuda_device):
    cells, F = 1536, 1000
    matrix, dense = _resident(cuda_device, 3 * cells + 11, F)
    eng = _engine(F, "negative binomial", cuda_device, True)
    assert eng.accepts_counts_rows(cells, True, n_iw=1)
    idx = _indices("repeats", dense.shape[0], cells, cuda_device)
    rc = matrix.gather_row_constants(idx, torch.empty(cells,
                                                      device=cuda_device))
    eps = _noise(cells, cuda_device, seed=4)
    cfg = om.ModelConfig(feature_size=F, latent_size=L, hidden_sizes=H,
                         likelihood="negative binomial")
    params = {k: v.detach().cpu().double()
              for k, v in eng.named_parameters().items()}
    moving = {k: v.detach().cpu().double()
              for k, v in eng.named_moving_statistics().items()}
    ll = torch.zeros(cells, device=cuda_device)
    sc = eng.step(dense, dense, eps=eps, row_const=rc, training=True,
                  x_counts=True, counts_rows=idx,
                  outputs={"log_p_x_given_z": ll}).cpu().numpy()
    dev_grads = {k: v.detach().cpu().double()
                 for k, v in eng.named_gradients().items()}
    torch.cuda.synchronize()
    xh = torch.index_select(_bits(dense), 0, idx)[:, :F].cpu().double()
    assert float(xh.min()) >= 0       # (counts far below 2^15)
    out, grads = om.gradients(
        lambda p: om.vae_forward(cfg, p, moving, xh, xh, eps.cpu().double(),
                                 True, 1.0, {}), params)
    close_scalar(sc[0], out["lower_bound"], what="lower_bound")
    close_scalar(sc[2], out["reconstruction_error"],
                 what="reconstruction_error")
    close_scalar(sc[3], out["kl_divergence"], what="kl_divergence")
    close_elementwise(ll, out["log_p_x_given_z"].reshape(-1), rtol=LL_RTOL,
                      atol=LL_ATOL, what="per-cell log-likelihood")
    for name, g in dev_grads.items():
        if name.endswith("DENSE/biases") and ("ENCODER/" in name
                                              or "DECODER/" in name):
            assert g.abs().max().item() == 0.0, name
            continue
        close_maxnorm(g, grads[name], rtol=2e-4, what="grad " + name)


# ------------------------------------------- 6: plans that gather the rows
@pytest.mark.parametrize("case", ["GMVAE", "fp32 heads"])
def test_plans_without_indexed_kernels_refuse_the_index_and_gather(
        cuda_device, case):
    from scvae_amd import _lib
    cells, F, K = 700, 2050, 3
    matrix, dense = _resident(cuda_device, 3 * cells + 11, F)
    gm = case == "GMVAE"

    def engine():
        eng = _engine(F, "negative binomial", cuda_device, True,
                      model_type="GMVAE" if gm else "VAE", K=K if gm else 1)
        if not gm:
            eng.set_head_arith("fp32")
        return eng
    idx = _indices("permutation slice", dense.shape[0], cells, cuda_device)
    rc = matrix.gather_row_constants(idx, torch.empty(cells,
                                                      device=cuda_device))
    g = torch.Generator().manual_seed(8)
    shape = (K, 1, cells, L) if gm else (1, cells, L)
    eps = torch.randn(shape, generator=g).to(cuda_device)
    eng = engine()
    assert eng.accepts_counts_u16(cells, True, n_iw=1)
    assert not eng.accepts_counts_rows(cells, True, n_iw=1)
    assert not eng.accepts_counts_rows(cells, False)
    # refused with an error and no launch: nothing the step writes has changed
    eng.grads.fill_(7.0)
    eng.scalars.fill_(-3.0)
    moving = eng.moving.clone()
    with pytest.raises(_lib.HipLibraryError, match="row index"):
        eng.step(dense, dense, eps=eps, row_const=rc, training=True,
                 x_counts=True, counts_rows=idx)
    torch.cuda.synchronize()
    assert bool((eng.grads == 7.0).all())
    assert bool((eng.scalars == -3.0).all())
    assert torch.equal(eng.moving, moving)
    # ... and trains bit-identically from the gathered rows
    gathered = matrix.gather_counts_u16(idx)       # (scvae_gather_rows_u16)
    fetched = _fetched(matrix, idx, torch.empty(cells, device=cuda_device))
    assert gathered.data_ptr() != fetched.data_ptr()
    assert torch.equal(_bits(gathered), _bits(fetched))
    results = []
    for x in (gathered, fetched):
        eng = engine()
        out = []
        for _ in range(2):
            s = eng.step(x, x, eps=eps, row_const=rc, training=True,
                         x_counts=True).clone()
            out += [s, eng.grads.clone()]
            eng.adam_step(1e-3)
        torch.cuda.synchronize()
        results.append(out + [eng.params.clone(), eng.moving.clone()])
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), i


# ------------------------------------------------- 7: under the workspace guard
GUARD_CASES = ([(likelihood, 130, 1000) for likelihood in LIKELIHOODS]
               + [(likelihood, 1536, 2050) for likelihood in LIKELIHOODS]
               + [("negative binomial", 100, 1000),
                  ("zero-inflated negative binomial", 128, 2050),
                  ("negative binomial", 700, 2050),
                  ("negative binomial", 4096, 1000)])


def test_indexed_steps_under_the_workspace_guard(cuda_device):
    """A cut of the grid again with a guard region behind every workspace
    buffer, checked after every step (a subprocess: the switch is read once
    per process)."""
    environment = dict(os.environ, SCVAE_WS_GUARD="1", PYTHONPATH=ROOT)
    done = subprocess.run(
        [sys.executable, os.path.abspath(__file__), "guard"], env=environment,
        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "guarded cases ok: {}".format(len(GUARD_CASES)) in done.stdout


# --------------------------------------------------------- 8: model.train
def _values(n, F, seed=3):
    rng = np.random.default_rng(seed)
    centres = rng.gamma(1.0, 2.0, size=(3, F))
    x = rng.poisson(centres[rng.integers(0, 3, size=n)]).astype(np.float64)
    x *= rng.random((n, F)) > 0.5
    return x.astype(np.float32)


def _data_set(values):
    from scvae_amd.data import DataSet
    n, F = values.shape
    return DataSet("resident", values=values, kind="training",
                   example_names=np.arange(n).astype(str),
                   feature_names=np.arange(F).astype(str))


def _trained(directory, device, data, F, B, resident, budget=None):
    """(per-epoch results of the epoch-end pass, final parameters, model)."""
    from scvae_amd.models import VariationalAutoencoder
    model = VariationalAutoencoder(
        feature_size=F, latent_size=8, hidden_sizes=[64, 48],
        reconstruction_distribution="negative binomial",
        log_directory=str(directory), device=device)
    model.engine.set_count_gemm(True, always=True)
    if budget is not None:
        model.training_resident_bytes = budget
    curves = []
    evaluation_pass = model._evaluation_pass

    def kept(*args, **kwargs):
        result = evaluation_pass(*args, **kwargs)
        curves.append(result)
        return result
    model._evaluation_pass = kept
    state = np.random.get_state()
    np.random.seed(20261016)
    try:
        keywords = dict(resident_training_set=True) if resident else {}
        assert model.train(data, None, number_of_epochs=2, minibatch_size=B,
                           learning_rate=1e-3, deterministic=True,
                           **keywords) == 0
    finally:
        np.random.set_state(state)
    torch.cuda.synchronize()
    return curves, model.engine.params.clone(), model


def _assert_same_run(a, b):
    (curves_a, params_a, _), (curves_b, params_b, _) = a, b
    assert len(curves_a) == len(curves_b) == 2
    for one, other in zip(curves_a, curves_b):
        assert one.keys() == other.keys()
        for key in one:
            assert np.array_equal(np.asarray(one[key]),
                                  np.asarray(other[key])), key
    assert torch.equal(params_a, params_b)


@pytest.mark.parametrize("B", [100, 1536])
def test_model_train_from_the_resident_set_is_the_same_run(
        tmp_path, cuda_device, capsys, B):
    n, F, epochs = 3437, 300, 2
    assert n % B
    data = _data_set(_values(n, F))
    steps = epochs * -(-n // B)
    plain = _trained(tmp_path / "plain", cuda_device, data, F, B, False)
    model = plain[2]
    assert model._training_resident_hits == 0
    assert model._training_resident_gathers == 0
    resident = _trained(tmp_path / "resident", cuda_device, data, F, B, True)
    _assert_same_run(resident, plain)
    model = resident[2]
    assert (model._training_resident_hits
            + model._training_resident_gathers) == steps
    if B == 1536:
        assert model._training_resident_hits > 0
    # one allocation: the epoch-end pass over the training set read the matrix
    # the steps indexed
    assert model._training_resident_address is not None
    assert (model._evaluation_resident_address
            == model._training_resident_address)
    assert model._evaluation_resident_hits > 0
    # a budget the set does not fit: trains as without the switch, and says so
    capsys.readouterr()
    refused = _trained(tmp_path / "refused", cuda_device, data, F, B, True,
                       budget=1)
    assert "Resident training set not used" in capsys.readouterr().out
    _assert_same_run(refused, plain)
    model = refused[2]
    assert model._training_resident_hits == 0
    assert model._training_resident_gathers == 0
    assert model._training_resident_address is None


# ------------------------------------------------------- 9: data parallel
def _two_rank_worker(rank, port, directory, result_path):
    """Both ranks share cuda:0 (gloo), as tests/test_gpu_dataparallel.py
    starts them: ``model.train(resident_training_set=True)`` under two ranks
    against one process without the switch."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        from scvae_amd.data import DataSet
        from scvae_amd.models import VariationalAutoencoder
        rng = np.random.default_rng(5)
        n, F = 96, 40
        values = (rng.poisson(2.0, (n, F)) * (rng.random((n, F)) > 0.5)
                  ).astype(np.float32)
        data = DataSet("dp", values=values,
                       example_names=np.array(["c%d" % i for i in range(n)]),
                       feature_names=np.array(["g%d" % i for i in range(F)]))

        def model(name):
            return VariationalAutoencoder(
                feature_size=F, latent_size=3, hidden_sizes=[10],
                reconstruction_distribution="negative binomial",
                log_directory=os.path.join(directory, name), device="cuda:0")
        sharded = model("dp")
        np.random.seed(11)
        sharded.train(data, None, number_of_epochs=2, minibatch_size=32,
                      learning_rate=1e-3, resident_training_set=True)
        counted = (sharded._training_resident_hits
                   + sharded._training_resident_gathers)
        params = sharded.engine.params.clone()
        if rank == 0:
            single = model("single")
            import scvae_amd.models.base as base
            original = base._distributed
            base._distributed = lambda: (1, 0)
            try:
                np.random.seed(11)
                single.train(data, None, number_of_epochs=2,
                             minibatch_size=32, learning_rate=1e-3)
            finally:
                base._distributed = original
            reference = single.engine.params
            worst = ((params - reference).abs().max()
                     / reference.abs().max()).item()
            with open(result_path, "w") as handle:
                handle.write(repr((worst, counted)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_from_the_resident_set_equal_single_process(cuda_device,
                                                              tmp_path):
    import torch.multiprocessing as mp
    result = tmp_path / "worst.txt"
    port = 29650 + (os.getpid() % 100)
    mp.spawn(_two_rank_worker, args=(port, str(tmp_path), str(result)),
             nprocs=2, join=True)
    worst, counted = eval(result.read_text().replace("nan", "float('nan')"))
    assert worst <= 5e-4, worst       # (test_gpu_dataparallel.py's bound)
    assert counted == 2 * 3           # every step of the rank took the set


if __name__ == "__main__":
    if sys.argv[1:] != ["guard"]:
        raise SystemExit("usage: test_gpu_resident_rows.py guard")
    assert os.environ.get("SCVAE_WS_GUARD") == "1"
    for case in GUARD_CASES:
        _check_indexed_step("cuda:0", *case)
        print("ok", case, flush=True)
    print("guarded cases ok: {}".format(len(GUARD_CASES)))
