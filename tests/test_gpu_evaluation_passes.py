"""GPU: evaluation passes (``_evaluation_pass``; the epoch-end passes of
``model.train``, ``model.evaluate``) against the fp64 oracle, on every path
a pass takes -- whole minibatches stacked into one step (``evaluation_chunks``),
the hidden stack as one launch (``eval_mlp_kernel``) or the mid-chain kernels,
uint16 minibatches whose fetch and noise ride on the step before ("carried"),
the resident uint16 copy of the set later passes read as views -- and the
sizing of those steps under memory pressure, across ranks and around a step
that raises.

The expected values are the reference's: ``sum_j mean_j / (N / B)`` over its
sequential minibatches of B cells, one oracle call per minibatch at the
engine's fp32 state, every cell with the Philox noise of its row in the set
(stream ``(1 << 40) + counter * (1 << 20)`` of the model's counter of passes).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import models as om

from _parity import ELBO_RTOL, close_elementwise, close_maxnorm, close_scalar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the step tests' bound for q_z_mean (of the tensor's largest magnitude)
Q_Z_MEAN_RTOL = 1e-4
# ... and theirs for the GMVAE's KL(q(y|x) || p(y)): a difference of entropies
KL_Y_RTOL = 2e-4
F_DEFAULT, L_DEFAULT, H_DEFAULT = 300, 8, (64, 48)


@pytest.fixture(autouse=True)
def _seeded_minibatch_order():
    """``model.train`` shuffles with NumPy's global generator."""
    state = np.random.get_state()
    np.random.seed(20261016)
    yield
    np.random.set_state(state)


def _values(n, F, seed=3, integer=True):
    """Counts of three kinds of cell, half of them zeroed; ``integer=False``:
    the same scaled to non-integer values (no uint16 minibatch)."""
    rng = np.random.default_rng(seed)
    centres = rng.gamma(1.0, 2.0, size=(3, F))
    x = rng.poisson(centres[rng.integers(0, 3, size=n)]).astype(np.float64)
    x *= rng.random((n, F)) > 0.5
    if not integer:
        x *= 0.37 + rng.random((n, F))
    return x.astype(np.float32)


def _data_set(values, kind="training"):
    from scvae_amd.data import DataSet
    n, F = values.shape
    return DataSet("passes", values=values, kind=kind,
                   example_names=np.arange(n).astype(str),
                   feature_names=np.arange(F).astype(str))


def _model(tmp_path, device, model_type="VAE", F=F_DEFAULT, L=L_DEFAULT,
           H=H_DEFAULT, K=3):
    from scvae_amd.models import (GaussianMixtureVariationalAutoencoder,
                                  VariationalAutoencoder)
    kw = dict(feature_size=F, latent_size=L, hidden_sizes=list(H),
              reconstruction_distribution="negative binomial",
              log_directory=str(tmp_path), device=device)
    if model_type == "VAE":
        model = VariationalAutoencoder(**kw)
    else:
        model = GaussianMixtureVariationalAutoencoder(
            number_of_latent_clusters=K, **kw)
    # (the plan takes a uint16 minibatch where its products with the count
    #  matrix run on the exact split kernels, by default from cells * F of
    #  768 x 32768 -- a step of the full-size set: at F = 300 these passes
    #  take that path when asked to always)
    model.engine.set_count_gemm(True, always=True)
    return model


def _perturb(model, seed=9):
    """Non-trivial parameters (Glorot weights scaled per tensor, biases and
    beta off zero) and moving statistics away from (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    engine = model.engine
    for name, p in engine.named_parameters().items():
        if name.endswith("weights"):
            p.mul_(0.75 + 0.5 * torch.rand((), generator=g).item())
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    for name, m in engine.named_moving_statistics().items():
        if name.endswith("moving_variance"):
            m.copy_(torch.rand(m.shape, generator=g) + 0.5)
        else:
            m.copy_(torch.randn(m.shape, generator=g) * 0.3)


def _philox(device, rows, cols, seed, stream_id):
    from scvae_amd.minibatch import philox_normal
    out = torch.empty(rows, cols, device=device)
    philox_normal(out, 0, seed, stream_id)
    return out.cpu().double()


def _oracle_pass(model, values, B, n_iw=1, n_mc=1, counter=None,
                 deterministic_z=False):
    """The reference's pass in fp64: one oracle call per minibatch of B
    sequential cells, ``sum_j mean_j / (N / B)``; noise of pass ``counter``."""
    engine = model.engine
    if counter is None:
        counter = model._evaluation_counter
    gm = model.type == "GMVAE"
    n, F = values.shape
    L = model.latent_size
    cfg = om.ModelConfig(
        feature_size=F, latent_size=L, hidden_sizes=tuple(model.hidden_sizes),
        likelihood=model.reconstruction_distribution_name,
        minibatch_normalisation=bool(model.minibatch_normalisation),
        n_iw=n_iw, n_mc=n_mc, kl_weight=model.kl_weight_value,
        **(dict(n_clusters=model.n_clusters,
                prior_probabilities_method=model.prior_probabilities_method)
           if gm else dict(analytical_kl_term=bool(model.analytical_kl_term))))
    params = {k: v.detach().cpu().double()
              for k, v in engine.named_parameters().items()}
    moving = {k: v.detach().cpu().double()
              for k, v in engine.named_moving_statistics().items()}
    x = torch.from_numpy(np.asarray(values, dtype=np.float64))
    shape = model._eps_shape(1 if deterministic_z else n_iw * n_mc, n)
    eps_all = None
    if not deterministic_z:
        blocks = int(np.prod(shape[:-2]))
        eps_all = _philox(engine.device, blocks * n, L, model.noise_seed,
                          (1 << 40) + counter * (1 << 20)).reshape(shape)
    tags = ([t for _, t, _ in model._loss_tags()]
            + (["kl_divergence"] if gm else []))
    totals = dict.fromkeys(tags, 0.0)
    kl_neurons = 0.0
    latent = []
    for i in range(0, n, B):
        xb = x[i:i + B]
        eps = None if eps_all is None else eps_all[..., i:i + B, :]
        if gm:
            out = om.gmvae_forward(cfg, params, moving, xb, xb, eps, False)
            latent.append(out["z_mean"])
        else:
            out = om.vae_forward(cfg, params, moving, xb, xb, eps, False,
                                 deterministic_z=deterministic_z)
            latent.append(out["q_z_mean"])
            kl_neurons = kl_neurons + out["kl_divergence_neurons"]
        for tag in tags:
            totals[tag] += float(out[tag])
    denominator = n / B
    want = {tag: value / denominator for tag, value in totals.items()}
    want["kl_divergence_neurons"] = (
        np.array([want["kl_divergence"]]) if gm
        else (kl_neurons / denominator).numpy())
    want["latent_values"] = torch.cat(latent).numpy()
    return want


def _assert_oracle(got, want, what=""):
    for tag, value in want.items():
        if tag == "latent_values":
            close_maxnorm(got[tag], value, Q_Z_MEAN_RTOL, what=what + tag)
        elif tag == "kl_divergence_neurons":
            close_elementwise(got[tag], value, rtol=ELBO_RTOL,
                              what=what + tag)
        else:
            close_scalar(got[tag], value,
                         rtol=KL_Y_RTOL if tag == "kl_divergence_y"
                         else ELBO_RTOL, what=what + tag)


@pytest.fixture
def steps(monkeypatch):
    """Every ``Engine.step`` as (training, cells, uint16 minibatch, carries
    the next step's fetch / noise, workspace address and cells before /
    after)."""
    from scvae_amd.engine import Engine
    seen = []
    step = Engine.step

    def spy(self, x, t, *args, **kwargs):
        before = (self.workspace.data_ptr() if self.workspace is not None
                  else None, self.max_cells)
        result = step(self, x, t, *args, **kwargs)
        seen.append(dict(
            training=bool(kwargs.get("training")), cells=int(x.shape[0]),
            u16=x.dtype == torch.uint16,
            carries=kwargs.get("next_minibatch") is not None,
            carries_noise=kwargs.get("next_noise") is not None,
            before=before,
            after=(self.workspace.data_ptr(), self.max_cells)))
        return result
    monkeypatch.setattr(Engine, "step", spy)
    return seen


def _eval_chain(model, cells, samples):
    """plan.hip ``eval_chain_ok`` written out for the models built here (batch
    norm, plain MLP, no decoder extra, single process): the hidden stack of
    an evaluation step is one ``eval_mlp_kernel`` launch."""
    H = list(model.hidden_sizes)
    return (os.environ.get("SCVAE_EVAL_CHAIN", "1")[:1] != "0"
            and model.type == "VAE" and samples == 1 and cells * samples > 128
            and model.latent_size <= 128 and max(H) <= 128
            and (len(H) - 1) + 2 + len(H) <= 10)


def _chunks(n, B, cells):
    from scvae_amd.models.utilities import evaluation_chunks
    return [c for _, c, _ in evaluation_chunks(n, B, cells)]


# ---------------------------------------------------------------------------
# 1. every path of the pass against the oracle
# ---------------------------------------------------------------------------

def test_stacked_uint16_carried_pass_then_resident_pass(tmp_path, cuda_device,
                                                         steps):
    """The product's default: B = 100, 40 minibatches per step of 4000 cells
    on ``eval_mlp_kernel``, uint16, each step carrying the next one's fetch and
    noise, the ragged tail of 37 cells on a step of its own (mid-chain
    regime).  The second pass reads every step from the resident copy -- and
    equals the oracle, not only the first pass."""
    n, B = 2 * 40 * 100 + 37, 100
    values = _values(n, F_DEFAULT)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device)
    _perturb(model)
    x, t = model._device_matrices(data)
    assert x is t and x.integer_counts
    assert _chunks(n, B, model._evaluation_step_cells(1)) == [4000, 4000, 37]
    for number in (1, 2):
        del steps[:]
        hits = model._evaluation_resident_hits
        got = model._evaluation_pass(x, t, data, B, 1, 1)
        assert [s["cells"] for s in steps] == [4000, 4000, 37]
        assert all(s["u16"] for s in steps)
        # (the second pass finds every minibatch there: a step carries the
        #  next one's noise, nothing to fetch)
        assert [s["carries"] for s in steps] == (
            [True, True, False] if number == 1 else [False] * 3)
        assert [s["carries_noise"] for s in steps] == [True, True, False]
        assert [_eval_chain(model, s["cells"], 1) for s in steps] == [
            True, True, False]
        assert model._evaluation_resident_hits - hits == (
            0 if number == 1 else 3)
        _assert_oracle(got, _oracle_pass(model, values, B),
                       what="pass {}: ".format(number))


@pytest.mark.parametrize("B,cells,chain", [(43, 129, True), (64, 128, False)])
def test_either_side_of_the_eval_chain_boundary(tmp_path, cuda_device, steps,
                                                B, cells, chain):
    """Steps of 3 x 43 = 129 cells take ``eval_mlp_kernel``, steps of
    2 x 64 = 128 the mid-chain kernels (``B * S <= 128``)."""
    n = 700
    values = _values(n, F_DEFAULT, seed=4)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device)
    _perturb(model, seed=10)
    model.evaluation_chunk_cells = cells
    x, t = model._device_matrices(data)
    got = model._evaluation_pass(x, t, data, B, 1, 1)
    sizes = [s["cells"] for s in steps]
    assert sizes == _chunks(n, B, cells) and sizes[0] == cells
    assert all(s["u16"] for s in steps) and steps[0]["carries"]
    assert _eval_chain(model, cells, 1) == chain
    _assert_oracle(got, _oracle_pass(model, values, B))


@pytest.mark.parametrize("H,L", [((64, 128), 8), ((64, 129), 8),
                                 (H_DEFAULT, 128), (H_DEFAULT, 129)])
def test_either_side_of_the_eval_chain_widths(tmp_path, cuda_device, steps,
                                              H, L):
    """Hidden and latent widths of 128 run the stacked steps on
    ``eval_mlp_kernel``; 129 on the launches."""
    n, B = 1337, 100
    values = _values(n, F_DEFAULT, seed=5)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device, H=H, L=L)
    _perturb(model, seed=11)
    x, t = model._device_matrices(data)
    got = model._evaluation_pass(x, t, data, B, 1, 1)
    assert [s["cells"] for s in steps] == [1300, 37]
    assert all(s["u16"] for s in steps) and steps[0]["carries"]
    assert _eval_chain(model, 1300, 1) == (max(H) <= 128 and L <= 128)
    _assert_oracle(got, _oracle_pass(model, values, B))


@pytest.mark.parametrize("n_iw,n_mc,deterministic_z", [
    (1, 1, True), (2, 2, False)])
def test_deterministic_z_and_several_samples(tmp_path, cuda_device, steps,
                                             n_iw, n_mc, deterministic_z):
    """The deterministic z = mu of the one-launch path; four importance /
    Monte-Carlo samples per cell (S > 1: the launch chain)."""
    n, B = 2037, 100
    values = _values(n, F_DEFAULT, seed=6)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device)
    _perturb(model, seed=12)
    x, t = model._device_matrices(data)
    got = model._evaluation_pass(x, t, data, B, n_iw, n_mc,
                                 deterministic_z=deterministic_z)
    samples = 1 if deterministic_z else n_iw * n_mc
    assert [s["cells"] for s in steps] == [2000, 37]
    assert all(s["u16"] for s in steps) and steps[0]["carries"]
    assert _eval_chain(model, 2000, samples) == deterministic_z
    _assert_oracle(got, _oracle_pass(model, values, B, n_iw, n_mc,
                                     deterministic_z=deterministic_z))


def test_stacked_pass_of_non_integer_values(tmp_path, cuda_device, steps):
    """fp32 values: stacked steps gathered with ``gather_dense``."""
    n, B = 2037, 100
    values = _values(n, F_DEFAULT, seed=7, integer=False)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device)
    _perturb(model, seed=13)
    x, t = model._device_matrices(data)
    assert not x.integer_counts
    got = model._evaluation_pass(x, t, data, B, 1, 1)
    assert [s["cells"] for s in steps] == [2000, 37]
    assert not any(s["u16"] or s["carries"] for s in steps)
    _assert_oracle(got, _oracle_pass(model, values, B))


def test_stacked_gmvae_pass(tmp_path, cuda_device, steps):
    """The GMVAE (K = 3) in stacked steps; its per-cell latent values are
    the y-weighted posterior means."""
    n, B = 2037, 100
    values = _values(n, F_DEFAULT, seed=8)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device, model_type="GMVAE", K=3)
    _perturb(model, seed=14)
    x, t = model._device_matrices(data)
    got = model._evaluation_pass(x, t, data, B, 1, 1)
    assert [s["cells"] for s in steps] == [2000, 37]
    _assert_oracle(got, _oracle_pass(model, values, B))


# ---------------------------------------------------------------------------
# 2. step sizing under memory pressure
# ---------------------------------------------------------------------------

def _workspace_bytes(model, cells, samples=1):
    engine = model.engine
    return int(engine.lib.scvae_plan_workspace_bytes(
        engine.handle, int(cells), int(samples)))


def _fake_free(monkeypatch, free):
    """``torch.cuda.mem_get_info`` reports ``free`` bytes (of the real
    total): the sizing decisions see pressure, the allocations do not."""
    real = torch.cuda.mem_get_info

    def fake(device=None):
        return int(free), real(device)[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", fake)


def test_pass_under_a_tight_budget(tmp_path, cuda_device, steps, monkeypatch):
    """Where half of what is free holds the workspace of 1024 cells but not
    of 2048, the pass runs steps of 10 minibatches -- and equals the oracle
    like the unpressured pass."""
    n, B = 8037, 100
    values = _values(n, F_DEFAULT, seed=15)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device)
    _perturb(model, seed=16)
    x, t = model._device_matrices(data)
    assert model.engine.workspace is None
    _fake_free(monkeypatch, 2 * _workspace_bytes(model, 1024) + 1)
    assert model._evaluation_step_cells(1) == 1024
    got = model._evaluation_pass(x, t, data, B, 1, 1)
    assert [s["cells"] for s in steps] == [1000] * 8 + [37]
    assert all(s["u16"] for s in steps) and steps[0]["carries"]
    _assert_oracle(got, _oracle_pass(model, values, B))


def test_workspace_stays_bound_from_reserve_to_the_epoch_end_passes(
        tmp_path, cuda_device, steps, monkeypatch):
    """A budget where the step ``train`` reserves for is 2048 cells (c / 2)
    but the same budget, asked again at the epoch-end pass -- with the
    reserved workspace counted as held -- admits 4096 (c): the pass must step
    as was reserved.  The workspace is bound once, before the first training
    step, and the epoch-end pass (training and validation set) equals the
    oracle at the trained state."""
    n, n_valid, B = 8037, 2037, 100
    values = _values(n + n_valid, F_DEFAULT, seed=17)
    training_set = _data_set(values[:n])
    validation_set = _data_set(values[n:], kind="validation")
    model = _model(tmp_path, cuda_device)
    assert model.engine.workspace is None
    half = max(_workspace_bytes(model, 2048),
               _workspace_bytes(model, 4096) - _workspace_bytes(model, 2000)
               - 256)
    assert half < _workspace_bytes(model, 4096)
    _fake_free(monkeypatch, 2 * half + 1)
    results = []
    evaluation_pass = model._evaluation_pass

    def kept(*args, **kwargs):
        result = evaluation_pass(*args, **kwargs)
        results.append((result, model._evaluation_counter))
        return result
    model._evaluation_pass = kept
    assert model.train(training_set, validation_set, number_of_epochs=1,
                       minibatch_size=B, learning_rate=1e-3) == 0
    assert len(results) == 2
    bound = {s["before"] for s in steps} | {s["after"] for s in steps}
    assert len(bound) == 1, bound
    assert next(iter(bound))[1] == 2000
    evaluation = [s["cells"] for s in steps if not s["training"]]
    assert evaluation == [2000] * 4 + [37] + [2000, 37]
    for (got, counter), part in zip(results, (values[:n], values[n:])):
        _assert_oracle(got, _oracle_pass(model, part, B, counter=counter))


def _dp_run(directory, values, B, free):
    """``model.train`` (one epoch) and a plain ``model.evaluate`` of
    ``values``; the results of their passes."""
    model = _model(directory, "cuda:0")
    data = _data_set(values)
    if free is not None:
        real = torch.cuda.mem_get_info
        torch.cuda.mem_get_info = lambda device=None: (
            int(free), real(device)[1])
    results = []
    evaluation_pass = model._evaluation_pass

    def kept(*args, **kwargs):
        results.append(evaluation_pass(*args, **kwargs))
        return results[-1]
    model._evaluation_pass = kept
    np.random.seed(11)
    assert model.train(data, None, number_of_epochs=1, minibatch_size=B,
                       learning_rate=1e-6) == 0
    model.evaluate(data, minibatch_size=B, log_results=False,
                   output_versions="latent")
    return results


def _rank_main(rank, port, directory):
    """One of two data-parallel ranks on cuda:0 (gloo): rank 1 sees a fourth
    of rank 0's step in free memory."""
    import torch.distributed as dist
    import datetime
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=120))
    try:
        values = np.load(os.path.join(directory, "values.npy"))
        free = None
        if rank == 1:
            probe = _model(os.path.join(directory, "probe"), "cuda:0")
            free = 2 * _workspace_bytes(probe, 1024) + 1
            del probe
        results = _dp_run(os.path.join(directory, "dp"), values, 100, free)
        if rank == 0:
            np.save(os.path.join(directory, "dp.npy"),
                    np.array(results, dtype=object), allow_pickle=True)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_ranks_with_different_free_memory_agree(tmp_path, cuda_device):
    """Two ranks, one of which sees little free memory: they step the
    evaluation passes alike (the smallest size), so every cell is evaluated
    once and the scalars all-reduced are of one shape.  The epoch-end pass
    of ``train`` and a plain ``evaluate`` (curves and latent values) equal
    one process's passes at the state the ranks trained.  The ranks run as
    child processes under a time limit: a disagreement fails instead of
    hanging."""
    n = 4 * 1000 + 37
    values = _values(n, F_DEFAULT, seed=18)
    np.save(tmp_path / "values.npy", values)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    code = ("import sys; sys.path[:0] = [{!r}, {!r}]; "
            "import test_gpu_evaluation_passes as m; "
            "m._rank_main({{}}, {}, {!r})").format(
                ROOT, os.path.join(ROOT, "tests"), port, str(tmp_path))
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(key, None)
    ranks = [subprocess.Popen([sys.executable, "-c", code.format(rank)],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
             for rank in range(2)]
    outputs = []
    try:
        for rank in ranks:
            outputs.append(rank.communicate(timeout=600)[0])
    finally:
        for rank in ranks:
            if rank.poll() is None:
                rank.kill()
                rank.wait()
    assert [r.returncode for r in ranks] == [0, 0], "\n".join(
        o[-3000:] for o in outputs)
    got = np.load(tmp_path / "dp.npy", allow_pickle=True)
    assert len(got) == 2
    # one process evaluates the state the ranks left (their checkpoint) with
    # the noise of the ranks' two passes
    single = _model(tmp_path / "dp", cuda_device)
    want = []
    evaluation_pass = single._evaluation_pass

    def kept(*args, **kwargs):
        want.append(evaluation_pass(*args, **kwargs))
        return want[-1]
    single._evaluation_pass = kept
    for counter in (0, 1):
        single._evaluation_counter = counter
        single.evaluate(_data_set(values), minibatch_size=100,
                        log_results=False, output_versions="latent")
    for one, two in zip(got, want):
        for tag in ("lower_bound", "reconstruction_error", "kl_divergence"):
            close_scalar(one[tag], two[tag], rtol=ELBO_RTOL, what=tag)
        close_elementwise(one["kl_divergence_neurons"],
                          two["kl_divergence_neurons"], rtol=ELBO_RTOL,
                          what="kl_divergence_neurons")
        close_maxnorm(one["latent_values"], two["latent_values"],
                      Q_Z_MEAN_RTOL, what="latent_values")


# ---------------------------------------------------------------------------
# 3. a step that raises inside a resident, carried pass
# ---------------------------------------------------------------------------

def test_resident_rows_of_a_step_that_raised_are_fetched_again(
        tmp_path, cuda_device, steps, monkeypatch):
    """The fourth step of a resident, carried pass raises (on the host, before
    anything is launched).  Only the rows of steps issued before it -- the
    first four minibatches of 1000 cells: the three steps run and the fetch
    the third one carried -- count as resident; the rest of the copy holds
    whatever its memory held (here: a fill that is no count matrix's).  The
    pass run again finds four steps there, fetches the others and equals the
    oracle."""
    from scvae_amd.engine import Engine
    n, B = 8037, 100
    values = _values(n, F_DEFAULT, seed=19)
    data = _data_set(values)
    model = _model(tmp_path, cuda_device)
    _perturb(model, seed=20)
    model.evaluation_chunk_cells = 1000
    x, t = model._device_matrices(data)
    step = Engine.step
    calls = []

    def failing(self, *args, **kwargs):
        calls.append(1)
        if len(calls) == 4:
            raise RuntimeError("injected")
        return step(self, *args, **kwargs)
    monkeypatch.setattr(Engine, "step", failing)
    with pytest.raises(RuntimeError, match="injected"):
        model._evaluation_pass(x, t, data, B, 1, 1)
    monkeypatch.setattr(Engine, "step", step)
    torch.cuda.synchronize()
    assert len(steps) == 3 and all(s["u16"] and s["carries"] for s in steps)
    dense, constants, filled = x._evaluation_resident
    assert filled[:4000].all() and not filled[4000:].any()
    dense[4000:].view(torch.int16).fill_(7)
    constants[4000:] = 0.0
    del steps[:]
    hits = model._evaluation_resident_hits
    got = model._evaluation_pass(x, t, data, B, 1, 1)
    assert len(steps) == 9 and model._evaluation_resident_hits - hits == 4
    assert filled.all()
    _assert_oracle(got, _oracle_pass(model, values, B))
