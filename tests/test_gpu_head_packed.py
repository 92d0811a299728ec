"""The packed remainder block of the producer / consumer head kernel against
the fp64 oracle (``oracle/likelihoods.py`` through torch fp64 autograd).

Where the contraction length H + 1 leaves at most 8 live rows in its last
32-wide block (H + 1 in 33..40, 65..72, 97..104) that block carries the three
bf16 terms of its rows side by side and costs three MFMAs per step instead of
nine in GEMM1, GEMM2 and GEMM3.  The comparison and the tolerances are those
of ``_run`` in ``tests/test_gpu_fused_decoder.py``: ``ll`` to 2e-5 of the
largest value + 1e-4; ``dd``, ``dW``, ``db`` to 3e-5 of the largest element.
The split terms of second order, far below these tolerances, are held by the
single-product probes of ``test_gpu_head_probes.py``.

Shapes: 200 rows (beyond 128 the producer / consumer kernel runs; seven
32-row tiles, the last ragged), F = 196 for one and two heads and F = 90 for
three (a ragged last strip).  Widths: rem = 1 and 8 at each of the three step
counts, and the first unpacked width on either side (40, 104).

``python tests/test_gpu_head_packed.py old-kernel|row-groups`` runs the cases
whose switch is read once per process (``SCVAE_D3_SCHEDULE``,
``SCVAE_D4_ROW_GROUPS``) in this process.
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

from oracle import likelihoods as lk  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 200
WIDTHS = [32, 39, 40, 71, 96, 100, 103, 104]
NAMES = ["poisson", "negative binomial", "zero-inflated negative binomial"]
SENTINEL = 7.0


def _genes(name):
    return 90 if name.startswith("zero-inflated negative") else 196


def _h0(H):
    """First row of the remainder block."""
    return 32 * ((H + 1 + 31) // 32 - 1)


@functools.lru_cache(maxsize=None)
def _case(name, rows, F, H, isolate=False, seed=0):
    """Inputs (numpy fp64) and the fp64 reference of one shape; computed once
    and shared.  ``isolate``: d[:, :h0] = 0 -- only the remainder block's
    columns and the bias drive the heads."""
    from scvae_amd import _lib
    P = len(_lib.LIKELIHOOD_KINDS[name][1])
    rng = np.random.default_rng(seed + H)
    d = np.maximum(rng.normal(0, 1, (rows, H)), 0)
    if isolate:
        d[:, :_h0(H)] = 0.0
        d[:, _h0(H):] += 0.25          # (no dead columns in the block)
    W = [rng.normal(0, 0.3, (H, F)) for _ in range(P)]
    b = [rng.normal(0, 0.3, F) for _ in range(P)]
    t = rng.poisson(3.0, (rows, F)) * (rng.random((rows, F)) < 0.2)
    t = t.astype(np.float64)
    t.flat[0] = 5000.0
    gw = rng.normal(0, 1, rows)
    T = torch.from_numpy
    dt = T(d).requires_grad_(True)
    Wt = [T(w).requires_grad_(True) for w in W]
    bt = [T(v).requires_grad_(True) for v in b]
    pre = tuple(dt @ w + v for w, v in zip(Wt, bt))
    ll = lk.log_prob(name, T(t), pre).sum(dim=1)
    (ll * T(gw)).sum().backward()
    ref = {"ll": ll.detach().numpy(), "dd": dt.grad.numpy(),
           "dW": [w.grad.numpy() for w in Wt], "db": [v.grad.numpy() for v in bt]}
    for a in [d, t, gw] + W + b + [ref["ll"], ref["dd"]] + ref["dW"] + ref["db"]:
        a.setflags(write=False)
    return {"name": name, "rows": rows, "F": F, "H": H, "P": P, "d": d, "W": W,
            "b": b, "t": t, "gw": gw, "ref": ref}


def _launch(device, case, train, flags, targets="f32", launches=1):
    """One call (or ``launches`` calls into fresh outputs) of the stand-alone
    entry.  Outputs live in buffers pre-filled with a sentinel and larger than
    what the call may write: dW_j as [H + 3, F], dd as [rows + 2, H]."""
    from scvae_amd import _lib
    lib = _lib.load()
    kind = _lib.LIKELIHOOD_KINDS[case["name"]][0]
    rows, F, H, P = case["rows"], case["F"], case["H"], case["P"]
    f32 = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(device)
    d, gw, t = f32(case["d"]), f32(case["gw"]), f32(case["t"])
    W, b = [f32(w) for w in case["W"]], [f32(v) for v in case["b"]]
    rc = torch.lgamma(t.double() + 1).sum(dim=1).float()
    if targets == "u16":
        ld = (F + 63) // 64 * 64
        t16 = torch.zeros(rows, ld, dtype=torch.int32, device=device)
        t16[:, :F] = t.to(torch.int32)
        t16 = t16.to(torch.uint16)
    nbytes = lib.scvae_decoder_fused_workspace_bytes(rows, H, F)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for _ in range(launches):
        ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=device)
        dW = [torch.full((H + 3, F), SENTINEL, device=device) for _ in range(P)]
        db = [torch.full((F + 3,), SENTINEL, device=device) for _ in range(P)]
        ll = torch.full((rows + 2,), SENTINEL, device=device)
        dd = torch.full((rows + 2, H), SENTINEL, device=device)
        head = (kind, train | flags, d.data_ptr(), rows, H, arr(W), arr(b),
                arr(dW), arr(db), F)
        tail = (rows, gw.data_ptr(), rc.data_ptr(), ll.data_ptr(),
                dd.data_ptr(), ws.data_ptr(), stream)
        if targets == "u16":
            _lib.check(lib.scvae_decoder_fused_u16(*head, t16.data_ptr(), ld, *tail),
                       "scvae_decoder_fused_u16")
        else:
            _lib.check(lib.scvae_decoder_fused(*head, t.data_ptr(), *tail),
                       "scvae_decoder_fused")
        torch.cuda.synchronize()
        outs.append({"ll": ll, "dd": dd, "dW": dW, "db": db, "ws": ws})
    return outs if launches > 1 else outs[0]


def _close(got, want, what, rel=3e-5, extra=0.0):
    got = got.cpu().double().numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= rel * scale + extra, (what, err, scale)


def _check_ll(out, case, what):
    rows = case["rows"]
    _close(out["ll"][:rows], case["ref"]["ll"], what + " ll", rel=2e-5, extra=1e-4)
    assert bool((out["ll"][rows:] == SENTINEL).all()), what


def _check(out, case, what):
    """ll, dd, dW_j, db_j against the oracle, and the sentinel around them."""
    rows, F, H, P = case["rows"], case["F"], case["H"], case["P"]
    _check_ll(out, case, what)
    _close(out["dd"][:rows], case["ref"]["dd"], what + " dd")
    assert bool((out["dd"][rows:] == SENTINEL).all()), what
    for j in range(P):
        _close(out["dW"][j][:H], case["ref"]["dW"][j], "%s dW%d" % (what, j))
        _close(out["db"][j][:F], case["ref"]["db"][j], "%s db%d" % (what, j))
        assert bool((out["dW"][j][H:] == SENTINEL).all()), what
        assert bool((out["db"][j][F:] == SENTINEL).all()), what


def _flags():
    from scvae_amd import _lib
    return _lib.HEADS_BF16X9, _lib.HEADS_BF16X6, _lib.HEADS_DD_ATOMICS


def _packed_kernel_runs(name, H, rows=ROWS):
    """What the library says it launches for this training call."""
    from scvae_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)
    _lib.check(lib.scvae_decoder_train_kernel_name(
        _lib.LIKELIHOOD_KINDS[name][0], H, rows, 1, 0, buf, 128), "kernel name")
    kernel = buf.value.decode()
    assert kernel.startswith("decoder_head4_kernel<"), kernel
    return kernel.endswith(", true>")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("H", WIDTHS)
def test_widths_against_the_oracle(cuda_device, name, H):
    """rem = 1 and 8 at two, three and four contraction steps, and the first
    unpacked width on either side: forward half, training through slabs and
    through atomics."""
    x9, _, atomics = _flags()
    rem = H + 1 - _h0(H)
    assert _packed_kernel_runs(name, H) == (1 <= rem <= 8 and H + 1 > 32)
    case = _case(name, ROWS, _genes(name), H)
    _check_ll(_launch(cuda_device, case, 0, x9), case, "forward")
    _check(_launch(cuda_device, case, 1, x9), case, "slabs")
    _check(_launch(cuda_device, case, 1, x9 | atomics), case, "atomics")


@pytest.mark.parametrize("targets", ["f32", "u16"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("H", [100, 39])
def test_targets_and_dd_paths(cuda_device, H, name, targets):
    """fp32 and uint16 targets, dd through atomics and through slabs; the slab
    mode is bit-repeatable from launch to launch."""
    x9, _, atomics = _flags()
    case = _case(name, ROWS, _genes(name), H)
    _check(_launch(cuda_device, case, 1, x9 | atomics, targets), case, "atomics")
    first, second = _launch(cuda_device, case, 1, x9, targets, launches=2)
    _check(first, case, "slabs")
    assert torch.equal(first["ll"], second["ll"])
    assert torch.equal(first["dd"], second["dd"])
    for j in range(case["P"]):
        assert torch.equal(first["dW"][j], second["dW"][j])
        assert torch.equal(first["db"][j], second["db"][j])


@pytest.mark.parametrize("name", NAMES)
def test_six_term_arithmetic(cuda_device, name):
    """One case per head count: under the six-term arithmetic the packed block
    still carries all nine terms (three MFMAs)."""
    _, x6, atomics = _flags()
    case = _case(name, ROWS, _genes(name), 100)
    _check(_launch(cuda_device, case, 1, x6), case, "six terms, slabs")
    _check(_launch(cuda_device, case, 1, x6 | atomics), case, "six terms, atomics")


@pytest.mark.parametrize("dd_path", ["atomics", "slabs"])
@pytest.mark.parametrize("name", NAMES[1:])
@pytest.mark.parametrize("H", [100, 39])
def test_packed_block_alone(cuda_device, H, name, dd_path):
    """d[:, :h0] = 0: only the packed columns and the bias drive the heads, and
    the packed rows of dW, db and the packed columns of dd are held to the
    oracle on the scale of those rows and columns ALONE.  Every row h < H of
    dW and every column of dd is written, nothing beyond them."""
    x9, _, atomics = _flags()
    case = _case(name, ROWS, _genes(name), H, isolate=True)
    rows, F, P, h0 = case["rows"], case["F"], case["P"], _h0(H)
    out = _launch(cuda_device, case, 1, x9 | (atomics if dd_path == "atomics" else 0))
    _check(out, case, "isolated")
    ref = case["ref"]
    assert np.abs(ref["dd"][:, h0:]).max() > 0
    _close(out["dd"][:rows, h0:], ref["dd"][:, h0:], "dd[:, h0:H]")
    for j in range(P):
        assert np.abs(ref["dW"][j][h0:]).max() > 0
        _close(out["dW"][j][h0:H], ref["dW"][j][h0:], "dW%d[h0:H]" % j)
        _close(out["db"][j][:F], ref["db"][j], "db%d" % j)
        # rows below h0 multiply zeros: exactly zero; every row h < H written
        assert bool((out["dW"][j][:h0] == 0).all())
        assert not bool((out["dW"][j][:H] == SENTINEL).any())
        assert bool((out["dW"][j][H:] == SENTINEL).all())
    assert not bool((out["dd"][:rows] == SENTINEL).any())
    assert bool((out["dd"][rows:] == SENTINEL).all())


def _slab_words(out, case):
    """The first row group's part of the workspace's dW / db slabs (its last
    region: 3 groups x 3 heads x [H + 1][F] floats + 64, + 64 of alignment)."""
    F, H, P = case["F"], case["H"], case["P"]
    floats = 3 * 3 * (H + 1) * F + 64 + 64
    return out["ws"].view(torch.int32)[-floats:][:P * (H + 1) * F]


def _row_group_case(device, name, rows, F, H):
    x9, _, atomics = _flags()
    case = _case(name, rows, F, H)
    for flags in (x9, x9 | atomics):
        out = _launch(device, case, 1, flags)
        # more than one row group ran: the second group's slab holds its sums
        assert not bool((_slab_words(out, case) == 0x5A5A5A5A).any()), (name, H)
        _check(out, case, "row groups")


def test_row_groups_by_the_launch_rule(cuda_device):
    """Enough strips (12) that d4_row_groups cuts 600 rows into two groups by
    its own rule: the packed rows of dW / db pass through the combine kernel."""
    _row_group_case(cuda_device, "negative binomial", 600, 710, 100)


def _child(mode, **env):
    done = subprocess.run(
        [sys.executable, os.path.abspath(__file__), mode],
        env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
        text=True, timeout=600, cwd=ROOT)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert mode + " ok" in done.stdout


def test_row_groups_on_a_few_strips(cuda_device):
    """600 rows x 130 genes with two row groups (three and five strips: the
    launch rule alone would keep one group -- ``SCVAE_D4_ROW_GROUPS=2``, read
    once per process, so a child process)."""
    _child("row-groups", SCVAE_D4_ROW_GROUPS="2")


def test_old_kernel_reads_the_plain_planes(cuda_device):
    """``SCVAE_D3_SCHEDULE=3`` (read once per process): the all-in-one-phase
    kernel at 200 rows, H = 100 -- its planes must come in the plain layout."""
    _child("old-kernel", SCVAE_D3_SCHEDULE="3")


def test_row_index_is_the_gathered_step(cuda_device):
    """``counts_rows`` through the engine at 200 rows, H = 100, NB: the indexed
    head kernel (packed as well) is bit-identical to the step on the gathered
    rows -- the check of ``tests/test_gpu_resident_rows.py`` at this size."""
    import test_gpu_resident_rows as resident
    assert resident.H[-1] == 100
    resident._check_indexed_step(cuda_device, "negative binomial", ROWS, 1000)


if __name__ == "__main__":
    device = torch.device("cuda:0")
    if sys.argv[1:] == ["old-kernel"]:
        assert os.environ.get("SCVAE_D3_SCHEDULE") == "3"
        x9, _, _ = _flags()
        for name in NAMES:
            from scvae_amd import _lib
            buf = ctypes.create_string_buffer(128)
            _lib.check(_lib.load().scvae_decoder_train_kernel_name(
                _lib.LIKELIHOOD_KINDS[name][0], 100, ROWS, 1, 0, buf, 128), "name")
            assert buf.value.decode().startswith("decoder_head3_kernel<")
            case = _case(name, ROWS, _genes(name), 100)
            _check(_launch(device, case, 1, x9), case, "old kernel")
    elif sys.argv[1:] == ["row-groups"]:
        assert os.environ.get("SCVAE_D4_ROW_GROUPS") == "2"
        for name in NAMES[1:]:
            for width in (100, 39):
                _row_group_case(device, name, 600, 130, width)
    else:
        raise SystemExit("usage: test_gpu_head_packed.py old-kernel|row-groups")
    print(sys.argv[1] + " ok")
