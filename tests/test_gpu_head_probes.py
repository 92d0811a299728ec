"""The fused decoder-head kernels held to their own promise -- every fp32
operand cut exactly into three bf16 terms, all nine (or six) products of a pair
accumulated in fp32 -- by the single-product probes of ``_head_probes.py``:
inputs that make every checked output element ONE product of two full-mantissa
fp32 numbers plus exact zeros, so that a lost, doubled or mis-paired term of
second order (2^-18 of a product, 10 to 1000 times below the tolerances of the
dense oracle tests) stands at least twice the bound away
(``test_head_probes_host.py`` proves that on the CPU).

Per launch geometry three probes, three seeds each, through
``scvae_decoder_fused`` / ``scvae_decoder_fused_u16`` with the sentinel-padded
outputs of ``test_gpu_head_packed.py``:

* GEMM3 probe: dW_j[h, f] = d[r(h), h] gw_r(h) c_j for every (h, f); db_j; dd
  exactly 0;
* GEMM2 probe: dd[r, h] = gw_r c_J W_J[h, f_J(h)] (+ 2^-40 of the other heads)
  for every (r, h); db_j; dW exactly 0;
* GEMM1 probe: pre = d W of magnitude 6 to 9.5 seen through the exponential of
  the gradient in dd[r, h(r)] and dW_J[h, f(h)] (training; the pi head of the
  zero-inflated kind with t = 1 on its live gene, where its gradient is
  -sigmoid(pre)) or of ll[r] (forward-only launches, |pre| from 8, the
  exponential heads log_lambda and log_r ONLY: the sigmoid heads' forward
  GEMM1 stays with the existing tests; the zero-inflated kind with t = 1 on
  the live gene, since at t = 0 its log likelihood never falls below
  log 1/2).  Columns without a live row (H > rows) have dW exactly 0.

Every case first asserts the kernel the library says it launches
(``scvae_decoder_train_kernel`` / ``scvae_decoder_train_kernel_name``: the
template arguments steps, producer waves, strip, DBP, terms, PACK), then every
probed element against its exact value and bound, the elements that must be
exactly zero, and the sentinel around the outputs.  Two assertions are weaker
than a kernel's name, because the library has no more to say: for the fp32
arithmetic ``scvae_decoder_train_kernel_name`` leaves the pipelined kernel's
last template argument open ("true|false"), and no query names the kernel of
a forward-only launch -- those cases assert the inputs of
``decoder_forward_choice`` (width, head count, no override in the
environment) instead.  A failure reports the worst
element with its (row mod 32, h, h mod 32, f mod strip, head).

Geometries (``d4_config`` / ``d4_launch_steps`` / ``d3_schedule``): 200 rows
(seven 32-row tiles, the last ragged) for the producer / consumer kernel, 100
rows for the all-in-one-phase kernel, F = P H + 5 (a ragged last strip).  Two
heads keep 64-gene strips up to H = 111 (the weight planes are padded to
H + 1 in sixteens: 112 rows fit LDS) and take 32-gene strips from 112; at
H = 126 and 100 rows they run the producer / consumer kernel as well, the
all-in-one-phase kernel having no room for them.

Out of scope: the ``_rows`` kernels (reached only through a step with
``counts_rows``; ``test_gpu_resident_rows.py`` holds them bit-identical to
their siblings), the head-dropout, the constrained-Poisson and the categorised
instantiations.

Worst |error| / bound on the MI355X over all cases and seeds (none may exceed
1; PRODUCT is the GEMM2 / GEMM3 probes' single products, where the bound is
8 u -- u for fp32 -- plus the constant's widening; every test prints its own):

    kernel family                              PRODUCT  sums (db)  through GEMM1
    producer / consumer, nine terms             0.251    0.024      0.216
    producer / consumer, packed block           0.280    0.013      0.285
    producer / consumer, six terms              0.274    0.023      0.278
    producer / consumer, uint16 targets         0.280    0.010      0.194
    producer / consumer, dd through atomics     0.280    0.002      --
    producer / consumer, two row groups         0.174    0.004      --
    all in one phase (100 rows)                 0.240    0.018      0.206
    fp32 matrix cores                           0.998    0.055      0.542
    forward only (ll), all three kinds          --       --         0.208

(0.3 of 8 u is 2.4 u: the kernels add the small terms first, and only the last
three adds round at the size of the product.  0.998 of u is round-to-nearest
at a product just above a power of two.)

The constants' e32 (torch-CPU fp32 against fp64 at pre = 0, t = 0), measured:
negative binomial p 0, log_r 2.7e-9; zero-inflated negative binomial pi 3.0e-8,
p 3.0e-8, log_r 2.7e-9.
"""
import ctypes
import os

import numpy as np
import pytest

import _head_probes as hp
import test_gpu_head_packed as packed

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
SENTINEL = packed.SENTINEL
POISSON, NB, ZINB = hp.NAMES
ARITH = {"fp32": 0, "bf16x9": 1, "bf16x6": 2}

# (kind, H): (steps, producer waves, strip (0: the head count's default), DBP,
# PACK) of the producer / consumer kernel at 200 rows
PC = {
    (POISSON, 20): (1, 4, 0, False, False), (POISSON, 39): (2, 4, 0, False, True),
    (POISSON, 40): (2, 4, 0, False, False), (POISSON, 64): (3, 4, 0, False, True),
    (POISSON, 100): (4, 4, 0, False, True), (POISSON, 104): (4, 4, 0, False, False),
    (POISSON, 127): (4, 4, 0, False, False), (POISSON, 128): (5, 4, 0, True, False),
    (POISSON, 130): (5, 4, 0, False, False), (POISSON, 255): (8, 4, 0, False, False),
    (POISSON, 256): (9, 4, 0, True, False),
    (NB, 39): (2, 8, 0, False, True), (NB, 100): (4, 8, 0, False, True),
    (NB, 110): (4, 8, 0, False, False), (NB, 111): (4, 8, 0, False, False),
    # (the weight planes of 64 genes fit LDS as long as H + 1 <= 112)
    (NB, 112): (4, 4, 32, False, False),
    (NB, 128): (5, 4, 32, True, False), (NB, 200): (7, 4, 32, False, False),
    (NB, 256): (9, 4, 32, True, False),
    (ZINB, 39): (2, 4, 0, False, True), (ZINB, 100): (4, 4, 0, False, True),
    (ZINB, 128): (5, 4, 0, True, False), (ZINB, 130): (5, 4, 0, False, False),
    (ZINB, 159): (5, 4, 0, False, False),
    # (the six-term cases' one width beside those)
    (NB, 20): (1, 8, 0, False, False), (ZINB, 20): (1, 4, 0, False, False),
    # (and the one width of the 100-row cases that only this kernel takes)
    (NB, 126): (4, 4, 32, False, False),
}
PC_CASES = [k for k in PC if k not in ((NB, 20), (ZINB, 20), (NB, 126))]

RATIOS = {}          # family -> worst |error| / bound seen in this process (printed)


def _genes(name, H):
    F = hp.HEADS[name] * H + 5
    return F + 3 if F % 32 == 0 else F


def _kernel(name, H, rows, arith, u16=False):
    """(which, name) of the training kernel the library launches."""
    from scvae_amd import _lib
    lib = _lib.load()
    kind = _lib.LIKELIHOOD_KINDS[name][0]
    buf = ctypes.create_string_buffer(160)
    _lib.check(lib.scvae_decoder_train_kernel_name(
        kind, H, rows, ARITH[arith], int(u16), buf, 160), "kernel name")
    return lib.scvae_decoder_train_kernel(kind, H, ARITH[arith]), buf.value.decode()


def _assert_head4(name, H, rows, arith="bf16x9", u16=False):
    """The producer / consumer instantiation of PC[(name, H)]; its strip."""
    from scvae_amd import _lib
    which, kernel = _kernel(name, H, rows, arith, u16)
    assert which == 3 and kernel.startswith("decoder_head4_kernel<"), kernel
    args = [a.strip() for a in kernel[kernel.index("<") + 1:-1].split(",")]
    steps, waves, strip, dbp, pack = PC[(name, H)]
    six = arith == "bf16x6"
    assert not six or (steps <= 4 and strip == 0 and not dbp), "no six-term instantiation"
    want = [str(_lib.LIKELIHOOD_KINDS[name][0]), str(steps), str(u16).lower(), str(waves),
            str(strip), str(dbp).lower(), args[6], "6" if six else "9", "false",
            str(pack).lower()]
    assert args == want, (kernel, want)
    return strip or (32 if hp.HEADS[name] == 3 else 64)


def _flags(arith, atomics=False):
    from scvae_amd import _lib
    return _lib.HEAD_ARITH_FLAGS[arith] | (_lib.HEADS_DD_ATOMICS if atomics else 0)


def _np(t):
    return t.detach().cpu().double().numpy()


def _where(c, probe, k, strip):
    """(row mod 32, h, h mod 32, f mod strip, head) of element k of a check."""
    out = c["out"]
    if out == "dW":
        h, f = np.unravel_index(k, c["exact"].shape)
        return (int(c["row"][h, f]) % 32, int(h), int(h) % 32, int(f) % strip, c["head"])
    if out == "dd":
        r, h = np.unravel_index(k, c["exact"].shape)
        return (int(r) % 32, int(h), int(h) % 32, int(c["gene"][r, h]) % strip,
                int(c["head"][r, h]))
    if out == "db":
        return (None, probe["H"], probe["H"] % 32, int(k) % strip, c["head"])
    if out == "dd_live":
        h = int(c["cols"][k])
        return (int(k) % 32, h, h % 32, int(probe["gene"][h]) % strip, int(c["head"][k]))
    if out == "dW_live":
        h = int(c["rows"][k])
        return (None, h, h % 32, int(c["cols"][k]) % strip, int(c["heads"][k]))
    return (int(k) % 32, int(probe["hr"][k]), int(probe["hr"][k]) % 32,
            int(probe["gene"][probe["hr"][k]]) % strip, int(c["head"][k]))


def _check(out, probe, family, strip, what):
    """Every check of the probe, its zeros and the sentinel; the worst
    |error| / bound goes to RATIOS[family]."""
    rows, F, H, P = probe["rows"], probe["F"], probe["H"], probe["P"]
    dd = _np(out["dd"])
    dW = [_np(w) for w in out["dW"]]
    for c in probe["checks"]:
        kind = c["out"]
        if kind == "dW":
            got = dW[c["head"]][:H]
        elif kind == "db":
            got = _np(out["db"][c["head"]])[:F]
        elif kind == "dd":
            got = dd[:rows]
        elif kind == "dd_live":
            got = dd[c["rows"], c["cols"]]
        elif kind == "dW_live":
            got = np.array([dW[j][h, f] for j, h, f in zip(c["heads"], c["rows"], c["cols"])])
        else:
            got = _np(out["ll"])[:rows]
        ratio = np.abs(got - c["exact"]) / c["bound"]
        k = int(np.argmax(ratio))
        worst = float(ratio.flat[k])
        name = family if kind not in ("db", "dW_live") else family + ", sums"
        if probe["probe"] == "gemm1":
            name = family + (", through GEMM1" if kind != "dW_live" else ", through GEMM1, sums")
        RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
        print("head probe: %-44s %-6s %s  worst |error| / bound %.3f" % (
            name, probe["probe"], kind, worst))
        assert worst <= 1.0, (
            what, probe["probe"], kind, "worst |error| / bound", worst,
            "(row mod 32, h, h mod 32, f mod strip, head)", _where(c, probe, k, strip),
            "got", float(got.flat[k]), "exact", float(c["exact"].flat[k]))
    if not probe.get("forward"):
        if "dd" in probe["zeros"]:
            assert (dd[:rows] == 0).all(), (what, "dd of a probe with W = 0")
        if "dW" in probe["zeros"]:
            assert all((w[:H] == 0).all() for w in dW), (what, "dW of a probe with d = 0")
        for h in probe.get("dead_cols", ()):
            assert all((w[h] == 0).all() for w in dW), (what, "dW of a dead column", int(h))
        assert (dd[rows:] == SENTINEL).all(), what
        for j in range(P):
            assert (dW[j][H:] == SENTINEL).all(), what
            assert bool((out["db"][j][F:] == SENTINEL).all()), what
    assert bool((out["ll"][rows:] == SENTINEL).all()), what


def _run(device, name, rows, H, arith, family, strip, probes=("gemm3", "gemm2", "gemm1"),
         atomics=False, targets="f32", seeds=SEEDS):
    F = _genes(name, H)
    build = {"gemm3": hp.gemm3_probe, "gemm2": hp.gemm2_probe, "gemm1": hp.gemm1_probe}
    for seed in seeds:
        for which in probes:
            probe = build[which](name, rows, H, F, seed, arith)
            out = packed._launch(device, probe, 1, _flags(arith, atomics), targets)
            _check(out, probe, family, strip, (name, H, arith, which, seed))


@pytest.mark.parametrize("name,H", PC_CASES, ids=lambda v: str(v).replace(" ", "-"))
def test_producer_consumer_kernel_nine_terms(cuda_device, name, H):
    """One to nine contraction steps; the packed block with 8, 1 and 5 live
    rows and the first unpacked width on either side; four and eight producer
    waves; 64- and 32-gene strips; DBP at 128 and 256."""
    strip = _assert_head4(name, H, 200)
    family = "producer / consumer, packed" if PC[(name, H)][4] else "producer / consumer"
    _run(cuda_device, name, 200, H, "bf16x9", family, strip)


@pytest.mark.parametrize("name", hp.NAMES)
@pytest.mark.parametrize("H", [20, 39, 100])
def test_producer_consumer_kernel_six_terms(cuda_device, H, name):
    """bf16x6 where it has an instantiation of its own; the packed block of
    39 and 100 still carries nine terms, the bound the six-term one."""
    strip = _assert_head4(name, H, 200, "bf16x6")
    _run(cuda_device, name, 200, H, "bf16x6", "producer / consumer, six terms", strip)


@pytest.mark.parametrize("name", hp.NAMES)
@pytest.mark.parametrize("H", [20, 39, 64, 100, 126])
def test_all_in_one_phase_kernel(cuda_device, H, name):
    """100 rows: ``d3_schedule`` picks decoder_head3_kernel -- except for two
    heads at H = 126, whose weight planes of 64 genes do not fit its LDS: the
    library then launches the producer / consumer kernel on 32-gene strips."""
    from scvae_amd import _lib
    if (name, H) == (NB, 126):
        strip = _assert_head4(name, H, 100)
        _run(cuda_device, name, 100, H, "bf16x9", "producer / consumer", strip)
        return
    which, kernel = _kernel(name, H, 100, "bf16x9")
    steps = ((H + 1 + 15) // 16 * 16 + 31) // 32
    assert which == 3 and kernel == "decoder_head3_kernel<%d, %d, false, true, false, 0>" % (
        _lib.LIKELIHOOD_KINDS[name][0], steps), kernel
    _run(cuda_device, name, 100, H, "bf16x9", "all in one phase",
         32 if hp.HEADS[name] == 3 else 64)


@pytest.mark.parametrize("name", hp.NAMES)
@pytest.mark.parametrize("H", [20, 64, 100, 126])
def test_fp32_kernels(cuda_device, H, name):
    """``HEADS_FP32``: one rounding per product, u."""
    which, kernel = _kernel(name, H, 200, "fp32")
    assert which in (1, 2) and kernel.startswith(
        "decoder_head2_kernel<" if which == 2 else "decoder_head_kernel<"), kernel
    _run(cuda_device, name, 200, H, "fp32", "fp32 matrix cores",
         32 if hp.HEADS[name] == 3 else 64)


@pytest.mark.parametrize("name,H", [(POISSON, 100), (POISSON, 127), (NB, 100), (NB, 127),
                                    (ZINB, 100), (ZINB, 159)],
                         ids=lambda v: str(v).replace(" ", "-"))
def test_forward_only(cuda_device, name, H):
    """``train = 0``: the GEMM1 probe through ll[r].  By ``decoder_forward_choice``:
    one and two heads at H = 100 take the forward instantiation of the
    all-in-one-phase kernel, three heads at H = 100 decoder_forward_kernel
    (fp32 matrix cores), and an odd width only the forward half of the
    producer / consumer kernel (127; 159 with three heads)."""
    from scvae_amd import _lib
    lib = _lib.load()
    kind = _lib.LIKELIHOOD_KINDS[name][0]
    assert "SCVAE_DECODER_FORWARD" not in os.environ
    assert lib.scvae_decoder_train_kernel(kind, H, 1) == 3
    assert (lib.scvae_decoder_fused_variant(kind, H) == 0) == (H % 2 == 1)
    F = _genes(name, H)
    for seed in SEEDS:
        probe = hp.gemm1_probe(name, 200, H, F, seed, "bf16x9", forward=True)
        out = packed._launch(cuda_device, probe, 0, _flags("bf16x9"))
        _check(out, probe, "forward only", 32 if hp.HEADS[name] == 3 else 64,
               (name, H, "forward", seed))


@pytest.mark.parametrize("name,H", [(POISSON, 100), (POISSON, 40), (NB, 100), (NB, 110),
                                    (ZINB, 100), (ZINB, 130)],
                         ids=lambda v: str(v).replace(" ", "-"))
def test_uint16_targets(cuda_device, name, H):
    """One packed and one unpacked width per head count."""
    strip = _assert_head4(name, H, 200, u16=True)
    _run(cuda_device, name, 200, H, "bf16x9", "producer / consumer, uint16 targets", strip,
         targets="u16")


@pytest.mark.parametrize("name", hp.NAMES)
@pytest.mark.parametrize("H", [100, 39])
def test_dd_through_atomics(cuda_device, H, name):
    """``HEADS_DD_ATOMICS``: the sum of one product and zeros is the same by
    either path."""
    strip = _assert_head4(name, H, 200)
    _run(cuda_device, name, 200, H, "bf16x9", "producer / consumer, dd atomics", strip,
         probes=("gemm2",), atomics=True)


def test_row_groups(cuda_device):
    """600 rows x 710 genes (12 strips): ``d4_row_groups`` cuts the rows into
    two groups by its own rule, as in ``test_gpu_head_packed.py``; the GEMM3
    probe with live rows in both -- the slab combine adds exact zeros to the
    single product."""
    strip = _assert_head4(NB, 100, 600)
    for seed in SEEDS:
        probe = hp.gemm3_probe(NB, 600, 100, 710, seed, two_groups=True)
        out = packed._launch(cuda_device, probe, 1, _flags("bf16x9"))
        assert not bool((packed._slab_words(out, probe) == 0x5A5A5A5A).any())
        _check(out, probe, "producer / consumer, row groups", strip, ("row groups", seed))
