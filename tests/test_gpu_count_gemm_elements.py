"""The two count products element by element against the fp64 oracle
(tests/_gemm_oracle.py), through all three entries on the same values --
``scvae_count_gemm`` (fp32 x), ``scvae_count_gemm_u16`` and
``scvae_count_gemm_u16_rows`` (x a taller resident matrix read through a
non-monotone row index with one repeat) -- which must agree bit for bit.  Every
case first asserts its route through ``scvae_count_gemm_route``.

Kinds of case: integer-exact, one- and two-product probes with the counts of
``PROBE_COUNTS`` against weights whose three bf16 pieces are all large, the
exact sub-case (every product fits 24 bits: bit-equal to x * w), operands inside
padding at odd pitches and 4-byte-aligned bases, non-finite `other`.

A non-finite `other[k, j]` reaches the whole column j: the split of an infinity
is NaN by construction (w2 = inf - inf) and 0 * NaN = NaN; only where an
infinity meets the plain fp32 leftover terms (k >= k_main) does it stay an
infinity, and ReLU(-inf) = 0 (`check_nonfinite_kept`).
"""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_launch as gl
import _gemm_oracle as go

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _lib_():
    from scvae_amd import _lib
    gl.assert_default_routes()
    return _lib.load()


class _X:
    """The same counts for the three entries.  x: [rows, cols] fp32 integers with
    x[rows - 1] == x[0] (the index repeats a resident row)."""

    def __init__(self, x, rng, pad=0):
        rows, cols = x.shape
        assert rows == 1 or np.array_equal(x[-1], x[0])
        self.rows, self.cols = rows, cols
        e32 = (1, 3, 5)[pad % 3] if pad else 0
        e16 = (cols & 1) + ((2, 6)[pad % 2] if pad else 0)
        self.f32 = gl.place(x, e32, (1, 3)[pad % 2] if pad else 0)
        self.u16 = gl.place_u16(x, e16, 2 if pad else 0)
        # resident matrix: three more rows than the minibatch, unused rows hold 65535
        res_rows = rows + 3
        idx = rng.permutation(res_rows)[:rows]
        if rows > 1:
            idx[-1] = idx[0]
        res = np.full((res_rows, cols), 65535.0, dtype=F32)
        res[idx] = x
        self.res = gl.place_u16(res, e16, 2 if pad else 0)
        self.idx = torch.from_numpy(idx.astype(np.int64)).to("cuda:0")

    def run(self, lib, mode, other, N, bias=None, relu=False, c_extra=0, c_off=0):
        """All three entries; asserts bit-identity; returns the result."""
        outs = []
        for entry, x in (("f32", self.f32), ("u16", self.u16), ("rows", self.res)):
            outs.append(gl.run_count(lib, entry, mode, x, self.rows, self.cols, other, N,
                                     bias, relu, c_extra, c_off,
                                     self.idx if entry == "rows" else None))
        for o, name in zip(outs[1:], ("u16", "rows")):
            same = (outs[0].view(np.uint32) == o.view(np.uint32)) | (
                np.isnan(outs[0]) & np.isnan(o))
            assert same.all(), "{} differs from fp32 x at {}".format(
                name, np.argwhere(~same)[:4].tolist())
        return outs[0]


def _assert_routes(lib, case, want):
    mode, rows, cols, N = case[:4]
    assert gl.count_route(lib, mode, rows, cols, N, 1, 0) == want
    assert gl.count_route(lib, mode, rows, cols, N, 1, 1) == want
    assert gl.count_route(lib, mode, rows, cols, N, 0, 0) == go.count_route_f32(want, mode)


def _to_x(X_op, mode):
    """op-space [M, K] counts -> x [rows, cols] with the repeat row enforced."""
    x = np.ascontiguousarray(X_op if mode == 0 else X_op.T).astype(F32)
    if x.shape[0] > 1:
        x[-1] = x[0]
    return x


def _op(x, mode):
    return x if mode == 0 else x.T


def _epilogue(case, rng, N):
    ep = case[4]
    bias = go.small_integers(rng, N) if "b" in ep else None
    return bias, "r" in ep


def _integer_exact(lib, case, rng, density=0.3, pad=0):
    mode, rows, cols, N = case[:4]
    M, K = (rows, cols) if mode == 0 else (cols, rows)
    x = _to_x((rng.integers(1, 700, (M, K)) * (rng.random((M, K)) < density)), mode)
    w = go.small_integers(rng, (K, N))
    bias, relu = _epilogue(case, rng, N)
    ref, S, _ = go.expect_dense(_op(x, mode), w, bias, None, relu, want_p=False)
    assert S.max() < 2 ** 24
    extra, off = ((1, 1), (3, 3), (5, 1))[pad % 3] if pad else (0, 0)
    got = _X(x, rng, pad).run(
        lib, mode, gl.place(w, extra, off), N,
        gl.place(bias[None, :], 0, off) if bias is not None else None, relu,
        c_extra=extra if pad else (1 if mode == 0 else 0), c_off=off)
    go.check_integer_exact(got, ref)


def _probes(lib, case, route, rng):
    """Bound probes at every position (one count per contraction, then two), and the
    exact sub-case."""
    mode, rows, cols, N = case[:4]
    M, K = (rows, cols) if mode == 0 else (cols, rows)
    k_main, splits, k_chunk = route[:3]
    bk = 32 if mode == 0 else 16
    bias, relu = _epilogue(case, rng, N)
    w = go.three_piece_weights(rng, (K, N))
    other = gl.place(w)
    bias_p = gl.place(bias[None, :] * F32(2.0 ** -24)) if bias is not None else None
    bias_s = bias * F32(2.0 ** -24) if bias is not None else None
    ks = go.probe_positions(K, k_chunk if splits > 1 else 0, bk, k_main)
    rounds = go.probe_rounds(ks, M, K, rng)
    counts = np.array(go.PROBE_COUNTS)
    worst = 0.0
    for r, k1 in enumerate(rounds + [None]):
        two = k1 is None
        if two:
            k1 = rng.integers(0, K, M)
        X = np.zeros((M, K), dtype=F32)
        X[np.arange(M), k1] = counts[rng.integers(0, len(counts), M)]
        if two and K > 1:
            k2 = go.second_positions(k1, K, k_chunk if splits > 1 else 0, bk, rng)
            X[np.arange(M), k2] = counts[rng.integers(0, len(counts), M)]
        x = _to_x(X, mode)
        got = _X(x, rng).run(lib, mode, other, N, bias_p, relu)
        ref, S, p = go.expect_dense(_op(x, mode), w, bias_s, None, relu)
        worst = max(worst, go.check_bound(got, ref, go.bound_count(S, p),
                                          "probe round {}".format(r)))
    # exact sub-case: the count of a k decides how many bits its weights carry
    ck = np.array([1, 3, 127, 100, 256, 257, 513, 32768, 43691, 65535, 2, 96])[
        rng.integers(0, 12, K)]
    k1 = rng.permutation(np.arange(K))[np.arange(M) % K]
    if mode == 1 and K > 2:          # (cells 0 and K - 1 are the repeated row: left empty)
        k1 = 1 + rng.integers(0, K - 2, M)
    X = np.zeros((M, K), dtype=F32)
    X[np.arange(M), k1] = ck[k1]
    x = _to_x(X, mode)
    if mode == 0 or K > 2:
        we = go.exact_weights(rng, np.repeat(ck[:, None], N, 1))
        got = _X(x, rng).run(lib, mode, gl.place(we), N)
        ref, S, p = go.expect_dense(_op(x, mode), we)
        assert p.max() <= 1
        go.check_bit_equal(got, ref)
    return worst


def _non_finite(lib, case, rng):
    mode, rows, cols, N = case[:4]
    M, K = (rows, cols) if mode == 0 else (cols, rows)
    assert N >= 3 and K >= 3
    x = _to_x((rng.integers(1, 700, (M, K)) * (rng.random((M, K)) < 0.3)), mode)
    w = go.full_mantissa(rng, (K, N))
    bias = go.full_mantissa(rng, N)
    spots = [(K // 2, 0, np.nan), (K - 1, N // 2, np.inf), (K // 3, N - 1, -np.inf)]
    wf = w.copy()
    for k, j, v in spots:
        w[k, j], wf[k, j] = v, 0
    pre = go.nonfinite_pre(_op(x, mode), spots, N)
    X = _X(x, rng)
    for relu in ((False, True) if mode == 0 else (False,)):
        b = bias if mode == 0 else None
        got = X.run(lib, mode, gl.place(w), N,
                    gl.place(b[None, :]) if b is not None else None, relu)
        ref, S, p = go.expect_dense(_op(x, mode), wf, b, None, relu)
        go.check_nonfinite_kept(got, pre, relu, ref, go.bound_count(S, p))


_IDS = ["m{}_{}x{}x{}{}".format(*c) for c, _ in go.COUNT_CASES]
# padding and alignment on six cases spread over the routes; non-finite on one per route
_PADDED = {1: 1, 4: 2, 10: 3, 13: 4, 28: 5, 36: 6}
_NON_FINITE = (1, 4, 10, 13, 26, 27, 28, 35, 36)


@pytest.mark.parametrize("n", range(len(go.COUNT_CASES)), ids=_IDS)
def test_count_elements(cuda_device, n):
    lib = _lib_()
    case, route = go.COUNT_CASES[n]
    _assert_routes(lib, case, route)
    rng = np.random.default_rng(1000 + n)
    _integer_exact(lib, case, rng)
    worst = _probes(lib, case, route, rng)
    print("count", case, "probe worst err/bound", worst)
    if n in _PADDED:
        _integer_exact(lib, case, rng, pad=_PADDED[n])
    if n in _NON_FINITE:
        _non_finite(lib, case, rng)


def test_padded_and_non_finite_cases_cover_the_routes():
    """(host logic, but it reads the tables of this module)"""
    def kind(c, r):
        if r[0] == 0:
            return (c[0], "reducer-only")
        return (c[0], "direct" if r[3] else "split" if r[1] > 1 else "one-slab", r[5])
    all_kinds = {kind(c, r) for c, r in go.COUNT_CASES if c[3] >= 3}
    assert {kind(*go.COUNT_CASES[n]) for n in _NON_FINITE} == all_kinds
    assert len(_PADDED) == 6
    assert len({kind(*go.COUNT_CASES[n]) for n in _PADDED}) == 6


def test_count_dw_eight_waves(cuda_device):
    """genes = 2048, cells = 14336, N = 100: the 8-wave gene-pair weight gradient."""
    lib = _lib_()
    case, route = go.COUNT_WAVES8
    assert route[6] == 8 and route[5] == 1
    _assert_routes(lib, case, route)
    rng = np.random.default_rng(8)
    _integer_exact(lib, case, rng, density=0.05)
    mode, rows, cols, N = case[:4]
    # probes: two launches cover every position of the 14336 cells
    w = go.three_piece_weights(rng, (rows, N))
    other = gl.place(w)
    ks = go.probe_positions(rows, route[2], 16, route[0])
    counts = np.array(go.PROBE_COUNTS)
    for k1 in go.probe_rounds(ks, cols, rows, rng):
        X = np.zeros((cols, rows), dtype=F32)
        X[np.arange(cols), k1] = counts[rng.integers(0, len(counts), cols)]
        x = _to_x(X, mode)
        got = _X(x, rng).run(lib, mode, other, N)
        ref, S, p = go.expect_dense(_op(x, mode), w)
        print("count 8 waves probe worst err/bound",
              go.check_bound(got, ref, go.bound_count(S, p)))


# ---- refusals: nothing is launched, C stays as it was ----
def test_count_refusals(cuda_device):
    lib = _lib_()
    big = 2 ** 32
    base = dict(ldx=34, rows=5, cols=33, ld_other=6, N=6, ldc=6)
    cases = []
    for name in base:
        cases += [(name, base[name] + big), (name, -1), (name, 2 ** 31)]
    cases += [("ldx", 32), ("ld_other", 5), ("ldc", 5)]
    x32 = gl.place(np.ones((40, 40), dtype=F32))
    x16 = gl.place_u16(np.ones((40, 40), dtype=F32))
    other = gl.place(np.ones((40, 8), dtype=F32))
    idx = torch.arange(5, dtype=torch.int64, device=cuda_device)
    for mode in (0, 1):
        nbytes = lib.scvae_count_gemm_workspace_bytes(mode, 5, 33, 6)
        ws = gl.workspace(nbytes, cuda_device)
        for name, value in cases:
            a = dict(base)
            a[name] = value
            for entry, x in (("f32", x32), ("u16", x16), ("rows", x16)):
                out = gl.Out(40, 8, cuda_device)
                args = [mode, x.ptr, a["ldx"], a["rows"], a["cols"], other.ptr,
                        a["ld_other"], a["N"], None, 0, out.ptr, a["ldc"],
                        ctypes.c_void_p(ws.data_ptr()), nbytes]
                if entry == "rows":
                    args.append(ctypes.c_void_p(idx.data_ptr()))
                fn = {"f32": lib.scvae_count_gemm, "u16": lib.scvae_count_gemm_u16,
                      "rows": lib.scvae_count_gemm_u16_rows}[entry]
                assert fn(*args, gl.stream()) == -1, (mode, entry, name, value)
                assert out.untouched(), (mode, entry, name, value)
