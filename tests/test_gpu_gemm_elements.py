"""``scvae_gemm`` element by element against the fp64 oracle (tests/_gemm_oracle.py)
on every route of its dispatcher: the 64-tile kernel with all four transposes,
the 128-tile kernel, the narrow-N kernel, both split-K reducers and the unsplit
fallback with no workspace.  Every case first asserts its route through
``scvae_gemm_route``.  Kinds of case: integer-exact (bit for bit), one- and
two-product probes at every k a kernel treats differently, graded random
(K <= 48), operands inside NaN-filled padding at odd leading dimensions and
4-byte-aligned bases, non-finite inputs, and the refusals.

Observed max err / bound on an MI355X: see DESIGN.md ("GEMM element bounds").
"""
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


def _k_step(kernel):
    return {0: 16, 1: 32, 2: 16}[kernel]


def _stored(X_op, t):
    """op-space [M, K] (or [K, N]) -> the stored layout."""
    return np.ascontiguousarray(X_op.T) if t else X_op


def _probe_launches(lib, ta, tb, A0, B, Bh, M, N, K, route, rng, dev):
    """One-product probes at every position (as many launches as it takes), then one
    two-product launch.  A0: a Placed zero matrix in the stored layout, rewritten
    in place; B dense with full mantissas (Bh on the host, [K, N])."""
    kernel, splits, k_chunk, _ = route
    worst = 0.0
    if K == 0:
        return worst
    ks = go.probe_positions(K, k_chunk if splits > 1 else 0, _k_step(kernel))
    rounds = go.probe_rounds(ks, M, K, rng)
    rows = np.arange(M)
    for r, k1 in enumerate(rounds + [None]):
        two = k1 is None
        if two:
            k1 = rng.integers(0, K, M)
        v = go.full_mantissa(rng, (M, 2))
        k2 = go.second_positions(k1, K, k_chunk if splits > 1 else 0, _k_step(kernel), rng)
        if not two or K == 1:
            v[:, 1] = 0
        A0.view.zero_()
        for kk, vv in ((k1, v[:, 0]), (k2, v[:, 1])):
            i0 = torch.from_numpy(kk if ta else rows).to(dev)
            i1 = torch.from_numpy(rows if ta else kk).to(dev)
            A0.view.index_put_((i0, i1), torch.from_numpy(vv.copy()).to(dev),
                               accumulate=True)
        same = (k1 == k2) & (v[:, 1] != 0)           # (cannot happen for K > 1)
        assert not same.any()
        got = gl.run_gemm(lib, ta, tb, A0, B, None, M, N, K, want_route=route)
        ref, S, p = go.expect_sparse_rows(np.stack([k1, k2], 1), v, Bh)
        worst = max(worst, go.check_bound(got, ref, go.bound_fp32(S, p, True),
                                          "probe round {}".format(r)))
    return worst


def _mirrored_probe(lib, ta, tb, M, N, K, route, rng, dev):
    """B sparse by column (one non-zero per column), A dense."""
    kernel, splits, k_chunk, _ = route
    if K == 0:
        return 0.0
    ks = go.probe_positions(K, k_chunk if splits > 1 else 0, _k_step(kernel))
    kj = go.probe_rounds(ks, N, K, rng)[0]
    v = go.full_mantissa(rng, N)
    Bh = np.zeros((K, N), dtype=F32)
    Bh[kj, np.arange(N)] = v
    Ah = go.full_mantissa(rng, (M, K))
    got = gl.run_gemm(lib, ta, tb, gl.place(_stored(Ah, ta)), gl.place(_stored(Bh, tb)),
                      None, M, N, K, want_route=route)
    ref = Ah.astype(F64)[:, kj] * v.astype(F64)[None, :]
    return go.check_bound(got, ref, go.U * np.abs(ref), "mirrored probe")


def _integer_exact(lib, ta, tb, A, B, ref0, bias_h, M, N, K, route, dev, use_ws=True):
    """Null bias; bias + ReLU; bias + accumulate.  ref0 = op(A) op(B) exactly."""
    got = gl.run_gemm(lib, ta, tb, A, B, None, M, N, K, use_ws=use_ws, want_route=route)
    go.check_integer_exact(got, ref0)
    bias = gl.place(bias_h[None, :])
    got = gl.run_gemm(lib, ta, tb, A, B, bias, M, N, K, relu=True, use_ws=use_ws,
                      want_route=route)
    go.check_integer_exact(got, go.relu64(ref0 + bias_h.astype(F64)))
    c0 = np.full((M, N), 5.0, dtype=F32)
    got = gl.run_gemm(lib, ta, tb, A, B, bias, M, N, K, use_ws=use_ws,
                      c0=torch.from_numpy(c0).to(dev), want_route=route)
    go.check_integer_exact(got, ref0 + bias_h.astype(F64) + 5.0)


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape,route", go.GEMM_SMALL,
                         ids=["x".join(map(str, s)) for s, _ in go.GEMM_SMALL])
def test_tile64_elements(cuda_device, shape, route, ta, tb):
    """K = 0 is pinned as the empty sum: C = act(bias), C0 + act(bias) with
    accumulate."""
    lib = _lib_()
    dev = cuda_device
    M, N, K = shape
    rng = np.random.default_rng(M * 131 + N * 17 + K + 2 * ta + tb)
    ws = lib.scvae_gemm_workspace_bytes(M, N, K)
    assert gl.gemm_route(lib, ta, tb, M, N, K, K if tb else N, ws) == route
    # integer-exact
    Ah, Bh = go.small_integers(rng, (M, K)), go.small_integers(rng, (K, N))
    bias_h = go.small_integers(rng, N)
    ref0 = Ah.astype(F64) @ Bh.astype(F64)
    A, B = gl.place(_stored(Ah, ta)), gl.place(_stored(Bh, tb))
    _integer_exact(lib, ta, tb, A, B, ref0, bias_h, M, N, K, route, dev)
    if route[1] > 1:                 # the unsplit fallback with no workspace
        _integer_exact(lib, ta, tb, A, B, ref0, bias_h, M, N, K, (route[0], 1, K, 0), dev,
                       use_ws=False)
    # probes
    Bp = go.full_mantissa(rng, (K, N))
    A0 = gl.place(np.zeros_like(_stored(Ah, ta)))
    worst = {"probe": _probe_launches(lib, ta, tb, A0, gl.place(_stored(Bp, tb)), Bp, M, N, K,
                                      route, rng, dev),
             "mirrored": _mirrored_probe(lib, ta, tb, M, N, K, route, rng, dev), "graded": 0.0}
    # graded random
    if K <= 48:
        Ag, Bg = go.graded(rng, M, N, K)
        bg, c0 = go.full_mantissa(rng, N), go.full_mantissa(rng, (M, N), -20, 0)
        for use_bias, relu, acc in ((0, 0, 0), (1, 1, 0), (1, 0, 1)):
            got = gl.run_gemm(lib, ta, tb, gl.place(_stored(Ag, ta)), gl.place(_stored(Bg, tb)),
                              gl.place(bg[None, :]) if use_bias else None, M, N, K,
                              relu=bool(relu),
                              c0=torch.from_numpy(c0).to(dev) if acc else None,
                              want_route=route)
            ref, S, p = go.expect_dense(Ag, Bg, bg if use_bias else None,
                                        c0 if acc else None, bool(relu))
            worst["graded"] = max(worst["graded"], go.check_bound(
                got, ref, go.bound_fp32(S, np.full_like(S, K), False), "graded"))
    print("gemm", shape, "ta", ta, "tb", tb, "worst err/bound", worst)
    # padding and alignment: every operand inside NaN, C inside the pattern
    for extra, off in ((1, 1), (3, 3), (5, 1)):
        Ap = gl.place(_stored(Ah, ta), extra, off)
        Bq = gl.place(_stored(Bh, tb), extra, off)
        bp = gl.place(bias_h[None, :], 0, off)
        ldb = Bq.ld
        want = gl.gemm_route(lib, ta, tb, M, N, K, ldb, ws)
        assert want == route
        got = gl.run_gemm(lib, ta, tb, Ap, Bq, bp, M, N, K, c_extra=extra, c_off=off)
        go.check_integer_exact(got, ref0 + bias_h.astype(F64))


def _plant(A, ta, M, K):
    """NaN, +inf, -inf into three distinct rows of op(A), interior and last k.
    Returns the (row, k, value) list and a restore function."""
    spots = [(M // 3, K // 2, np.nan), (M // 2, K - 1, np.inf), (M - 1, K // 3, -np.inf)]
    saved = []
    for i, k, v in spots:
        idx = (k, i) if ta else (i, k)
        saved.append((idx, float(A.view[idx])))
        A.view[idx] = float(v)

    def restore():
        for idx, v in saved:
            A.view[idx] = v
    return spots, restore


def _non_finite(lib, ta, tb, A, B, Ah_op, Bh_op, ref0, M, N, K, route, use_ws):
    """Ah_op, Bh_op: the finite operands on the host; ref0 their exact product."""
    spots, restore = _plant(A, ta, M, K)
    rows = [i for i, _, _ in spots]
    Ar = Ah_op[rows].copy()
    for n, (_, k, v) in enumerate(spots):
        Ar[n, k] = v
    pre = ref0.copy()
    pre[rows] = go.row_sums_fp64(Ar, Bh_op, range(len(rows)))
    try:
        for relu in (False, True):
            got = gl.run_gemm(lib, ta, tb, A, B, None, M, N, K, relu=relu, use_ws=use_ws,
                              want_route=route)
            ref = go.relu64(pre) if relu else pre
            go.check_classes(got, ref)
            keep = np.ones(M, dtype=bool)
            keep[rows] = False
            go.check_integer_exact(got[keep], ref[keep])
    finally:
        restore()


def test_tile64_non_finite(cuda_device):
    lib = _lib_()
    for shape, route in (go.GEMM_SMALL[6], go.GEMM_SMALL[8]):     # unsplit, wide reducer
        M, N, K = shape
        for ta, tb in ((0, 0), (1, 1)):
            rng = np.random.default_rng(K + ta)
            Ah, Bh = go.small_integers(rng, (M, K)), go.small_integers(rng, (K, N))
            _non_finite(lib, ta, tb, gl.place(_stored(Ah, ta)), gl.place(_stored(Bh, tb)),
                        Ah, Bh, Ah.astype(F64) @ Bh.astype(F64), M, N, K, route, True)


# ---- the big routes: operands of 3 to 60 M elements, built once per module ----
@pytest.fixture(scope="module")
def big_operands(cuda_device):
    cache = {}

    def get(shape):
        if shape not in cache:
            M, N, K = shape
            rng = np.random.default_rng(M + N + K)
            Ah, Bh = go.small_integers(rng, (M, K)), go.small_integers(rng, (K, N))
            At = torch.from_numpy(Ah).to(cuda_device)
            cache[shape] = dict(
                Ah=Ah, Bh=Bh, ref0=Ah.astype(F64) @ Bh.astype(F64),
                bias=go.small_integers(rng, N),
                A={0: gl.place(At), 1: gl.place(At.T.contiguous())},
                B=gl.place(Bh), Bp_h=None)
        return cache[shape]
    yield get
    cache.clear()


def _big_case(lib, dev, ops, shape, route, ta, probes=True):
    M, N, K = shape
    A, B = ops["A"][ta], ops["B"]
    rng = np.random.default_rng(K + ta)
    unsplit = (route[0], 1, K, 0)
    _integer_exact(lib, ta, 0, A, B, ops["ref0"], ops["bias"], M, N, K, route, dev)
    if route[1] > 1:
        got = gl.run_gemm(lib, ta, 0, A, B, None, M, N, K, use_ws=False, want_route=unsplit)
        go.check_integer_exact(got, ops["ref0"])
    _non_finite(lib, ta, 0, A, B, ops["Ah"], ops["Bh"], ops["ref0"], M, N, K, route, True)
    if route[1] > 1:
        _non_finite(lib, ta, 0, A, B, ops["Ah"], ops["Bh"], ops["ref0"], M, N, K, unsplit,
                    False)
    # probes: the A upload is rewritten in place and restored
    if ops["Bp_h"] is None:
        ops["Bp_h"] = go.full_mantissa(np.random.default_rng(N), (K, N))
        ops["Bp"] = gl.place(ops["Bp_h"])
    keep = A.view.clone()
    try:
        worst = _probe_launches(lib, ta, 0, A, ops["Bp"], ops["Bp_h"], M, N, K, route, rng,
                                dev)
    finally:
        A.view.copy_(keep)
    print("gemm", shape, "ta", ta, "probe worst err/bound", worst)


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("shape,route", go.GEMM_BIG,
                         ids=["x".join(map(str, s)) for s, _ in go.GEMM_BIG])
def test_tile128_elements(cuda_device, big_operands, shape, route, ta):
    lib = _lib_()
    ops = big_operands(shape)
    _big_case(lib, cuda_device, ops, shape, route, ta)
    # padding and alignment
    M, N, K = shape
    Ah_st = _stored(ops["Ah"], ta)
    for extra, off in ((1, 1), (3, 3)):
        got = gl.run_gemm(lib, ta, 0, gl.place(Ah_st, extra, off),
                          gl.place(ops["Bh"], extra, off), gl.place(ops["bias"][None, :], 0, off),
                          M, N, K, c_extra=extra, c_off=off, want_route=route)
        go.check_integer_exact(got, ops["ref0"] + ops["bias"].astype(F64))


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("shape,route", go.GEMM_NARROW,
                         ids=["x".join(map(str, s)) for s, _ in go.GEMM_NARROW])
def test_narrow_elements(cuda_device, big_operands, shape, route, ta):
    lib = _lib_()
    ops = big_operands(shape)
    M, N, K = shape
    assert M * N * K >= 4e9 and K % 16 in (0, 1, 15) and 1 <= N % 32 <= 8
    _big_case(lib, cuda_device, ops, shape, route, ta)
    # ldb = N + 3 (and the base 12 bytes off): still the narrow route; A padded too
    Bq = gl.place(ops["Bh"], 3, 3)
    Ap = gl.place(_stored(ops["Ah"], ta), 1, 1)
    got = gl.run_gemm(lib, ta, 0, Ap, Bq, gl.place(ops["bias"][None, :], 0, 1), M, N, K,
                      c_extra=5, c_off=3, want_route=route)
    go.check_integer_exact(got, ops["ref0"] + ops["bias"].astype(F64))
    got = gl.run_gemm(lib, ta, 0, Ap, Bq, None, M, N, K, use_ws=False, c_extra=1, c_off=1,
                      want_route=(2, 1, K, 0))
    go.check_integer_exact(got, ops["ref0"])


# ---- refusals: nothing is launched, C stays as it was ----
def _refusal_args():
    big = 2 ** 32
    base = dict(M=5, N=6, K=7, lda=7, ldb=6, ldc=6)
    cases = []
    for name in base:
        cases.append((name, base[name] + big))      # casts down to the base value
        cases.append((name, -1))
        cases.append((name, 2 ** 31))
    cases += [("lda", 6), ("ldb", 5), ("ldc", 5)]
    return base, cases


def test_gemm_refusals(cuda_device):
    lib = _lib_()
    base, cases = _refusal_args()
    dev = cuda_device
    A = gl.place(np.ones((8, 8), dtype=F32))
    B = gl.place(np.ones((8, 8), dtype=F32))
    for ta, tb in ((0, 0), (1, 1)):
        for name, value in cases:
            a = dict(base)
            if ta:
                a["lda"] = 5
            if tb:
                a["ldb"] = 7
            if name in ("lda", "ldb", "ldc") and value < 8 and value >= 0:
                value = a[name] - 1                   # one below the extent
            a[name] = value
            out = gl.Out(8, 8, dev)
            rc = lib.scvae_gemm(ta, tb, A.ptr, B.ptr, None, out.ptr, a["M"], a["N"], a["K"],
                                a["lda"], a["ldb"], a["ldc"], 0, 0, None, 0, gl.stream())
            assert rc == -1, (ta, tb, name, value)
            assert out.untouched(), (ta, tb, name, value)
