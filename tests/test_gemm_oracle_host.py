"""The GEMM oracle (tests/_gemm_oracle.py) on the CPU: every checker accepts the
faithful NumPy emulation of its arithmetic and rejects each listed defect; the
old matrix-wide criterion accepts a defect the element checkers reject; and the
case tables of the GPU tests reach every route the dispatchers can produce (the
route queries are host code: nothing is launched)."""
import ctypes

import numpy as np
import pytest

import _gemm_oracle as go

F32, F64 = np.float32, np.float64
M, N, K, KC = 9, 7, 40, 16          # three slabs of the emulated split-K


# ------------------------------------------------------------ fp32 GEMM
def _int_case(ta=False, tb=False, bias=True, relu=False, seed=0):
    rng = np.random.default_rng(seed)
    A = go.small_integers(rng, (K, M) if ta else (M, K))
    B = go.small_integers(rng, (N, K) if tb else (K, N))
    b = go.small_integers(rng, N) if bias else None
    if b is not None:
        b[1] = -b[0]                 # (neighbouring columns differ)
    ref, _, _ = go.expect_dense(go.op(A, ta), go.op(B, tb), b, None, relu)
    return A, B, b, ref


def _probe_case(seed=1):
    rng = np.random.default_rng(seed)
    k1 = rng.permutation(go.probe_positions(K, KC, 16))[:M]
    k2 = go.second_positions(k1, K, KC, 16, rng)
    v = go.full_mantissa(rng, (M, 2))
    v[::2, 1] = 0                    # even rows: a single product
    A = np.zeros((M, K), dtype=F32)
    A[np.arange(M), k1] = v[:, 0]
    A[np.arange(M), k2] += v[:, 1]
    B = go.full_mantissa(rng, (K, N))
    ref, S, p = go.expect_sparse_rows(np.stack([k1, k2], 1), v, B)
    return A, B, ref, go.bound_fp32(S, p, True)


def _nan_case(relu):
    rng = np.random.default_rng(2)
    A, B = go.full_mantissa(rng, (M, K)), go.full_mantissa(rng, (K, N))
    A[1, 5], A[3, K - 1], A[6, 17] = np.nan, np.inf, -np.inf
    ref = go.row_sums_fp64(A, B, range(M))
    return A, B, go.relu64(ref) if relu else ref


def test_fp32_checkers_accept_the_faithful_emulation():
    for ta, tb in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for relu in (False, True):
            A, B, b, ref = _int_case(ta, tb, True, relu)
            go.check_integer_exact(
                go.emulate_fp32_gemm(A, B, b, None, relu, ta, tb, KC), ref)
    A, B, ref, bound = _probe_case()
    assert go.check_bound(go.emulate_fp32_gemm(A, B, k_chunk=KC), ref, bound) <= 1.0
    rng = np.random.default_rng(3)
    A, B = go.graded(rng, M, N, K)
    b, c0 = go.full_mantissa(rng, N), go.full_mantissa(rng, (M, N))
    ref, S, p = go.expect_dense(A, B, b, c0)
    go.check_bound(go.emulate_fp32_gemm(A, B, b, c0, k_chunk=KC), ref,
                   go.bound_fp32(S, p, False))
    for relu in (False, True):
        A, B, ref = _nan_case(relu)
        go.check_classes(go.emulate_fp32_gemm(A, B, relu=relu, k_chunk=KC), ref)


@pytest.mark.parametrize("defect", go.FP32_DEFECTS)
def test_fp32_checkers_reject(defect):
    if defect in ("bf16_operand", "mant10_operand"):
        A, B, ref, bound = _probe_case()
        with pytest.raises(AssertionError):
            go.check_bound(go.emulate_fp32_gemm(A, B, k_chunk=KC, defect=defect),
                           ref, bound)
        return
    if defect == "nan_to_zero":
        for relu in (False, True):
            A, B, ref = _nan_case(relu)
            with pytest.raises(AssertionError):
                go.check_classes(go.emulate_fp32_gemm(
                    A, B, relu=relu, k_chunk=KC, defect=defect), ref)
        return
    ta = defect == "ignore_ta"
    tb = defect == "ignore_tb"
    relu = defect == "relu_before_sum"
    A, B, b, ref = _int_case(ta, tb, True, relu)
    at = (2, 3, 21)
    if defect == "swap":             # two outputs of different value
        j = int(np.argmax(ref[2, :-1] != ref[2, 1:]))
        assert ref[2, j] != ref[2, j + 1]
        at = (2, j, 0)
    got = go.emulate_fp32_gemm(A, B, b, None, relu, ta, tb, KC, defect, at)
    with pytest.raises(AssertionError):
        go.check_integer_exact(got, ref)


# ----------------------------------------------------------- count GEMM
KM = 32                              # k_main of the emulated count product: 8 leftover k


def _count_int_case(relu=False, seed=4):
    rng = np.random.default_rng(seed)
    x = (rng.integers(1, 700, (M, K)) * (rng.random((M, K)) < 0.5)).astype(F32)
    w = go.small_integers(rng, (K, N))
    b = go.small_integers(rng, N)
    b[1] = -b[0]
    ref, _, _ = go.expect_dense(x, w, b, None, relu)
    return x, w, b, ref


def _count_probe_case(exact=False, seed=5):
    rng = np.random.default_rng(seed)
    k1 = rng.permutation(K)[:M]
    k2 = go.second_positions(k1, K, KC, 32, rng)
    c = np.array(go.PROBE_COUNTS)[np.arange(2 * M) % len(go.PROBE_COUNTS)].reshape(M, 2)
    if exact:
        c = np.array([1, 3, 127, 256, 257, 513, 32768, 65535, 100]).reshape(M, 1)
        k2 = None
    else:
        c[::2, 1] = 0
    x = np.zeros((M, K), dtype=F32)
    x[np.arange(M), k1] = c[:, 0]
    if k2 is not None:
        x[np.arange(M), k2] = c[:, 1]
    if exact:
        w = np.zeros((K, N), dtype=F32)
        w[k1] = go.exact_weights(rng, np.repeat(c, N, 1))
        ks = k1[:, None]
    else:
        w = go.three_piece_weights(rng, (K, N))
        ks = np.stack([k1, k2], 1)
    ref, S, p = go.expect_sparse_rows(ks, c, w)
    return x, w, ref, go.bound_count(S, p)


def test_count_checkers_accept_the_faithful_emulation():
    for relu in (False, True):
        x, w, b, ref = _count_int_case(relu)
        go.check_integer_exact(go.emulate_count_gemm(x, w, b, relu, KM, KC), ref)
    x, w, ref, bound = _count_probe_case()
    go.check_bound(go.emulate_count_gemm(x, w, None, False, KM, KC), ref, bound)
    x, w, ref, _ = _count_probe_case(exact=True)
    go.check_bit_equal(go.emulate_count_gemm(x, w, None, False, KM, KC), ref)
    # a non-finite weight: its whole column is non-finite (0 * NaN = NaN, and the
    # split of an infinity is NaN), with and without ReLU
    x, w, b, _ = _count_int_case()
    spots = [(5, 1, np.nan), (K - 1, 3, np.inf), (17, 4, -np.inf), (K - 2, 5, -np.inf)]
    for k, j, v in spots:            # (k >= KM: the unsplit leftover terms)
        w[k, j] = v
    pre = go.nonfinite_pre(x, spots, N)
    wf = np.where(np.isfinite(w), w, 0).astype(F32)
    for relu in (False, True):
        ref, S, p = go.expect_dense(x, wf, b, None, relu)
        go.check_nonfinite_kept(go.emulate_count_gemm(x, w, b, relu, KM, KC),
                                pre, relu, ref, go.bound_count(S, p))


@pytest.mark.parametrize("defect", go.COUNT_DEFECTS)
def test_count_checkers_reject(defect):
    if defect in ("drop_w2", "drop_w3", "drop_lo", "drop_lo_w2"):
        x, w, ref, bound = _count_probe_case()
        with pytest.raises(AssertionError):
            go.check_bound(go.emulate_count_gemm(x, w, None, False, KM, KC, defect),
                           ref, bound)
        if defect != "drop_w3":      # (a 17-bit weight has no third piece)
            x, w, ref, _ = _count_probe_case(exact=True)
            with pytest.raises(AssertionError):
                go.check_bit_equal(
                    go.emulate_count_gemm(x, w, None, False, KM, KC, defect), ref)
        return
    if defect == "nan_to_zero":
        x, w, b, _ = _count_int_case()
        w[5, 1] = np.nan
        pre = go.nonfinite_pre(x, [(5, 1, np.nan)], N)
        ref, S, p = go.expect_dense(x, np.where(np.isfinite(w), w, 0).astype(F32), b,
                                    None, True)
        with pytest.raises(AssertionError):
            go.check_nonfinite_kept(
                go.emulate_count_gemm(x, w, b, True, KM, KC, defect), pre, True, ref,
                go.bound_count(S, p))
        return
    relu = defect == "relu_before_sum"
    x, w, b, ref = _count_int_case(relu)
    i0, k0 = 2, int(np.argmax(x[2] != 0))
    at = (i0, 3, k0)
    if defect == "swap":
        j = int(np.argmax(ref[2, :-1] != ref[2, 1:]))
        at = (2, j, 0)
    got = go.emulate_count_gemm(x, w, b, relu, KM, KC, defect, at)
    with pytest.raises(AssertionError):
        go.check_integer_exact(got, ref)


def test_old_criterion_accepts_a_lost_product_and_the_element_bound_rejects_it():
    """The gap: test_count_gemm_matches_fp32_mfma_and_fp64's criterion -- relative
    to the output's largest magnitude, at its shape (37, 203, 24) and with its
    operands -- passes a result in which a small element lost a whole product;
    the per-element bound on the same operands does not."""
    rows, cols, n = 37, 203, 24
    rng = np.random.default_rng(rows * 7 + cols + n)
    x = rng.poisson(3.0, size=(rows, cols)) * (rng.random((rows, cols)) < 0.3)
    x = x.astype(F32)
    k = max(1, rows * cols // 500)
    x.flat[rng.integers(0, x.size, k)] = rng.integers(256, 65536, k).astype(F32)
    x.flat[0], x.flat[-1] = 65535.0, 257.0
    w = (rng.standard_normal((cols, n)) * np.exp(rng.uniform(-12, 1, (cols, n)))
         ).astype(F32)
    b = None                          # (mode 1 of the old test: no bias)
    ref, S, p = go.expect_dense(x, w)
    ref32 = go.emulate_fp32_gemm(x, w, b)
    scale = np.abs(ref).max()
    # the product to lose: below a quarter of the old limit, as far beyond its
    # element's bound as any
    prods = np.abs(x.astype(F64)[:, :, None] * w.astype(F64)[None, :, :])   # [i, k, j]
    ratio = np.where(prods <= 0.25e-6 * scale, prods, 0) / go.bound_count(S, p)[:, None, :]
    i0, k0, j0 = (int(v) for v in np.unravel_index(np.argmax(ratio), ratio.shape))
    assert ratio[i0, k0, j0] > 4

    def old_criterion(got):
        ok = np.isfinite(got).all()
        ok &= np.abs(got - ref32).max() <= 1e-6 * scale
        err_split = np.abs(got - ref).max() / scale
        err_fp32 = np.abs(ref32 - ref).max() / scale
        return ok and err_split <= max(4.0 * err_fp32, 5e-7)

    good = go.emulate_count_gemm(x, w, b, False, 192, 192)
    bad = go.emulate_count_gemm(x, w, b, False, 192, 192, "drop_product", (i0, j0, k0))
    assert not np.array_equal(good, bad)
    assert old_criterion(good) and old_criterion(bad)
    go.check_bound(good, ref, go.bound_count(S, p))
    with pytest.raises(AssertionError):
        go.check_bound(bad, ref, go.bound_count(S, p))


# ------------------------------------------------- routes of the case tables
def _gemm_route(lib, ta, tb, shape, ldb, ws):
    out = (ctypes.c_int32 * 4)()
    assert lib.scvae_gemm_route(ta, tb, *shape, ldb, ws, out) == 0
    return tuple(out)


def _count_route(lib, mode, rows, cols, n, u16, indexed):
    out = (ctypes.c_int32 * 8)()
    assert lib.scvae_count_gemm_route(mode, rows, cols, n, u16, indexed, out) == 0
    assert out[7] == 0
    return tuple(out)[:7]


def test_case_tables_reach_every_route():
    from scvae_amd import _lib
    lib = _lib.load()
    kernels, reducers, unsplit_fallback = set(), set(), set()
    for table in (go.GEMM_SMALL, go.GEMM_BIG, go.GEMM_NARROW):
        for shape, want in table:
            ws = lib.scvae_gemm_workspace_bytes(*shape)
            assert _gemm_route(lib, 0, 0, shape, shape[1], ws) == want, shape
            assert _gemm_route(lib, 1, 0, shape, shape[1], ws) == want, shape
            kernels.add(want[0])
            reducers.add(want[3])
            if want[1] > 1:          # the same shape with no workspace: unsplit
                assert _gemm_route(lib, 0, 0, shape, shape[1], 0) == (
                    want[0], 1, shape[2], 0)
                unsplit_fallback.add(want[0])
    for shape, want in go.GEMM_NARROW:   # ldb = N is still the narrow route
        assert _gemm_route(lib, 0, 0, shape, shape[1] + 3, 0)[0] == 2
    # tb = 1 never leaves the 64-tile kernel
    assert _gemm_route(lib, 0, 1, go.GEMM_BIG[0][0], go.GEMM_BIG[0][0][2], 0)[0] == 0
    assert kernels == {0, 1, 2} and reducers == {0, 1, 2}
    assert unsplit_fallback == {0, 1, 2}

    seen = {"direct": set(), "NQ": set(), "NT": set(), "pair": set(), "waves": set(),
            "k_main0": set(), "split": set(), "leftover": set()}
    for (case, want) in go.COUNT_CASES + [go.COUNT_WAVES8]:
        mode, rows, cols, n = case[:4]
        assert _count_route(lib, mode, rows, cols, n, 1, 0) == want, case
        assert _count_route(lib, mode, rows, cols, n, 1, 1) == want, case
        assert _count_route(lib, mode, rows, cols, n, 0, 0) == go.count_route_f32(
            want, mode), case
        kk = cols if mode == 0 else rows
        seen["k_main0"].add((mode, want[0] == 0))
        if want[0]:
            seen["direct"].add(want[3])
            seen["NQ" if mode == 0 else "NT"].add(want[4])
            seen["split"].add((mode, want[1] > 1))
            seen["leftover"].add((mode, want[0] < kk))
            if mode == 1:
                seen["pair"].add(want[5])
                seen["waves"].add(want[6])
                seen["waves"].add(go.count_route_f32(want, mode)[6])
    assert seen["direct"] == {0, 1}
    assert seen["NQ"] == {1, 2} and seen["NT"] == {1, 2, 3, 4}
    assert seen["pair"] == {0, 1} and seen["waves"] == {4, 8}
    for key in ("k_main0", "split", "leftover"):
        assert seen[key] == {(0, False), (0, True), (1, False), (1, True)}, key
    # the values the issue lists all appear
    m0 = [c for c, _ in go.COUNT_CASES if c[0] == 0]
    m1 = [c for c, _ in go.COUNT_CASES if c[0] == 1]
    assert {c[3] for c in m0} == {1, 31, 32, 33, 64, 65, 96, 97, 128}
    assert {c[1] for c in m0} == {1, 255, 256, 257, 700}
    assert {c[2] for c in m0} == {31, 32, 33, 64, 95, 256, 257, 1024, 1039}
    assert {c[3] for c in m1} == {1, 32, 33, 64, 65, 96, 97, 128}
    assert {c[2] for c in m1} == {1, 63, 64, 255, 256, 257, 512, 1025}
    assert {c[1] for c in m1} == {15, 16, 17, 31, 48, 512, 527}
    for kind in ("direct", "reduced", "reducer-only"):
        assert any(c[4] == "br" and (
            (kind == "direct" and w[3] == 1) or
            (kind == "reduced" and w[0] > 0 and w[3] == 0) or
            (kind == "reducer-only" and w[0] == 0)) for c, w in go.COUNT_CASES
            if c[0] == 0), kind


def test_route_queries_refuse_what_the_entries_refuse():
    from scvae_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 8)()
    big = 2 ** 31
    assert lib.scvae_gemm_route(0, 0, big, 1, 1, 1, 0, out) == -1
    assert lib.scvae_gemm_route(0, 0, 1, -1, 1, 1, 0, out) == -1
    assert lib.scvae_count_gemm_route(2, 1, 1, 1, 1, 0, out) == -1
    assert lib.scvae_count_gemm_route(0, 1, 1, 129, 1, 0, out) == -1
    assert lib.scvae_count_gemm_route(0, big, 1, 1, 1, 0, out) == -1
