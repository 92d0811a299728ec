"""fp64 oracle of the fp32 GEMM (``scvae_gemm``) and of the two count products
(``scvae_count_gemm*``), element by element: operand builders, expectations, one
checker per kind of case, the tables of cases the GPU tests run, and plain NumPy
emulations of the two arithmetics with switchable defects (for the host tests,
which show that every checker accepts the faithful arithmetic and rejects each
defect).

Bounds (u = 2^-24; derived, no number is taken from the kernels).  With
``S_ij = sum_k |a_ik b_kj| + |bias_j| (+ |C0_ij|)`` in fp64 and ``p_ij`` the number
of non-zero products of the element (adding an exact zero rounds nothing):

* fp32 GEMM: at most p + 2 roundings (the fused adds, bias, accumulate), so by
  the running-error bound ``|err| <= 1.01 (p + 2) u S``; a single product with no
  bias and no accumulate is one rounding of an exact product: ``|err| <= u |ab|``.
* count GEMM: six exact partial products per count summed in fp32, the slab
  sum, bias, leftover: ``|err| <= 1.01 (7 p + 2) u S``.

An element with p = 0 is exactly act(bias) (0 without a bias).
"""
import numpy as np

U = 2.0 ** -24
F32 = np.float32
F64 = np.float64

PROBE_COUNTS = (1, 255, 256, 257, 511, 513, 32768, 32769, 43691, 65535)


def op(X, t):
    return X.T if t else X


def relu64(v):
    """ReLU of the reference: where(v < 0, 0, v) -- a NaN stays NaN."""
    return np.where(v < 0, 0.0, v)


# ----------------------------------------------------------------- builders
def full_mantissa(rng, shape, lo_exp=-1, hi_exp=1):
    """Non-zero fp32 values with all 24 mantissa bits drawn (the last one set),
    random sign, magnitude in [2^lo_exp, 2^hi_exp)."""
    m = rng.integers(2 ** 23, 2 ** 24, size=shape, dtype=np.int64) | 1
    e = rng.integers(lo_exp, hi_exp, size=shape)
    s = rng.integers(0, 2, size=shape) * 2 - 1
    return (s * m * np.exp2(e - 23.0)).astype(F32)


def small_integers(rng, shape):
    """Non-zero integers in +-1..3."""
    table = np.array([-3, -2, -1, 1, 2, 3], dtype=F32)
    return table[rng.integers(0, 6, size=shape, dtype=np.uint8)]


def graded(rng, M, N, K):
    """Dense Gaussian operands, row i of A scaled by 2^(-20 i / M), column j of B
    by 2^(-20 j / N): elements of C span forty binades."""
    A = rng.standard_normal((M, K)) * np.exp2(-20.0 * np.arange(M) / M)[:, None]
    B = rng.standard_normal((K, N)) * np.exp2(-20.0 * np.arange(N) / N)[None, :]
    return A.astype(F32), B.astype(F32)


def probe_positions(K, k_chunk, k_step, k_main=None):
    """The k every probe design has to visit: 0, K - 1, +-1 around every multiple
    of k_chunk and of the k-step, and k_main .. K - 1."""
    ks = {0, K - 1}
    for step in (k_chunk, k_step):
        if step and step > 0:
            m = np.arange(0, K + step, step)
            for d in (-1, 0, 1):
                ks.update((m + d).tolist())
    if k_main is not None:
        ks.update(range(k_main, K))
    return np.array(sorted(k for k in ks if 0 <= k < K), dtype=np.int64)


def probe_rounds(ks, M, K, rng):
    """Split the positions `ks` into launches of M rows (one position per row);
    rows left over in the last launch take random k.  Where M >= K every k is
    visited."""
    if M >= K:
        ks = np.arange(K, dtype=np.int64)
    out = []
    for s in range(0, len(ks), M):
        part = ks[s:s + M]
        if len(part) < M:
            part = np.concatenate([part, rng.integers(0, K, M - len(part))])
        out.append(rng.permutation(part))
    return out


def second_positions(k1, K, k_chunk, k_step, rng):
    """A second non-zero per row: in another split where there is one, else
    beyond the last whole k-step where there is one, else any other k."""
    k1 = np.asarray(k1)
    k2 = np.empty_like(k1)
    tail0 = K // k_step * k_step if k_step else K
    for i, k in enumerate(k1):
        if k_chunk and k_chunk < K:
            nsp = -(-K // k_chunk)
            z = (k // k_chunk + 1 + rng.integers(0, nsp - 1)) % nsp
            lo, hi = z * k_chunk, min(K, (z + 1) * k_chunk)
            k2[i] = rng.integers(lo, hi)
        elif tail0 < K and k < tail0:
            k2[i] = rng.integers(tail0, K)
        else:
            k2[i] = (k + 1 + rng.integers(0, max(K - 1, 1))) % K
    return k2


# ------------------------------------------------- bf16 pieces (count GEMM)
def _bits(v):
    return np.ascontiguousarray(v, dtype=F32).view(np.uint32)


def bf16_rne(v):
    b = _bits(v).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(F32)


def split3(w):
    """w = w1 + w2 + w3, round-to-nearest bf16 remainders (exact for finite w)."""
    w = np.asarray(w, dtype=F32)
    with np.errstate(invalid="ignore"):
        w1 = bf16_rne(w)
        r1 = (w - w1).astype(F32)
        w2 = bf16_rne(r1)
        w3 = bf16_rne((r1 - w2).astype(F32))
    return w1, w2, w3


def cut_hi_lo(x):
    x = np.asarray(x, dtype=F32)
    hi = (_bits(x) & np.uint32(0xFFFF0000)).view(F32)
    return hi, (x - hi).astype(F32)


def three_piece_weights(rng, shape):
    """fp32 weights whose three bf16 pieces are all large: |w2| >= 2^-10 |w| and
    |w3| >= 2^-18 |w| (asserted), so a lost term is not small by luck.  Mantissa
    m1 2^16 + r1 with m1 in 128..159, r1 in [2^14, 2^15) and the low seven bits
    of r1 at least 41 away from a multiple of 128."""
    m1 = rng.integers(128, 160, size=shape)
    top = rng.integers(128, 256, size=shape)            # bits 14..7 of r1
    low = rng.integers(41, 64, size=shape)
    low = np.where(rng.integers(0, 2, size=shape) == 1, 128 - low, low)
    m = m1 * 65536 + top * 128 + low
    e = rng.integers(-30, -20, size=shape)
    s = rng.integers(0, 2, size=shape) * 2 - 1
    w = (s * m * np.exp2(e.astype(F64))).astype(F32)
    w1, w2, w3 = split3(w)
    assert np.array_equal(w1.astype(F64) + w2 + w3, w.astype(F64))
    assert (np.abs(w2) >= 2.0 ** -10 * np.abs(w)).all()
    assert (np.abs(w3) >= 2.0 ** -18 * np.abs(w)).all()
    return w


def significant_bits(c):
    c = int(c)
    return 0 if c == 0 else c.bit_length() - ((c & -c).bit_length() - 1)


def exact_weights(rng, counts):
    """One weight per count such that count * weight fits 24 bits: 24 minus the
    count's significant bits, all of them drawn (first and last set).  A count
    of up to 7 significant bits meets a 17-bit weight (two pieces; a 17-bit
    span can hold no third), a power of two meets all 24 bits (three pieces)."""
    counts = np.asarray(counts, dtype=np.int64)
    nb = 24 - np.vectorize(significant_bits, otypes=[np.int64])(counts)
    m = rng.integers(2 ** (nb - 1), 2 ** nb) | 1
    s = rng.integers(0, 2, size=counts.shape) * 2 - 1
    e = rng.integers(-24, -8, size=counts.shape)
    return (s * m * np.exp2(e.astype(F64))).astype(F32)


# ----------------------------------------------------------- expectations
def expect_dense(A, B, bias=None, c0=None, relu=False, want_p=True):
    """(ref, S, p) of C = C0 + act(A B + bias) in fp64; A [M, K], B [K, N]."""
    A64, B64 = A.astype(F64), B.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = A64 @ B64
        S = np.abs(A64) @ np.abs(B64)
    p = (A64 != 0).astype(F64) @ (B64 != 0).astype(F64) if want_p else None
    return _finish(ref, S, p, bias, c0, relu)


def _finish(ref, S, p, bias, c0, relu):
    if bias is not None:
        ref = ref + bias.astype(F64)[None, :]
        S = S + np.abs(bias.astype(F64))[None, :]
    if relu:
        ref = relu64(ref)
    if c0 is not None:
        ref = ref + c0.astype(F64)
        S = S + np.abs(c0.astype(F64))
    return ref, S, p


def expect_sparse_rows(rows_k, rows_v, B, bias=None, c0=None, relu=False):
    """A has, in row i, the values rows_v[i][t] at k = rows_k[i][t] (t = 0 .. T-1,
    a zero value = no entry): the expectation without a dense product."""
    rows_k = np.asarray(rows_k).reshape(len(rows_k), -1)
    rows_v = np.asarray(rows_v, dtype=F64).reshape(rows_k.shape)
    B64 = B.astype(F64)
    M, N = rows_k.shape[0], B.shape[1]
    ref, S, p = np.zeros((M, N)), np.zeros((M, N)), np.zeros((M, N))
    for t in range(rows_k.shape[1]):
        prod = rows_v[:, t, None] * B64[rows_k[:, t]]
        ref += prod
        S += np.abs(prod)
        p += prod != 0
    return _finish(ref, S, p, bias, c0, relu)


def bound_fp32(S, p, single_exact):
    """single_exact: no bias and no accumulate -- a p = 1 element is one rounding."""
    b = 1.01 * (p + 2.0) * U * S
    if single_exact:
        b = np.where(p == 1, U * S, b)
    return np.where(p == 0, 0.0, b) if single_exact else b


def bound_count(S, p):
    return 1.01 * (7.0 * p + 2.0) * U * S


# --------------------------------------------------------------- checkers
def _where(bad):
    idx = np.argwhere(bad)
    return "{} elements, first {}".format(len(idx), idx[:4].tolist())


def check_bit_equal(got, want):
    """Integer-exact and exact-product cases: the fp32 result is `want` bit for
    bit (want is exact in fp64 and representable)."""
    want32 = want.astype(F32)
    assert np.array_equal(want32.astype(F64), want), "expectation not representable"
    bad = _bits(got) != _bits(want32)
    # (+0 and -0: an exact zero sum is +0 in round-to-nearest)
    assert not bad.any(), "not bit-equal: " + _where(bad)


def check_integer_exact(got, want):
    assert np.abs(want).max() < 2 ** 24
    check_bit_equal(got, want)


def check_bound(got, ref, bound, what=""):
    """|got - ref| <= bound for every element; no element skipped; a zero bound
    demands the exact value.  Returns max err / bound over elements with a
    non-zero bound (information)."""
    got = got.astype(F64)
    assert np.isfinite(got).all(), what + " non-finite output: " + _where(~np.isfinite(got))
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), "{} beyond the bound: {}; worst err/bound {:.3g}".format(
        what, _where(bad), float((err[bad] / np.maximum(bound[bad], 1e-300)).max()))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def classes(v):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    v = np.asarray(v, dtype=F64)
    return np.where(np.isnan(v), 1, np.where(v == np.inf, 2, np.where(v == -np.inf, 3, 0)))


def check_classes(got, ref):
    """fp32 GEMM with non-finite inputs: every element's class equals the fp64
    reference's of the same sums."""
    bad = classes(got) != classes(ref)
    assert not bad.any(), "element class differs: " + _where(bad)


def nonfinite_pre(x_op, spots, N):
    """The fp64 pre-activation where `other[k, j] = v` is planted (spots: (k, j, v), one
    per column): NaN where the count is 0 (0 * inf) or v is NaN, else v; 0 elsewhere."""
    pre = np.zeros((x_op.shape[0], N))
    for k, j, v in spots:
        pre[:, j] = np.where((x_op[:, k] == 0) | np.isnan(v), np.nan, v)
    return pre


def check_nonfinite_kept(got, pre, relu, ref, bound):
    """Count GEMM with non-finite `other`.  `pre`: the fp64 pre-activation where it is
    non-finite (anything finite elsewhere).  Such an element is NaN -- the split of an
    infinity is NaN by construction (w2 = inf - inf) -- or, where the infinity met the
    plain fp32 leftover terms unsplit, what IEEE gives: +-inf, 0 for ReLU(-inf).  A NaN
    reference is NaN.  Every other element meets its bound."""
    got = got.astype(F64)
    nf = ~np.isfinite(pre)
    low = 0.0 if relu else -np.inf
    ok = np.isnan(got) | ((pre == np.inf) & (got == np.inf)) | ((pre == -np.inf) & (got == low))
    lost = nf & ~ok
    assert not lost.any(), "a non-finite value was lost: " + _where(lost)
    err = np.abs(got - ref)
    bad = ~nf & ~(err <= bound)
    assert not bad.any(), "beyond the bound beside non-finite values: " + _where(bad)


def row_sums_fp64(A, B, rows):
    """Rows `rows` of A B summed without BLAS (non-finite values take the IEEE
    path: 0 * inf = NaN, inf - inf = NaN)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(A[r].astype(F64)[:, None] * B.astype(F64)).sum(0) for r in rows])


def check_padding(buf_after, buf_before, view_mask):
    """No byte of the buffer outside the [M, N] view may change."""
    a, b = _bits(buf_after.ravel()), _bits(buf_before.ravel())
    bad = (a != b) & ~view_mask.ravel()
    assert not bad.any(), "bytes outside C changed: " + _where(bad)


# ------------------------------------------------- emulations (host tests)
def _fma_step(acc, prod64):
    """acc (fp32) + an exact product (fp64) rounded once to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc.astype(F64) + prod64).astype(F32)


def emulate_fp32_gemm(A, B, bias=None, c0=None, relu=False, ta=False, tb=False,
                      k_chunk=None, defect=None, at=(0, 0, 0)):
    """A k-ordered fp32 fused-multiply-add chain per split-K slab, slabs summed in
    order, + bias, activation, accumulate.  `defect` names one of FP32_DEFECTS
    (`at` = (i, j, k) of the single-element ones)."""
    if defect == "ignore_ta":
        A2 = A.reshape(A.shape[::-1]) if ta else A       # read as if not transposed
    else:
        A2 = op(A, ta)
    if defect == "ignore_tb":
        B2 = B.reshape(B.shape[::-1]) if tb else B
    else:
        B2 = op(B, tb)
    A2, B2 = np.array(A2, dtype=F32), np.array(B2, dtype=F32)
    if defect == "bf16_operand":
        A2 = bf16_rne(A2)
    if defect == "mant10_operand":
        b = _bits(A2).astype(np.uint64)
        A2 = (((b + 0xFFF + ((b >> 13) & 1)) >> 13) << 13).astype(np.uint32).view(F32)
    M, K = A2.shape
    N = B2.shape[1]
    k_chunk = k_chunk or max(K, 1)
    i0, j0, k0 = at
    total = np.zeros((M, N), dtype=F32)
    nsplit = max(1, -(-K // k_chunk))
    for z in range(nsplit):
        acc = np.zeros((M, N), dtype=F32)
        for k in range(z * k_chunk, min(K, (z + 1) * k_chunk)):
            prod = A2[:, k, None].astype(F64) * B2[None, k, :].astype(F64)
            if defect == "drop_product" and k == k0:
                prod[i0, j0] = 0.0
            if defect == "double_product" and k == k0:
                prod[i0, j0] *= 2.0
            acc = _fma_step(acc, prod)
        if defect == "bias_per_split" and bias is not None:
            acc = (acc + bias[None, :]).astype(F32)
        if defect == "relu_before_sum" and relu:
            acc = np.where(acc < 0, F32(0), acc)
        with np.errstate(invalid="ignore"):
            total = (total + acc).astype(F32) if nsplit > 1 else acc
    return _epilogue(total, bias, c0, relu, defect, at)


def _epilogue(total, bias, c0, relu, defect, at):
    N = total.shape[1]
    with np.errstate(invalid="ignore"):
        if bias is not None and defect != "bias_per_split":
            bb = np.roll(bias, 1) if defect == "bias_wrong_column" and N > 1 else bias
            total = (total + bb[None, :]).astype(F32)
        if relu:
            if defect == "nan_to_zero":
                total = np.fmax(total, F32(0))          # fmax drops a NaN
            else:
                total = np.where(total < 0, F32(0), total).astype(F32)
        elif defect == "nan_to_zero":
            total = np.where(np.isnan(total), F32(0), total)
        if c0 is not None:
            total = (c0 + total).astype(F32)
    if defect == "swap":
        i0, j0, _ = at
        j1 = (j0 + 1) % N
        total = total.copy()
        total[i0, j0], total[i0, j1] = total[i0, j1], total[i0, j0]
    return total


def emulate_count_gemm(x, w, bias=None, relu=False, k_main=None, k_chunk=None,
                       defect=None, at=(0, 0, 0)):
    """x [M, K] counts, w [K, N]: hi/lo cut of x times the three-term split of w,
    the six exact partial products of a k added in fp32 smallest term first,
    per slab; the slabs, the k >= k_main leftover (fp32 fma on the original
    operands), bias, activation.  `defect` names one of COUNT_DEFECTS."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(w, dtype=F32)
    M, K = x.shape
    N = w.shape[1]
    k_main = K if k_main is None else k_main
    k_chunk = k_chunk or max(k_main, 1)
    hi, lo = cut_hi_lo(x)
    w1, w2, w3 = split3(w)
    if defect == "drop_lo":
        lo = np.zeros_like(lo)
    i0, j0, k0 = at
    nsplit = max(1, -(-k_main // k_chunk)) if k_main else 0
    total = np.zeros((M, N), dtype=F32)
    for z in range(nsplit):
        acc = np.zeros((M, N), dtype=F32)
        for k in range(z * k_chunk, min(k_main, (z + 1) * k_chunk)):
            for t, wt in ((3, w3), (2, w2), (1, w1)):
                if (defect == "drop_w2" and t == 2) or (defect == "drop_w3" and t == 3):
                    continue
                for part, xs in (("lo", lo), ("hi", hi)):
                    if defect == "drop_lo_w2" and part == "lo" and t == 2:
                        continue
                    with np.errstate(invalid="ignore"):
                        prod = xs[:, k, None].astype(F64) * wt[None, k, :].astype(F64)
                    if defect == "drop_product" and k == k0:
                        prod[i0, j0] = 0.0
                    if defect == "double_product" and k == k0:
                        prod[i0, j0] *= 2.0
                    acc = _fma_step(acc, prod)
        if defect == "bias_per_split" and bias is not None:
            acc = (acc + bias[None, :]).astype(F32)
        if defect == "relu_before_sum" and relu:
            acc = np.where(acc < 0, F32(0), acc)
        with np.errstate(invalid="ignore"):
            total = (total + acc).astype(F32)
    for k in range(k_main, K):
        with np.errstate(invalid="ignore"):
            prod = x[:, k, None].astype(F64) * w[None, k, :].astype(F64)
        total = _fma_step(total, prod)
    return _epilogue(total, bias, None, relu, defect, at)


FP32_DEFECTS = ("drop_product", "double_product", "swap", "ignore_ta", "ignore_tb",
                "bf16_operand", "mant10_operand", "bias_per_split",
                "bias_wrong_column", "relu_before_sum", "nan_to_zero")
COUNT_DEFECTS = ("drop_product", "double_product", "swap", "drop_w2", "drop_w3",
                 "drop_lo", "drop_lo_w2", "bias_per_split", "bias_wrong_column",
                 "relu_before_sum", "nan_to_zero")


# ------------------------------------------------------ the GPU tests' cases
# fp32 GEMM: (M, N, K), the transposes it runs with, and the route the dispatcher
# has to take with the full workspace: (kernel, splits, k_chunk, reducer).
GEMM_SMALL = [
    # 64-tile kernel, all four (ta, tb)
    ((1, 1, 1), (0, 1, 1, 0)),
    ((1, 1, 0), (0, 1, 0, 0)),
    ((63, 65, 15), (0, 1, 15, 0)),
    ((64, 64, 16), (0, 1, 16, 0)),
    ((65, 63, 17), (0, 1, 17, 0)),
    ((129, 130, 48), (0, 1, 48, 0)),
    ((37, 100, 203), (0, 1, 203, 0)),
    ((300, 500, 1000), (0, 13, 80, 1)),       # slab reducer
    ((37, 100, 5000), (0, 63, 80, 2)),        # wide reducer (78 wanted, 63 after rounding)
    ((130, 70, 5000), (0, 63, 80, 2)),
]
# 128-tile kernel, ta in {0, 1}, tb = 0; each also with no workspace (unsplit)
GEMM_BIG = [
    ((257, 333, 46751), (1, 57, 832, 1)),
    ((2049, 1537, 1283), (1, 1, 1283, 0)),
]
# narrow-N kernel: (M, N, K) with M N K just above 4e9 and K % 16 in {0, 1, 15};
# every shape runs with ta = 0 and 1, ldb = N and N + 3, with and without workspace
GEMM_NARROW = [
    ((255, 65, 241328), (2, 64, 3776, 1)),
    ((256, 72, 217025), (2, 64, 3392, 1)),
    ((257, 97, 160463), (2, 64, 2512, 1)),
    ((513, 100, 77984), (2, 64, 1232, 1)),
    ((256, 104, 150241), (2, 64, 2352, 1)),
]

# count GEMM: (mode, rows, cols, N, epilogue) -> (k_main, splits, k_chunk, direct,
# NQ/NT, pair(u16), waves(u16)); for fp32 x pair = 0 and mode 1 waves = 4.
# epilogue: "" none, "b" bias, "br" bias + ReLU (mode 0 only).
COUNT_CASES = [
    # mode 0: rows x cols -> rows x N.  cols = 31: the reducer does everything; 32, 64, 256: the
    # direct store; 33, 95, 257: one slab + leftover; 1024: split; 1039: split + leftover.
    # mode 1: rows = cells (contracted), cols = genes; an even gene count takes the pair kernel.
    ((0, 1, 31, 1, 'br'), (0, 0, 0, 0, 0, 0, 0)),
    ((0, 255, 31, 33, ''), (0, 0, 0, 0, 0, 0, 0)),
    ((0, 700, 31, 128, 'b'), (0, 0, 0, 0, 0, 0, 0)),
    ((0, 256, 32, 31, 'br'), (32, 1, 32, 1, 1, 0, 8)),
    ((0, 257, 32, 97, ''), (32, 1, 32, 1, 2, 0, 8)),
    ((0, 1, 64, 64, 'b'), (64, 1, 64, 1, 1, 0, 8)),
    ((0, 255, 64, 96, ''), (64, 1, 64, 1, 2, 0, 8)),
    ((0, 700, 256, 65, 'br'), (256, 1, 256, 1, 2, 0, 8)),
    ((0, 256, 256, 128, ''), (256, 1, 256, 1, 2, 0, 8)),
    ((0, 257, 33, 32, ''), (32, 1, 32, 0, 1, 0, 8)),
    ((0, 1, 95, 96, 'br'), (64, 1, 64, 0, 2, 0, 8)),
    ((0, 700, 257, 1, 'b'), (256, 1, 256, 0, 1, 0, 8)),
    ((0, 255, 1024, 33, 'b'), (1024, 4, 256, 0, 1, 0, 8)),
    ((0, 256, 1024, 97, 'br'), (1024, 4, 256, 0, 2, 0, 8)),
    ((0, 1, 1024, 128, ''), (1024, 4, 256, 0, 2, 0, 8)),
    ((0, 257, 1039, 64, 'br'), (1024, 4, 256, 0, 1, 0, 8)),
    ((0, 700, 1039, 31, ''), (1024, 4, 256, 0, 1, 0, 8)),
    ((0, 255, 1039, 65, 'b'), (1024, 4, 256, 0, 2, 0, 8)),
    ((0, 256, 95, 1, ''), (64, 1, 64, 0, 1, 0, 8)),
    ((0, 700, 33, 64, 'b'), (32, 1, 32, 0, 1, 0, 8)),
    ((0, 257, 257, 128, 'br'), (256, 1, 256, 0, 2, 0, 8)),
    ((0, 1, 1039, 32, 'b'), (1024, 4, 256, 0, 1, 0, 8)),
    ((0, 255, 256, 97, ''), (256, 1, 256, 1, 2, 0, 8)),
    ((0, 256, 64, 33, ''), (64, 1, 64, 1, 1, 0, 8)),
    ((0, 700, 1024, 96, ''), (1024, 4, 256, 0, 2, 0, 8)),
    ((1, 15, 1, 1, ''), (0, 0, 0, 0, 0, 0, 0)),
    ((1, 15, 64, 32, ''), (0, 0, 0, 0, 0, 0, 0)),
    ((1, 16, 63, 33, ''), (16, 1, 16, 0, 2, 0, 4)),
    ((1, 16, 256, 64, ''), (16, 1, 16, 0, 2, 1, 4)),
    ((1, 17, 255, 65, ''), (16, 1, 16, 0, 3, 0, 4)),
    ((1, 17, 512, 96, ''), (16, 1, 16, 0, 3, 1, 4)),
    ((1, 31, 257, 97, ''), (16, 1, 16, 0, 4, 0, 4)),
    ((1, 31, 1025, 128, ''), (16, 1, 16, 0, 4, 0, 4)),
    ((1, 48, 64, 1, ''), (48, 1, 48, 0, 1, 1, 4)),
    ((1, 48, 1, 128, ''), (48, 1, 48, 0, 4, 0, 4)),
    ((1, 512, 63, 32, ''), (512, 2, 256, 0, 1, 0, 4)),
    ((1, 512, 256, 97, ''), (512, 2, 256, 0, 4, 1, 4)),
    ((1, 527, 255, 64, ''), (512, 2, 256, 0, 2, 0, 4)),
    ((1, 527, 512, 33, ''), (512, 2, 256, 0, 2, 1, 4)),
    ((1, 512, 1025, 65, ''), (512, 2, 256, 0, 3, 0, 4)),
    ((1, 527, 1025, 96, ''), (512, 2, 256, 0, 3, 0, 4)),
    ((1, 48, 257, 64, ''), (48, 1, 48, 0, 2, 0, 4)),
    ((1, 31, 512, 1, ''), (16, 1, 16, 0, 1, 1, 4)),
]
# the 8-wave weight gradient (uint16 gene pairs; fp32 x: the 4-wave single-gene kernel)
COUNT_WAVES8 = ((1, 14336, 2048, 100, ""), (14336, 56, 256, 0, 4, 1, 8))


def count_route_f32(route_u16, mode):
    """The same shape with fp32 x: never the pair kernel, so 4 waves in mode 1."""
    r = list(route_u16)
    r[5] = 0
    if mode == 1 and r[0] > 0:
        r[6] = 4
    return tuple(r)
