"""Feature selection and example filters on the device
(``scvae_amd/csrc/selection.hip`` through the C ABI and through
``scvae_amd/data/processing.py``): the moments ``==`` the Python-integer
oracle of ``tests/_selection_oracle.py``, the sub-matrix bit-identical to
SciPy's indexing, the device path equal to the host path array for array, and
one whole run of the CLI.

The moments kernel splits the stored entries, not the rows: a workgroup takes
a slab of 8192 genes and a stretch of entries in tiles of 4096 (1024 threads
x 4), at most 2^23 entries between two flushes of its slab.  The shapes: one
slab + 37 genes that are a multiple of nothing; a sum beyond 2^32; 1 x 1;
column indices beyond 16 bits; one entry more than a tile; and 2^20 genes
with more entries than the four stretches of that launch take in one pass
(4 x 2^23), so that workgroups flush, empty their slab and go on."""
import ctypes
import os
import subprocess
import sys

import numpy
import pytest
import scipy.sparse
import torch

import _selection_oracle as oracle

from scvae_amd import _lib
from scvae_amd.data import processing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB = 8192
TILE = 4096


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr() if tensor is not None else None)


def _moments(device, indptr, indices, values, n_rows, n_features, bad=None):
    """The three results of ``scvae_csr_feature_moments`` as NumPy arrays,
    and the ``bad`` word."""
    lib = _lib.load()
    d_indptr = torch.as_tensor(numpy.asarray(indptr, dtype=numpy.int64)).to(
        device)
    d_indices = torch.as_tensor(numpy.asarray(indices, dtype=numpy.int32)).to(
        device)
    d_values = torch.as_tensor(numpy.asarray(values, dtype=numpy.float32)).to(
        device)
    results = torch.full((3, n_features), -7, dtype=torch.int64,
                         device=device)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.check(lib.scvae_csr_feature_moments(
        _ptr(d_indptr), _ptr(d_indices), _ptr(d_values), n_rows, n_features,
        _ptr(results[0]), _ptr(results[1]), _ptr(results[2]), _ptr(bad),
        None), "scvae_csr_feature_moments")
    torch.cuda.synchronize(device)
    results = results.cpu().numpy()
    return (results[0].view(numpy.uint64), results[1].view(numpy.uint64),
            results[2], int(bad.item()))


def _matrix_moments(device, matrix):
    return _moments(device, matrix.indptr, matrix.indices, matrix.data,
                    *matrix.shape)


def _assert_oracle(device, matrix):
    sums, squares, nonzeros, bad = _matrix_moments(device, matrix)
    want = oracle.moments(matrix)
    assert bad == 0
    assert sums.tolist() == want[0]
    assert squares.tolist() == want[1]
    assert nonzeros.tolist() == want[2]
    return sums, squares, nonzeros


@pytest.fixture(scope="module")
def slab_matrix():
    """300 x (8192 + 37), about 5 % non-zero, empty rows and genes, 65 535s."""
    return oracle.count_matrix(
        300, SLAB + 37, 0.05, seed=31, empty_rows=(0, 17, 299),
        empty_columns=(0, 8191, 8192, SLAB + 36), maxima=40)


def test_moments_across_a_slab_boundary(cuda_device, slab_matrix):
    sums, _, nonzeros = _assert_oracle(cuda_device, slab_matrix)
    assert sums[SLAB - 2] and sums[SLAB + 1]           # both slabs are used
    assert nonzeros[[0, 8191, 8192, SLAB + 36]].tolist() == [0, 0, 0, 0]
    again = _matrix_moments(cuda_device, slab_matrix)
    for first, second in zip((sums, nonzeros), (again[0], again[2])):
        assert first.tobytes() == second.tobytes()
    assert again[1].tobytes() == _matrix_moments(
        cuda_device, slab_matrix)[1].tobytes()


def test_moments_of_a_sum_beyond_32_bits(cuda_device):
    n = 70001
    rows = numpy.concatenate([numpy.arange(n), [n - 1]])
    columns = numpy.concatenate([numpy.ones(n, dtype=numpy.int64), [2]])
    data = numpy.concatenate([numpy.full(n, 65535.0), [3.0]])
    matrix = scipy.sparse.csr_matrix(
        (data.astype(numpy.float32), (rows, columns)), shape=(n, 3))
    sums, squares, nonzeros, bad = _matrix_moments(cuda_device, matrix)
    assert bad == 0
    assert sums.tolist() == [0, 65535 * n, 3] and sums[1] > 2 ** 32
    assert squares.tolist() == [0, 65535 ** 2 * n, 9]
    assert nonzeros.tolist() == [0, n, 1]


@pytest.mark.parametrize("value", [0.0, 1.0, 65535.0])
def test_moments_of_one_value(cuda_device, value):
    sums, squares, nonzeros, bad = _moments(
        cuda_device, [0, 1], [0], [value], 1, 1)
    x = int(value)
    assert (sums.tolist(), squares.tolist(), nonzeros.tolist(), bad) == (
        [x], [x * x], [1 if x else 0], 0)


def test_moments_of_an_empty_matrix(cuda_device):
    sums, squares, nonzeros, bad = _moments(
        cuda_device, [0, 0, 0], [], [], 2, 5)
    assert sums.tolist() == squares.tolist() == nonzeros.tolist() == [0] * 5
    assert bad == 0


def test_moments_with_column_indices_beyond_16_bits(cuda_device):
    dense = oracle.count_matrix(2, 70000, 0.4, seed=32, maxima=5).toarray()
    dense[1, 69999] = 12
    sums, _, _ = _assert_oracle(cuda_device, scipy.sparse.csr_matrix(dense))
    assert sums[69999] >= 12


def test_moments_of_one_entry_more_than_a_tile(cuda_device):
    """TILE + 1 stored entries: the second workgroup of the slab takes one."""
    random_state = numpy.random.RandomState(33)
    dense = numpy.zeros((3, 2000), dtype=numpy.float32)
    cells = random_state.permutation(6000)[:TILE + 1]
    dense.reshape(-1)[cells] = 1 + random_state.poisson(2.0, size=TILE + 1)
    matrix = scipy.sparse.csr_matrix(dense)
    assert matrix.nnz == TILE + 1
    _assert_oracle(cuda_device, matrix)


def test_moments_with_explicitly_stored_zeros(cuda_device):
    sums, squares, nonzeros, bad = _moments(
        cuda_device, [0, 3, 5], [0, 1, 2, 1, 2], [0, 4, 0, 0, 9], 2, 3)
    assert (sums.tolist(), squares.tolist(), nonzeros.tolist(), bad) == (
        [0, 4, 9], [0, 16, 81], [0, 1, 1], 0)


def test_moments_over_more_than_one_pass_of_a_workgroup(cuda_device):
    """2^20 genes are 128 slabs and so 4 stretches of at most 2^23 entries:
    4 x 2^23 + 4097 entries (duplicates, which the kernel adds up) make the
    first workgroup of every slab flush, empty its slab and take a second
    stretch.  The reference here is ``numpy.bincount`` on integers."""
    n_features = 2 ** 20
    total = 4 * 2 ** 23 + 4097
    position = numpy.arange(total, dtype=numpy.int64)
    indices = ((position * 7919) % n_features).astype(numpy.int32)
    values = (position % 3).astype(numpy.float32)          # 0, 1, 2
    indices[-1] = n_features - 1
    values[-1] = 65535
    sums, squares, nonzeros, bad = _moments(
        cuda_device, [0, 11, total], indices, values, 2, n_features)
    assert bad == 0
    integers = values.astype(numpy.int64)
    for got, weights in ((sums, integers), (squares, integers * integers),
                         (nonzeros, (integers != 0).astype(numpy.int64))):
        # every sum here is below 2^53: bincount's fp64 sums are exact
        want = numpy.bincount(indices, weights=weights,
                              minlength=n_features).astype(numpy.int64)
        assert numpy.array_equal(got.astype(numpy.int64), want)


@pytest.mark.parametrize("value", [2.5, 65536.0, -1.0, float("nan")])
def test_bad_values_set_bit_0(cuda_device, value):
    sums, squares, nonzeros, bad = _moments(
        cuda_device, [0, 2, 3], [0, 1, 1], [3, value, 5], 2, 2)
    assert bad == 1
    assert (sums.tolist(), squares.tolist(), nonzeros.tolist()) == (
        [3, 5], [9, 25], [1, 1])                      # the value is left out


def test_a_column_index_outside_the_genes_sets_bit_1(cuda_device):
    for index in (2, -1):
        sums, _, _, bad = _moments(
            cuda_device, [0, 2, 3], [0, index, 1], [3, 4, 5], 2, 2)
        assert bad == 2 and sums.tolist() == [3, 5]
    # the word is set, never cleared
    word = torch.tensor([1], dtype=torch.int32, device=cuda_device)
    assert _moments(cuda_device, [0, 1], [5], [1], 1, 2, bad=word)[3] == 3
    assert _moments(cuda_device, [0, 1], [0], [1], 1, 2, bad=word)[3] == 3


def test_limits_are_refused(cuda_device):
    lib = _lib.load()
    word = torch.zeros(4, dtype=torch.int64, device=cuda_device)
    for n_rows, n_features in ((0, 1), (2 ** 31, 1), (1, 0), (1, 2 ** 20 + 1)):
        assert lib.scvae_csr_feature_moments(
            _ptr(word), _ptr(word), _ptr(word), n_rows, n_features,
            _ptr(word), _ptr(word), _ptr(word), _ptr(word), None) == -1
        assert b"bad argument" in lib.scvae_last_error()


# -- sub-matrix -----------------------------------------------------------------

def _assert_same_csr(got, want):
    assert got.shape == want.shape
    assert got.indptr.tolist() == want.indptr.tolist()
    assert got.indices.tolist() == want.indices.tolist()
    assert got.data.tobytes() == want.data.astype(numpy.float32).tobytes()


def test_submatrix_is_bit_identical_to_scipy(cuda_device, slab_matrix):
    matrix = slab_matrix.copy()
    matrix.data[5] = 0                                   # a stored zero
    n_rows, n_features = matrix.shape
    random_state = numpy.random.RandomState(34)
    columns = numpy.sort(random_state.permutation(n_features)[:3000])
    rows = numpy.sort(random_state.permutation(n_rows)[:120])
    permutation = random_state.permutation(n_rows)
    # four columns: most rows lose all their entries, a few keep some
    few = numpy.sort(matrix[1].indices[:4])
    kept_per_row = numpy.diff(matrix[:, few].indptr)
    assert (kept_per_row == 0).sum() > 100 and (kept_per_row > 0).sum() > 4
    cases = [(None, columns), (rows, None), (rows, columns), (None, few),
             (permutation, None), (permutation, columns),
             (numpy.array([3, 3, 0]), columns[:1]), (None, None)]
    for r, c in cases:
        got = processing.submatrix(matrix, rows=r, columns=c, on_device=True)
        want = matrix
        if r is not None:
            want = want[r]
        if c is not None:
            want = want[:, c]
        _assert_same_csr(got, want)
        _assert_same_csr(got, processing.submatrix(
            matrix, rows=r, columns=c, on_device=False))
    assert 0 in processing.submatrix(matrix, on_device=True).data.tolist()


def test_submatrix_takes_an_unsorted_matrix_with_duplicates(cuda_device):
    matrix = scipy.sparse.csr_matrix(
        (numpy.array([1, 2, 7, 5, 3, 4], dtype=numpy.float32),
         numpy.array([2, 2, 0, 1, 2, 0], dtype=numpy.int32),
         numpy.array([0, 3, 3, 6], dtype=numpy.int32)), shape=(3, 3))
    got = processing.submatrix(matrix, rows=[2, 1, 0], columns=[0, 2],
                               on_device=True)
    assert got.toarray().tolist() == [[4, 3], [0, 0], [7, 3]]
    assert got.indptr.tolist() == [0, 2, 2, 4]
    assert got.indices.tolist() == [0, 1, 0, 1]


def test_submatrix_flags_rows_outside_the_matrix(cuda_device):
    lib = _lib.load()
    indptr = torch.tensor([0, 1, 2], dtype=torch.int64, device=cuda_device)
    indices = torch.tensor([0, 1], dtype=torch.int32, device=cuda_device)
    rows = torch.tensor([1, 2, -1, 0], dtype=torch.int64, device=cuda_device)
    counts = torch.full((4,), -1, dtype=torch.int64, device=cuda_device)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    _lib.check(lib.scvae_csr_submatrix_count(
        _ptr(indptr), _ptr(indices), 2, 2, _ptr(rows), 4, None, _ptr(counts),
        _ptr(bad), None), "scvae_csr_submatrix_count")
    assert counts.tolist() == [1, 0, 0, 1] and int(bad.item()) == 8


# -- the host layer on the device -----------------------------------------------

@pytest.mark.parametrize("method,parameters", [
    ("keep_highest_variances", [5000]), ("keep_highest_variances", [1]),
    ("keep_variances_above", [0.5]), ("remove_zeros", None)])
def test_select_features_on_the_device_equals_the_host(
        cuda_device, slab_matrix, method, parameters, capsys):
    names = numpy.arange(slab_matrix.shape[1])
    logged = processing.build_preprocessor(["log"])(slab_matrix)
    versions = {"original": slab_matrix, "preprocessed": logged, "none": None}
    on_device = processing.select_features(
        versions, names, method=method, parameters=parameters, on_device=True)
    on_host = processing.select_features(
        versions, names, method=method, parameters=parameters,
        on_device=False)
    assert "not used" not in capsys.readouterr().out
    assert on_device[1].tolist() == on_host[1].tolist()
    assert on_device[1].tolist() == oracle.select(
        slab_matrix, method, parameters[0] if parameters else None)
    for version in ("original", "preprocessed"):
        _assert_same_csr(on_device[0][version], on_host[0][version])
        assert on_device[0][version].shape[1] == len(on_host[1])
    assert on_device[0]["none"] is None and on_host[0]["none"] is None
    moments = [processing.feature_moments(slab_matrix, on_device=flag)
               for flag in (True, False)]
    for a, b in zip(*moments):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("method,parameters", [
    ("random", [111]), ("remove_count_sum_above", "median"),
    ("inverse_macosko", None)])
def test_filter_examples_on_the_device_equals_the_host(
        cuda_device, slab_matrix, method, parameters):
    count_sum = numpy.asarray(slab_matrix.sum(axis=1)).reshape(-1, 1)
    if parameters == "median":
        parameters = [int(numpy.median(count_sum))]
    if method == "inverse_macosko":
        # rows on both sides of 900 non-zeros
        dense = numpy.zeros((9, 1200), dtype=numpy.float32)
        for i in range(9):
            dense[i, :896 + i] = 1 + i
        values = scipy.sparse.csr_matrix(dense)
    else:
        values = slab_matrix
    n_examples = values.shape[0]
    versions = {"original": values,
                "preprocessed": processing.build_preprocessor(["log"])(values)}
    results = [processing.filter_examples(
        versions, numpy.arange(n_examples), method=method,
        parameters=parameters, count_sum=count_sum, on_device=flag)
        for flag in (True, False)]
    assert results[0][1].tolist() == results[1][1].tolist()
    assert 0 < len(results[0][1]) < n_examples
    if method == "inverse_macosko":
        assert results[0][1].tolist() == [0, 1, 2, 3, 4]
    for version in versions:
        _assert_same_csr(results[0][0][version], results[1][0][version])
        _assert_same_csr(results[0][0][version],
                         versions[version][results[0][1]])


def test_a_float_matrix_falls_back_and_says_so(cuda_device, capsys):
    random_state = numpy.random.RandomState(35)
    values = scipy.sparse.csr_matrix(
        (random_state.gamma(0.5, 2.0, size=(50, 40))
         * (random_state.random_sample((50, 40)) < 0.3)).astype(numpy.float32))
    names = numpy.arange(40)
    _, selected = processing.select_features(
        {"original": values}, names, method="keep_highest_variances",
        parameters=[10])
    out = capsys.readouterr().out
    assert ("feature selection on the device not used: the values are not "
            "integer counts in [0, 65535].") in out
    _, on_host = processing.select_features(
        {"original": values}, names, method="keep_highest_variances",
        parameters=[10], on_device=False)
    assert "not used" not in capsys.readouterr().out
    assert selected.tolist() == on_host.tolist()
    with pytest.raises(_lib.HipLibraryError, match="not integer counts"):
        processing.select_features(
            {"original": values}, names, method="keep_highest_variances",
            parameters=[10], on_device=True)
    processing.filter_examples(
        {"original": values.toarray()}, numpy.arange(50), method="random",
        parameters=[5])
    assert ("example filter on the device not used: the values are a dense "
            "array.") in capsys.readouterr().out


# -- the whole path -------------------------------------------------------------

def test_cli_trains_and_evaluates_on_the_selected_features(cuda_device,
                                                           tmp_path):
    models = str(tmp_path / "models")
    arguments = ["synthetic_1k", "-M", models, "-r", "negative_binomial",
                 "-l", "3", "-H", "20", "-B", "100",
                 "-F", "keep_highest_variances", "64"]
    entry = os.path.join(ROOT, "tests", "_cli_entry.py")
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(key, None)
    outputs = []
    for command in (["train"] + arguments + ["-e", "1"],
                    ["evaluate"] + arguments):
        done = subprocess.run([sys.executable, entry] + command, env=env,
                              cwd=ROOT, capture_output=True, text=True,
                              timeout=600)
        assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
        outputs.append(done.stdout)
    for output in outputs:
        assert "Selecting features.\n64 features selected, 36 excluded (" in (
            output)
        assert "not used" not in output
    assert "(64, 20)" in outputs[0] and "(100, 20)" not in outputs[0]
    assert "Evaluating trained" in outputs[1]
    from scvae_amd.models.utilities import (checkpoint_epoch,
                                            get_checkpoint_state)
    directory = os.path.join(
        models, "synthetic_1k", "no_split", "keep_highest_variances_64",
        "VAE", "gaussian", "negative_binomial-l_3-h_20-mc_1-iw_1-kl-bn")
    path = get_checkpoint_state(directory)
    assert path and checkpoint_epoch(path) == 1
