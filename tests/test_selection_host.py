"""Feature selection and example filters on the host
(``scvae_amd/data/processing.py``): parity with the selections the reference's
own code makes (``tests/golden/selection_reference.*``, written by
``tests/golden/make_selection_fixtures.py``), the exact rule against the
Python-integer oracle of ``tests/_selection_oracle.py``, the float fallback,
the errors, ``DataSet`` end to end and the two CLI options.  No GPU."""
import json
import os

import numpy
import pytest
import scipy.sparse

import _selection_oracle as oracle

from scvae_amd.data import processing
from scvae_amd.data.data_set import DataSet
from scvae_amd.data.synthetic import SYNTHETIC_DATA_SETS
from scvae_amd.data.utilities import build_directory_path

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def reference():
    arrays = numpy.load(os.path.join(GOLDEN, "selection_reference.npz"))
    with open(os.path.join(GOLDEN, "selection_reference.json")) as f:
        cases = json.load(f)

    def matrix(name):
        return scipy.sparse.csr_matrix(
            (arrays[name + "_data"].astype(numpy.float32),
             arrays[name + "_indices"].astype(numpy.int32),
             arrays[name + "_indptr"].astype(numpy.int32)),
            shape=tuple(arrays[name + "_shape"]))
    return {"arrays": arrays, "cases": cases, "counts": matrix("counts"),
            "macosko": matrix("macosko"), "labels": arrays["labels"]}


def _last_line(capsys):
    return capsys.readouterr().out.strip().splitlines()[-1]


def test_fixture_holds_the_cases_of_the_issue(reference):
    selections = {(c["method"], tuple(c["parameters"] or ()))
                  for c in reference["cases"]["feature_selection"]}
    for k in (1, 50, 150, 293):
        assert ("keep_highest_variances", (k,)) in selections
    for t in (0.5, 0, 3):
        assert ("keep_variances_above", (t,)) in selections
    assert ("remove_zeros", ()) in selections
    filters = {c["method"] for c in reference["cases"]["example_filter"]}
    assert filters == set(processing.EXAMPLE_FILTERS)
    assert reference["counts"].shape == (400, 300)
    assert int((reference["counts"].sum(axis=0) == 0).sum()) == 7


def test_feature_selections_equal_the_reference(reference, capsys):
    values = reference["counts"]
    names = numpy.array(["gene {}".format(j) for j in range(300)])
    for case in reference["cases"]["feature_selection"]:
        expected = reference["arrays"][case["key"]]
        selected_values, selected_names = processing.select_features(
            {"original": values, "preprocessed": None}, names,
            method=case["method"], parameters=case["parameters"],
            on_device=False)
        line = _last_line(capsys)
        assert selected_names.tolist() == names[expected].tolist(), case
        assert selected_values["preprocessed"] is None
        got = selected_values["original"]
        want = values[:, expected]
        assert got.shape == want.shape == (400, case["selected"])
        assert (got != want).nnz == 0
        assert line.startswith(case["line"] + " ("), (line, case["line"])
        assert line.endswith(").")


def test_example_filters_equal_the_reference(reference, capsys):
    for case in reference["cases"]["example_filter"]:
        values = reference[case["matrix"]]
        n_examples = values.shape[0]
        labels = reference["labels"] if case["matrix"] == "counts" else None
        expected = reference["arrays"][case["key"]]
        if case["method"] == "keep":
            # the one deliberate difference: ascending order, where the
            # reference has the order of a Python set
            expected = numpy.sort(expected)
        filtered_values, names, filtered_labels, batch_indices = (
            processing.filter_examples(
                {"original": values, "preprocessed": None},
                numpy.arange(n_examples), method=case["method"],
                parameters=case["parameters"], labels=labels,
                excluded_classes=case["excluded_classes"],
                batch_indices=numpy.arange(n_examples).reshape(-1, 1) % 3,
                count_sum=numpy.asarray(values.sum(axis=1)).reshape(-1, 1),
                on_device=False))
        line = _last_line(capsys)
        assert names.tolist() == expected.tolist(), case
        assert (filtered_values["original"] != values[expected]).nnz == 0
        assert batch_indices.reshape(-1).tolist() == (expected % 3).tolist()
        if labels is not None:
            assert filtered_labels.tolist() == labels[expected].tolist()
        else:
            assert filtered_labels is None
        assert line.startswith(case["line"] + " ("), (line, case["line"])
        assert (case["removed"], case["remaining"]) == (
            n_examples - len(expected), len(expected))


def _edge_matrix():
    """37 x 53 counts with ties (equal columns, constant columns), empty
    columns and values of 65 535."""
    random_state = numpy.random.RandomState(5)
    dense = random_state.poisson(0.7, size=(37, 53)).astype(numpy.float32)
    dense[:, 4] = dense[:, 9] = dense[:, 30]           # three equal variances
    dense[:, 11] = 7                                   # constant: variance 0
    dense[:, 12] = 65535                               # constant at the limit
    dense[:, [0, 20, 52]] = 0
    dense[::2, 13] = 65535                             # the largest variance
    dense[3, 14] = 65535
    return dense


def test_host_moments_equal_the_oracle():
    dense = _edge_matrix()
    sparse = scipy.sparse.csr_matrix(dense)
    for values in (sparse, dense, sparse.astype(numpy.int64)):
        sums, squares, nonzeros = processing.feature_moments(
            values, on_device=False)
        assert sums.dtype == numpy.uint64 and squares.dtype == numpy.uint64
        assert nonzeros.dtype == numpy.int64
        want = oracle.moments(sparse)
        assert [sums.tolist(), squares.tolist(), nonzeros.tolist()] == list(
            want)
    assert squares[12] == 37 * 65535 ** 2


def test_host_moments_sum_duplicates_and_skip_stored_zeros():
    matrix = scipy.sparse.csr_matrix(
        (numpy.array([1, 2, 0, 5, 3], dtype=numpy.float32),
         numpy.array([2, 2, 1, 0, 2], dtype=numpy.int32),
         numpy.array([0, 3, 5], dtype=numpy.int32)), shape=(2, 3))
    sums, squares, nonzeros = processing.feature_moments(
        matrix, on_device=False)
    assert sums.tolist() == [5, 0, 6]
    assert squares.tolist() == [25, 0, 18]           # (1 + 2)^2 + 3^2
    assert nonzeros.tolist() == [1, 0, 2]
    assert matrix.nnz == 5                           # the input is left alone


def test_host_moments_are_exact_where_fp64_products_are_not():
    """2^20 + 3 rows of 65 535 in one gene: sum x^2 = 4.5e15 and
    N sum x^2 - (sum x)^2 around 2^84 are beyond fp64's 53 bits; more rows
    than one block of the host sums."""
    n = 2 ** 20 + 3
    column = numpy.full(n, 65535, dtype=numpy.float32)
    column[5] = 65534
    matrix = scipy.sparse.csr_matrix(
        (column, numpy.zeros(n, dtype=numpy.int32),
         numpy.arange(n + 1, dtype=numpy.int64)), shape=(n, 1))
    sums, squares, nonzeros = processing.feature_moments(
        matrix, on_device=False)
    assert int(sums[0]) == 65535 * n - 1
    assert int(squares[0]) == 65535 ** 2 * (n - 1) + 65534 ** 2
    assert int(nonzeros[0]) == n
    numerator = processing.variance_numerators(sums, squares, n)[0]
    assert numerator == n * int(squares[0]) - int(sums[0]) ** 2 == n - 1


@pytest.mark.parametrize("method,parameter", [
    ("remove_zeros", None), ("keep_variances_above", None),
    ("keep_variances_above", 0), ("keep_variances_above", "1.25"),
    ("keep_highest_variances", None), ("keep_highest_variances", 1),
    ("keep_highest_variances", 2), ("keep_highest_variances", "3"),
    ("keep_highest_variances", 47), ("keep_highest_variances", 50),
    ("keep_highest_variances", 52)])
def test_host_selection_equals_the_oracle(method, parameter, capsys):
    dense = _edge_matrix()
    sparse = scipy.sparse.csr_matrix(dense)
    names = numpy.arange(53)
    want = oracle.select(sparse, method, parameter)
    for values in (sparse, dense):
        _, selected = processing.select_features(
            {"original": values}, names, method=method,
            parameters=None if parameter is None else [parameter],
            on_device=False)
        assert selected.tolist() == want


def test_ties_go_to_the_higher_gene_index():
    dense = _edge_matrix()
    # genes 4, 9 and 30 are equal: the cut at two of them keeps 9 and 30
    numerators = oracle.numerators(scipy.sparse.csr_matrix(dense))
    assert numerators[4] == numerators[9] == numerators[30]
    above = sum(1 for v in numerators if v > numerators[4])
    _, selected = processing.select_features(
        {"original": scipy.sparse.csr_matrix(dense)}, numpy.arange(53),
        method="keep_highest_variances", parameters=[above + 2],
        on_device=False)
    assert 9 in selected and 30 in selected and 4 not in selected


def test_float_matrices_take_the_fp64_two_pass_path(capsys):
    random_state = numpy.random.RandomState(6)
    dense = random_state.gamma(0.4, 2.0, size=(41, 29)) * (
        random_state.random_sample((41, 29)) < 0.5)
    dense[:, 3] = dense[:, 17]                       # a tie
    dense[:, 8] = 0
    dense = dense.astype(numpy.float32)
    variances = ((dense.astype(numpy.float64)
                  - dense.astype(numpy.float64).mean(axis=0)) ** 2).mean(
                      axis=0)
    for values in (dense, scipy.sparse.csr_matrix(dense)):
        with pytest.raises(ValueError, match="integer counts"):
            processing.feature_moments(values, on_device=False)
        _, selected = processing.select_features(
            {"original": values}, numpy.arange(29),
            method="keep_highest_variances", parameters=[10],
            on_device=False)
        order = numpy.argsort(variances, kind="stable")
        _, sparse_variances = processing._float_column_moments(
            processing._canonical(values))
        numpy.testing.assert_allclose(sparse_variances, variances,
                                      rtol=1e-12, atol=0)
        want = numpy.sort(numpy.argsort(sparse_variances,
                                        kind="stable")[-10:])
        assert selected.tolist() == want.tolist()
        assert set(order[-9:]) <= set(selected.tolist())
        _, selected = processing.select_features(
            {"original": values}, numpy.arange(29), method="remove_zeros",
            on_device=False)
        assert selected.tolist() == [j for j in range(29) if j != 8]
        _, selected = processing.select_features(
            {"original": values}, numpy.arange(29),
            method="keep_variances_above", parameters=[0.3],
            on_device=False)
        assert selected.tolist() == numpy.flatnonzero(
            sparse_variances > 0.3).tolist()


def test_submatrix_on_the_host_is_scipy_on_the_canonical_matrix():
    matrix = oracle.count_matrix(23, 40, 0.3, seed=7, empty_rows=(2, 22),
                                 empty_columns=(0, 39))
    shuffled = matrix.copy()                 # unsorted indices, a stored zero
    for i in range(23):
        begin, end = shuffled.indptr[i], shuffled.indptr[i + 1]
        shuffled.indices[begin:end] = shuffled.indices[begin:end][::-1].copy()
        shuffled.data[begin:end] = shuffled.data[begin:end][::-1].copy()
    shuffled.has_sorted_indices = False
    shuffled.data[1] = 0
    canonical = shuffled.copy()
    canonical.sum_duplicates()
    rows = numpy.random.RandomState(8).permutation(23)[:11]
    columns = numpy.array([1, 2, 3, 17, 38, 39])
    for r, c in ((None, columns), (rows, None), (rows, columns)):
        got = processing.submatrix(shuffled, rows=r, columns=c,
                                   on_device=False)
        want = canonical
        if r is not None:
            want = want[r]
        if c is not None:
            want = want[:, c]
        assert got.shape == want.shape
        assert got.indptr.tolist() == want.indptr.tolist()
        assert got.indices.tolist() == want.indices.tolist()
        assert got.data.tolist() == want.data.tolist()
        assert got.data.dtype == numpy.float32
    assert 0 in processing.submatrix(
        shuffled, on_device=False).data.tolist()     # the stored zero stays
    mask = numpy.zeros(40, dtype=bool)
    mask[columns] = True
    assert (processing.submatrix(shuffled, columns=mask, on_device=False)
            != canonical[:, columns]).nnz == 0
    with pytest.raises(ValueError, match="ascending"):
        processing.submatrix(shuffled, columns=[3, 2], on_device=False)
    with pytest.raises(IndexError):
        processing.submatrix(shuffled, rows=[23], on_device=False)
    with pytest.raises(IndexError):
        processing.submatrix(shuffled, columns=[40], on_device=False)


def test_error_messages(reference):
    values = {"original": reference["counts"], "preprocessed": None}
    names = numpy.arange(300)
    examples = numpy.arange(400)
    labels = reference["labels"]
    with pytest.raises(ValueError,
                       match="Feature selection `keep_best` not found."):
        processing.select_features(values, names, method="keep best",
                                   on_device=False)
    with pytest.raises(ValueError,
                       match="Example filter `mocasko` not found."):
        processing.filter_examples(values, examples, method="mocasko",
                                   on_device=False)
    with pytest.raises(Exception, match="No features excluded using feature "
                                        "selection keep_highest_variances."):
        processing.select_features(values, names,
                                   method="keep_highest_variances",
                                   parameters=[300], on_device=False)
    with pytest.raises(Exception, match="No features excluded using feature "
                                        "selection keep_variances_above."):
        processing.select_features(values, names,
                                   method="keep_variances_above",
                                   parameters=[-1], on_device=False)
    with pytest.raises(Exception, match="No examples filtered out using "
                                        "example filter `remove`."):
        processing.filter_examples(values, examples, method="remove",
                                   parameters=["no such class"],
                                   labels=labels, on_device=False)
    with pytest.raises(Exception, match="No examples filtered out using "
                                        "example filter `random`."):
        processing.filter_examples(values, examples, method="random",
                                   parameters=[400], on_device=False)
    for method in ("keep", "remove", "excluded_classes"):
        with pytest.raises(ValueError, match="Cannot filter examples based on "
                                             "labels, since data set is "
                                             "unlabelled."):
            processing.filter_examples(values, examples, method=method,
                                       parameters=["other"], on_device=False)


def test_superset_labels_are_used_when_given(reference):
    values = {"original": reference["counts"]}
    labels = reference["labels"]
    superset = numpy.where(numpy.isin(labels, ["B cells", "T-cells"]),
                           "lymphocytes", "rest")
    _, names, filtered_labels, _ = processing.filter_examples(
        values, numpy.arange(400), method="excluded_classes", labels=labels,
        excluded_classes=["other"], superset_labels=superset,
        excluded_superset_classes=["lymphocytes"], on_device=False)
    assert names.tolist() == numpy.flatnonzero(superset == "rest").tolist()
    assert filtered_labels.tolist() == labels[superset == "rest"].tolist()


def test_device_is_required_when_asked_for_and_absent(reference):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib
    with pytest.raises(_lib.HipLibraryError, match="no GPU is visible"):
        processing.feature_moments(reference["counts"], on_device=True)
    with pytest.raises(_lib.HipLibraryError, match="no GPU is visible"):
        processing.submatrix(reference["counts"], rows=[0], on_device=True)


# -- DataSet, end to end -------------------------------------------------------

def _data_set(**keyword_arguments):
    return DataSet("synthetic_1k", **keyword_arguments)


@pytest.fixture(scope="module")
def synthetic():
    return SYNTHETIC_DATA_SETS["synthetic_1k"]()


def test_data_set_selects_and_filters(synthetic, capsys):
    values = scipy.sparse.csr_matrix(synthetic["values"])
    data_set = _data_set(feature_selection=["keep_highest_variances", "64"],
                         example_filter=["remove", "cluster 3"])
    data_set.load()
    out = capsys.readouterr().out
    genes = oracle.select(values, "keep_highest_variances", 64)
    cells = numpy.flatnonzero(synthetic["labels"] != "cluster 3")
    assert 0 < len(cells) < 1000
    assert "Selecting features.\n64 features selected, 36 excluded (" in out
    assert ("Filtering examples.\n{} examples filtered out, {} remaining ("
            .format(1000 - len(cells), len(cells))) in out
    assert out.index("Selecting features.") < out.index("Filtering examples.")
    want = values[cells][:, genes]
    assert data_set.values.shape == (len(cells), 64)
    assert (data_set.number_of_examples, data_set.number_of_features) == (
        len(cells), 64)
    assert (data_set.values != want).nnz == 0
    assert data_set.feature_names.tolist() == (
        synthetic["feature names"][genes].tolist())
    assert data_set.example_names.tolist() == (
        synthetic["example names"][cells].tolist())
    assert data_set.labels.tolist() == synthetic["labels"][cells].tolist()
    assert "cluster 3" not in data_set.class_names
    assert data_set.number_of_classes == 7
    numpy.testing.assert_array_equal(
        data_set.count_sum.reshape(-1),
        numpy.asarray(want.sum(axis=1), dtype=numpy.float32).reshape(-1))
    assert data_set.feature_selection_method == "keep_highest_variances"
    assert data_set.feature_selection_parameters == ["64"]
    assert data_set.example_filter_method == "remove"
    assert data_set.example_filter_parameters == ["cluster 3"]
    directory = build_directory_path("models", data_set, "random", 0.9)
    assert directory == os.path.join(
        "models", "synthetic_1k", "split-random_0.9",
        "keep_highest_variances_64-remove_cluster_3")


def test_selection_is_applied_to_both_versions_and_before_the_split(
        synthetic, capsys):
    values = scipy.sparse.csr_matrix(synthetic["values"])
    data_set = _data_set(feature_selection=["keep_highest_variances", "64"],
                         preprocessing_methods=["log"])
    training_set, validation_set, test_set = data_set.split("random", 0.9)
    genes = oracle.select(values, "keep_highest_variances", 64)
    # the genes of the full set, not those of a subset's own variances
    training_rows = data_set.split_indices["training"]
    assert oracle.select(values[training_rows], "keep_highest_variances",
                         64) != genes
    for subset, kind in ((training_set, "training"),
                         (validation_set, "validation"), (test_set, "test")):
        rows = data_set.split_indices[kind]
        assert subset.values.shape == (len(rows), 64)
        assert (subset.values != values[rows][:, genes]).nnz == 0
        assert subset.feature_names.tolist() == (
            synthetic["feature names"][genes].tolist())
        assert subset.feature_selection == ["keep_highest_variances", "64"]
        logged = subset.preprocessed_values
        assert logged.shape == (len(rows), 64)
        numpy.testing.assert_array_equal(
            logged.toarray(),
            numpy.log1p(values[rows][:, genes].toarray()))
    assert capsys.readouterr().out.count("Selecting features.") == 1


def test_default_parameters_are_filled_in_and_named_in_the_directory():
    data_set = _data_set(feature_selection=["keep_highest_variances"])
    assert data_set.feature_selection_parameters is None
    data_set.load()
    assert data_set.feature_selection_parameters == [50]
    assert data_set.number_of_features == 50
    assert build_directory_path("m", data_set).endswith(
        os.path.join("no_split", "keep_highest_variances_50"))
    dense = _edge_matrix()
    data_set = DataSet(
        "edges", feature_selection=["keep_variances_above"],
        generator=lambda: {"values": scipy.sparse.csr_matrix(dense)})
    data_set.load()
    assert data_set.feature_selection_parameters == [0.5]
    assert data_set.number_of_features == len(oracle.select(
        scipy.sparse.csr_matrix(dense), "keep_variances_above", 0.5)) < 53
    assert data_set.feature_names is None and data_set.example_names is None
    assert build_directory_path("m", data_set).endswith(
        os.path.join("edges", "no_split", "keep_variances_above_0.5"))


def test_without_the_options_a_data_set_is_what_the_generator_made(
        synthetic, capsys):
    data_set = _data_set()
    data_set.load()
    out = capsys.readouterr().out
    assert out == ""
    values = scipy.sparse.csr_matrix(synthetic["values"], dtype=numpy.float32)
    assert data_set.values.shape == (1000, 100)
    for name in ("indptr", "indices", "data"):
        numpy.testing.assert_array_equal(getattr(data_set.values, name),
                                         getattr(values, name))
    assert data_set.preprocessed_values is None
    assert data_set.feature_names.tolist() == (
        synthetic["feature names"].tolist())
    assert data_set.example_names.tolist() == (
        synthetic["example names"].tolist())
    assert data_set.labels.tolist() == synthetic["labels"].tolist()
    assert data_set.feature_selection == [] and data_set.example_filter == []
    assert data_set.feature_selection_method is None
    assert data_set.feature_selection_parameters is None
    assert data_set.example_filter_method is None
    assert data_set.example_filter_parameters is None
    assert build_directory_path("m", data_set).endswith(
        os.path.join("synthetic_1k", "no_split", "no_preprocessing"))


# -- CLI -----------------------------------------------------------------------

def test_cli_parses_both_options():
    from scvae_amd import cli
    parser = cli.build_parser()
    for command in ("train", "evaluate"):
        parsed = parser.parse_args([command, "synthetic_1k"])
        assert parsed.feature_selection is None
        assert parsed.example_filter is None
        parsed = parser.parse_args([
            command, "synthetic_1k", "-F", "keep_highest_variances", "64",
            "-E", "remove", "cluster 3", "cluster 4"])
        assert parsed.feature_selection == ["keep_highest_variances", "64"]
        assert parsed.example_filter == ["remove", "cluster 3", "cluster 4"]
        parsed = parser.parse_args([
            command, "synthetic_1k", "--feature-selection", "remove_zeros",
            "--example-filter", "macosko"])
        assert parsed.feature_selection == ["remove_zeros"]
        assert parsed.example_filter == ["macosko"]


def test_cli_hands_the_options_to_the_data_set(capsys):
    from scvae_amd import cli
    data_set, subsets, _, _ = cli._load_data(
        "synthetic_1k", None, None, None, None, True, "random", 0.9,
        feature_selection=["keep_highest_variances", "64"],
        example_filter=["random", "500"])
    assert data_set.values.shape == (500, 64)
    assert [s.values.shape for s in subsets] == [
        (405, 64), (45, 64), (50, 64)]
    data_set, subsets, _, _ = cli._load_data(
        "synthetic_1k", None, None, None, None, False, None, None)
    assert data_set.values.shape == (1000, 100)
    import inspect
    for function in (cli.train, cli.evaluate):
        parameters = inspect.signature(function).parameters
        assert parameters["feature_selection"].default is None
        assert parameters["example_filter"].default is None
