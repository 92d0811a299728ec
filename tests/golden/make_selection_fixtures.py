#!/usr/bin/env python3
"""Feature selections and example filters as the REFERENCE's own code makes
them (build container only): the method of ``make_reference_fixtures.py``.

``SparseRowMatrix`` (data/sparse.py:23-62), ``select_features`` and
``filter_examples`` (data/processing.py:95-302), ``normalise_string`` and
``format_duration`` (utilities.py:36-76) are pulled out of the reference
source files with ``ast`` and run where they lie; only inputs, selected
indices, filter indices and the printed summary lines are written, to

    tests/golden/selection_reference.npz
    tests/golden/selection_reference.json

``tests/test_selection_host.py`` compares the build with those.

The reference takes the variances in fp32 as E[x^2] - E[x]^2 and orders them
with an unstable sort; the build decides both exactly
(``tests/_selection_oracle.py``).  Every case is checked here against the
exact rule: one where the reference differs is dropped with a printed line,
not stored.
"""
import ast
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _selection_oracle as oracle                      # noqa: E402
from make_reference_fixtures import REF, load_plain_module   # noqa: E402


def definitions(relative, names, namespace):
    """Compile the named top-level classes and functions of a reference file
    into ``namespace``."""
    with open(os.path.join(REF, relative)) as f:
        body = ast.parse(f.read()).body
    picked = [n for n in body
              if isinstance(n, (ast.FunctionDef, ast.ClassDef))
              and n.name in names]
    missing = set(names) - {n.name for n in picked}
    if missing:
        raise KeyError("{}: {} not found".format(relative, sorted(missing)))
    exec(compile(ast.Module(body=picked, type_ignores=[]),
                 os.path.join(REF, relative), "exec"), namespace)
    return namespace


def count_matrix():
    """400 x 300 gamma-Poisson counts, about 60 % zeros, 7 all-zero genes."""
    random_state = numpy.random.RandomState(20)
    rates = random_state.gamma(0.5, 3.0, size=(400, 300))
    rates *= random_state.gamma(2.0, 0.5, size=(1, 300))
    counts = random_state.poisson(rates)
    counts[:, [3, 41, 42, 118, 200, 251, 299]] = 0
    return counts.astype(numpy.float32)


def macosko_matrix():
    """60 x 1200, rows of 880 .. 920 non-zeros: both sides of 900, and 900."""
    random_state = numpy.random.RandomState(21)
    counts = numpy.zeros((60, 1200), dtype=numpy.float32)
    for i in range(60):
        n = 900 if i in (7, 8) else 880 + (i * 7) % 41
        columns = random_state.permutation(1200)[:n]
        counts[i, columns] = 1 + random_state.poisson(1.5, size=n)
    return counts


def summary_numbers(printed):
    """The two counts of the reference's summary line."""
    line = printed.strip().splitlines()[-1]
    words = line.split()
    return line.rsplit(" (", 1)[0], int(words[0]), int(words[
        4 if "examples" in line else 3])


def main():
    utilities = load_plain_module("utilities.py", "_ref_utilities")
    namespace = {"numpy": numpy, "scipy": scipy, "time": time.time,
                 "normalise_string": utilities.normalise_string,
                 "format_duration": utilities.format_duration}
    definitions("data/sparse.py", ["SparseRowMatrix"], namespace)
    definitions("data/processing.py", ["select_features", "filter_examples"],
                namespace)
    SparseRowMatrix = namespace["SparseRowMatrix"]
    select_features = namespace["select_features"]
    filter_examples = namespace["filter_examples"]

    counts = count_matrix()
    macosko = macosko_matrix()
    random_state = numpy.random.RandomState(22)
    class_names = numpy.array(["B cells", "T-cells", "NK (bright)", "other"])
    labels = class_names[random_state.randint(0, 4, size=400)]
    print("count matrix: {:.1%} zeros, {} all-zero genes".format(
        (counts == 0).mean(), int((counts.sum(axis=0) == 0).sum())))

    arrays, cases = {}, {"feature_selection": [], "example_filter": []}
    for name, dense in (("counts", counts), ("macosko", macosko)):
        sparse = scipy.sparse.csr_matrix(dense)
        arrays[name + "_indptr"] = sparse.indptr.astype(numpy.int32)
        arrays[name + "_indices"] = sparse.indices.astype(numpy.int16)
        arrays[name + "_data"] = sparse.data.astype(numpy.uint16)
        arrays[name + "_shape"] = numpy.array(dense.shape)
    arrays["labels"] = labels

    # ---- feature selections ------------------------------------------------
    values = SparseRowMatrix(scipy.sparse.csr_matrix(counts))
    feature_names = numpy.arange(300)
    selections = ([("keep_highest_variances", [k]) for k in (1, 50, 150, 293)]
                  + [("keep_variances_above", [t]) for t in (0.5, 0, 3)]
                  + [("keep_variances_above", None),
                     ("keep_highest_variances", None), ("remove_zeros", None)])
    for method, parameters in selections:
        printed = io.StringIO()
        with redirect_stdout(printed):
            selected_values, selected = select_features(
                {"original": values, "preprocessed": None}, feature_names,
                method=method, parameters=parameters)
        exact = oracle.select(
            scipy.sparse.csr_matrix(counts), method,
            parameters[0] if parameters else None)
        key = "selection_{}".format(len(cases["feature_selection"]))
        if list(selected) != exact:
            print("DROPPED {} {}: the reference's fp32 variances or its sort "
                  "differ from the exact rule in {} genes".format(
                      method, parameters,
                      len(set(selected) ^ set(exact))))
            continue
        assert selected_values["original"].shape == (400, len(selected))
        line, n_selected, n_excluded = summary_numbers(printed.getvalue())
        arrays[key] = numpy.asarray(selected, dtype=numpy.int32)
        cases["feature_selection"].append({
            "key": key, "method": method, "parameters": parameters,
            "line": line, "selected": n_selected, "excluded": n_excluded})

    # ---- example filters ---------------------------------------------------
    count_sum = counts.sum(axis=1).reshape(-1, 1)
    filters = [
        ("macosko", "macosko", None), ("macosko", "inverse_macosko", None),
        ("counts", "keep", ["T cells", "other"]),
        ("counts", "remove", ["NK bright"]),
        ("counts", "remove", ["b_cells", "Other"]),
        ("counts", "excluded_classes", None),
        ("counts", "remove_count_sum_above", [int(numpy.median(count_sum))]),
        ("counts", "random", [123]), ("counts", "random", ["37"]),
    ]
    for matrix, method, parameters in filters:
        dense = counts if matrix == "counts" else macosko
        n_examples = dense.shape[0]
        printed = io.StringIO()
        with redirect_stdout(printed):
            filtered_values, filtered_names, filtered_labels, _ = (
                filter_examples(
                    {"original": SparseRowMatrix(
                        scipy.sparse.csr_matrix(dense)),
                     "preprocessed": None},
                    numpy.arange(n_examples), method=method,
                    parameters=parameters,
                    labels=labels if matrix == "counts" else None,
                    excluded_classes=["other"],
                    count_sum=dense.sum(axis=1).reshape(-1, 1)))
        assert filtered_values["original"].shape[0] == len(filtered_names)
        line, n_removed, n_remaining = summary_numbers(printed.getvalue())
        key = "filter_{}".format(len(cases["example_filter"]))
        arrays[key] = numpy.asarray(filtered_names, dtype=numpy.int32)
        cases["example_filter"].append({
            "key": key, "matrix": matrix, "method": method,
            "parameters": parameters, "excluded_classes": ["other"],
            "line": line, "removed": n_removed, "remaining": n_remaining})

    numpy.savez_compressed(
        os.path.join(HERE, "selection_reference.npz"), **arrays)
    cases["reference"] = (
        "scvae/scvae v2.1.4: data/processing.py:95-302 executed by "
        "tests/golden/make_selection_fixtures.py")
    with open(os.path.join(HERE, "selection_reference.json"), "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
    print("{} feature selections and {} example filters written to {}".format(
        len(cases["feature_selection"]), len(cases["example_filter"]), HERE))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("this script needs the reference checkout at " + REF)
    main()
