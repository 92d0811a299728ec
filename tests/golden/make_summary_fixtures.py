#!/usr/bin/env python3
"""Golden tables printed by the REFERENCE's own ``format_summary_statistics``
(build container only).

The reference's ``analyses/metrics/summary.py`` imports the ``scvae`` package
(and with it TensorFlow, which is not importable here), so the function's
definition is pulled out of the source file with ``ast`` and run where it lies
under /root/reference, as ``make_reference_fixtures.py`` does.  Statistic sets
and the tables the function returns for them go to

    tests/golden/summary_tables.json

``tests/test_summary_host.py`` compares the build's restatement with those.
Only the sets and the tables travel; no reference source text is stored.

Function executed (file:line in /root/reference/scvae):
    analyses/metrics/summary.py:60-93    format_summary_statistics
"""
import ast
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "/root/reference/scvae/analyses/metrics/summary.py"


def reference_function(name):
    with open(SOURCE) as f:
        body = ast.parse(f.read()).body
    picked = [n for n in body if isinstance(n, ast.FunctionDef)
              and n.name == name]
    if not picked:
        raise KeyError(name)
    namespace = {}
    exec(compile(ast.Module(body=picked, type_ignores=[]), SOURCE, "exec"),
         namespace)
    return namespace[name]


def statistics(name, mean, standard_deviation, minimum, maximum, sparsity):
    return {
        "name": name, "mean": mean,
        "standard deviation": standard_deviation,
        "minimum": minimum, "maximum": maximum,
        "dispersion": (standard_deviation ** 2 / mean if mean
                       else float("nan")),
        "sparsity": sparsity,
    }


NAN = float("nan")
CASES = {
    # the table of an extensive analysis: nan sparsities in the last two rows
    "extensive": {"sets": [
        statistics("original", 0.2718281828, 3.14159265, 0.0, 2847.0,
                   0.9324512),
        statistics("reconstructed", 0.27055, 2.987654321, 1.2345e-9,
                   2101.337, 0.9876543),
        statistics("differences", 0.0912345, 1.23456789, 0.0, 1500.25, NAN),
        statistics("log-ratios", 0.04567891, 0.2345678, 0.0, 7.123456, NAN)]},
    # one dict, not a list
    "single": {"sets": statistics("original", 1234567.0, 7654321.5, -12.5,
                                  98765432.1, 0.0)},
    # a name longer than the heading's
    "long name": {"sets": [
        statistics("a transformed and binarised set", 0.125, 0.33072, 0.0,
                   1.0, 0.875),
        statistics("reconstructed", 0.1249, 0.2, 1e-12, 0.999999, 1.0)]},
    # a heading of the caller's, longer than the names
    "custom heading": {"name": "Evaluation sets of the model", "sets": [
        statistics("x", 1e-7, 2.5e-5, -1e-3, 1e-3, NAN),
        statistics("y", NAN, NAN, NAN, NAN, NAN),
        statistics("z", float("inf"), NAN, 0.0, float("inf"), 0.5)]},
    # all zeros: a nan dispersion
    "zeros": {"sets": [statistics("", 0.0, 0.0, 0.0, 0.0, 1.0)]},
}


def main():
    format_summary_statistics = reference_function(
        "format_summary_statistics")
    out = {}
    for title, case in CASES.items():
        keyword_arguments = (
            {"name": case["name"]} if "name" in case else {})
        out[title] = dict(case, table=format_summary_statistics(
            case["sets"], **keyword_arguments))
    path = os.path.join(HERE, "summary_tables.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
