"""Host side of the device summary statistics (``analyses/summary.py``,
``csrc/summary.hip``): the C entries exist and refuse bad arguments, the
table is the reference's text, argument errors need no GPU, and
``--summary-statistics`` / ``--analysis-level`` reach ``model.evaluate``."""
import ctypes
import json
import math
import os
import re

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scvae_summary_workspace_bytes", "scvae_summary_reset",
         "scvae_summary_accumulate", "scvae_summary_finish")


def test_entries_are_declared_bound_and_exported():
    from scvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "scvae_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    nbytes = lib.scvae_summary_workspace_bytes()
    assert nbytes > 0 and nbytes % 8 == 0


def test_entries_refuse_bad_arguments_without_a_gpu():
    """-1 and a message naming the argument; every pointer and size is
    checked before anything is launched (there is no GPU here to launch on)."""
    from scvae_amd import _lib
    lib = _lib.load()
    need = lib.scvae_summary_workspace_bytes()
    buffer = (ctypes.c_double * 64)()
    p = ctypes.cast(buffer, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)

    def accumulate(recon=p, ldr=8, orig=p, ldo=8, rows=4, features=8,
                   comparisons=0, workspace=p, nbytes=need):
        return lib.scvae_summary_accumulate(
            recon, ldr, orig, ldo, rows, features, 0.5, comparisons,
            workspace, nbytes, None)
    for arguments, names in (
            ({"rows": 0}, "rows >= 1"), ({"features": 0}, "F >= 1"),
            ({"rows": -3}, "rows >= 1"),
            ({"features": 2 ** 31 - 8192, "ldr": 2 ** 31, "ldo": 2 ** 31},
             "F <= INT32_MAX"),
            ({"ldr": 7}, "ldr >= F"), ({"ldo": 7}, "ldo >= F"),
            ({"recon": None, "orig": None}, "recon || orig"),
            ({"recon": odd}, "recon"), ({"orig": odd}, "orig"),
            ({"orig": None, "comparisons": 1}, "comparisons"),
            ({"recon": None, "comparisons": 1}, "comparisons"),
            ({"workspace": None}, "workspace"),
            ({"nbytes": need - 1}, "workspace_bytes"),
            ({"rows": 1 << 62, "ldr": 1 << 20}, "rows <=")):
        assert accumulate(**arguments) == -1, arguments
        message = lib.scvae_last_error().decode()
        assert "bad argument" in message and names in message, message
    assert lib.scvae_summary_accumulate(p, 8, p, 8, 4, 8, float("nan"), 0, p,
                                        need, None) == -1
    assert "tolerance" in lib.scvae_last_error().decode()
    assert lib.scvae_summary_reset(None, need, None) == -1
    assert lib.scvae_summary_reset(p, need - 1, None) == -1
    assert "workspace_bytes" in lib.scvae_last_error().decode()
    assert lib.scvae_summary_finish(p, need, None, p, None) == -1
    assert "stats" in lib.scvae_last_error().decode()
    assert lib.scvae_summary_finish(p, need, p, None, None) == -1
    assert lib.scvae_summary_finish(p, need - 1, p, p, None) == -1
    assert lib.scvae_summary_finish(None, need, p, p, None) == -1


def _tables():
    with open(os.path.join(ROOT, "tests", "golden",
                           "summary_tables.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("title", ["extensive", "single", "long name",
                                   "custom heading", "zeros"])
def test_table_is_the_reference_text(title):
    """Against what the reference's own ``format_summary_statistics``
    returned (``tests/golden/make_summary_fixtures.py``)."""
    from scvae_amd.analyses.summary import format_summary_statistics
    case = _tables()[title]
    keyword_arguments = {"name": case["name"]} if "name" in case else {}
    assert format_summary_statistics(
        case["sets"], **keyword_arguments) == case["table"]


def test_fixture_covers_what_it_claims():
    tables = _tables()
    assert isinstance(tables["single"]["sets"], dict)
    assert isinstance(tables["extensive"]["sets"], list)
    assert math.isnan(tables["extensive"]["sets"][2]["sparsity"])
    assert "nan" in tables["extensive"]["table"].splitlines()[3]
    assert max(len(s["name"]) for s in tables["long name"]["sets"]) > len(
        "Data set")
    assert tables["custom heading"]["table"].startswith(
        "Evaluation sets of the model")
    assert math.isnan(tables["zeros"]["sets"][0]["dispersion"])


def test_statistics_dictionary_follows_the_reference():
    from scvae_amd.analyses.summary import statistics_dictionary
    row = statistics_dictionary("x", 8, 2, 0.5, 2.0, -1.0, 3.0)
    assert list(row) == ["name", "mean", "standard deviation", "minimum",
                         "maximum", "dispersion", "sparsity"]
    assert row["dispersion"] == 8.0 and row["sparsity"] == 0.75
    assert math.isnan(statistics_dictionary(
        "x", 8, 2, 0.5, 2.0, -1.0, 3.0, skip_sparsity=True)["sparsity"])
    zeros = statistics_dictionary("x", 8, 0, 0.0, 0.0, 0.0, 0.0)
    assert math.isnan(zeros["dispersion"]) and zeros["sparsity"] == 1.0


def test_argument_errors_come_before_the_device(monkeypatch):
    import scipy.sparse
    import torch
    from scvae_amd.analyses import summary

    def never(*arguments, **keyword_arguments):
        raise AssertionError("the device path was entered")
    monkeypatch.setattr(summary._lib, "load", never)
    monkeypatch.setattr(summary.torch.cuda, "is_available", never)
    x = numpy.ones((4, 3), dtype=numpy.float32)
    with pytest.raises(ValueError, match="no values"):
        summary.summary_statistics(numpy.zeros((0, 3)))
    with pytest.raises(ValueError, match="float32 tensor"):
        summary.summary_statistics(torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="tolerance"):
        summary.summary_statistics(x, tolerance=float("nan"))
    with pytest.raises(ValueError, match="one shape"):
        summary.comparison_statistics(x, numpy.ones((4, 4)))
    with pytest.raises(ValueError, match="one shape"):
        summary.comparison_statistics(numpy.ones(12), numpy.ones(12))
    with pytest.raises(ValueError, match="dense"):
        summary.comparison_statistics(x, scipy.sparse.csr_matrix(x))
    with pytest.raises(ValueError, match="Two names"):
        summary.comparison_statistics(x, x, names=("a",))
    with pytest.raises(ValueError, match="at least one row"):
        summary.comparison_statistics(x, x, row_block=0)
    with pytest.raises(ValueError, match="tolerance"):
        summary.comparison_statistics(x, x, tolerance=float("nan"))


def test_device_summary_refuses_to_run_without_gpu():
    import scipy.sparse
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scvae_amd import _lib, analyses
    x = numpy.ones((4, 3), dtype=numpy.float32)
    for call in (lambda: analyses.summary_statistics(x),
                 lambda: analyses.summary_statistics(
                     scipy.sparse.csr_matrix(x)),
                 lambda: analyses.comparison_statistics(x, x),
                 lambda: analyses.comparison_statistics(
                     x, x, extensive=True)):
        with pytest.raises(_lib.HipLibraryError, match="no CPU path") as info:
            call()
        assert "No GPU visible" in str(info.value)
        assert "summary statistics" in str(info.value)


def test_evaluate_help_lists_both_flags(capsys):
    from scvae_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["evaluate", "--help"])
    out = capsys.readouterr().out
    assert "--summary-statistics" in out
    assert "--analysis-level {limited,normal,extensive}" in out


def test_flags_parse_and_reach_evaluate(monkeypatch):
    from scvae_amd import cli
    from scvae_amd.defaults import defaults
    seen = []
    monkeypatch.setattr(cli, "evaluate", lambda **kw: seen.append(kw) or 0)
    cli.main(["evaluate", "some_data"])
    cli.main(["evaluate", "some_data", "--summary-statistics"])
    cli.main(["evaluate", "some_data", "--summary-statistics",
              "--analysis-level", "extensive"])
    assert [kw["summary_statistics"] for kw in seen] == [False, True, True]
    assert [kw["analysis_level"] for kw in seen] == [
        defaults["analyses"]["analysis_level"], "normal", "extensive"]
    with pytest.raises(SystemExit):
        cli.main(["evaluate", "some_data", "--analysis-level", "everything"])


class _Set:
    kind = "test"
    version = "original"
    has_labels = False
    number_of_examples = 5
    number_of_features = 3
    number_of_batches = None
    has_batches = False


ROWS = [
    {"name": "original", "mean": 0.5, "standard deviation": 1.5,
     "minimum": 0.0, "maximum": 9.0, "dispersion": 4.5, "sparsity": 0.8},
    {"name": "reconstructed", "mean": 0.25, "standard deviation": 1.0,
     "minimum": 1e-3, "maximum": 7.5, "dispersion": 4.0, "sparsity": 0.9}]
EXTRA = [
    {"name": "differences", "mean": 0.3, "standard deviation": 0.5,
     "minimum": 0.0, "maximum": 4.0, "dispersion": 0.25 / 0.3,
     "sparsity": float("nan")},
    {"name": "log-ratios", "mean": 0.1, "standard deviation": 0.2,
     "minimum": 0.0, "maximum": 1.0, "dispersion": 0.4,
     "sparsity": float("nan")}]


def _run_evaluate(monkeypatch, capsys, device_calls, **switches):
    """``cli.evaluate`` over a model whose ``evaluate`` is the part of
    ``ModelBase.evaluate`` this is about: it prints the loss line, and asks
    the device function for the rows only when told to."""
    from scvae_amd import cli
    from scvae_amd.analyses import summary

    def device(csr, reconstructed, names, extensive=False, **rest):
        device_calls.append((names, extensive))
        return ROWS + (EXTRA if extensive else [])
    monkeypatch.setattr(summary, "evaluation_statistics", device)
    received = []

    class Model:
        description = "A model."

        def has_been_trained(self, run_id=None):
            return True

        def evaluate(self, **keyword_arguments):
            received.append(keyword_arguments)
            print("    Test set (0s):  ELBO: -1.")
            reconstructed = _Set()
            level = keyword_arguments.get("summary_statistics")
            if level:
                reconstructed.summary_statistics = (
                    summary.evaluation_statistics(
                        None, None, names=("original", "reconstructed"),
                        extensive=level == "extensive"))
                reconstructed.summary_statistics_duration = 0.25
            return [_Set(), reconstructed, {"z": _Set()}]
    data_set = _Set()
    monkeypatch.setattr(
        cli, "_load_data",
        lambda *a, **kw: (data_set, (data_set, None, data_set), None, None))
    monkeypatch.setattr(cli, "build_directory_path", lambda *a, **kw: "x")
    monkeypatch.setattr(cli, "indices_for_evaluation_subset",
                        lambda data_set: set())
    monkeypatch.setattr(cli, "_setup_model", lambda **kw: Model())
    capsys.readouterr()
    cli.evaluate("some_data", sample_size=0,
                 model_versions=["end_of_training"], **switches)
    return received, capsys.readouterr().out


def test_a_set_without_rows_prints_nothing(capsys):
    """A rank other than 0 of a data-parallel run: ``evaluate`` attached
    nothing to its reconstructed set."""
    from scvae_amd import cli
    cli._print_summary_statistics(_Set())
    assert capsys.readouterr().out == ""
    with_rows = _Set()
    with_rows.summary_statistics = ROWS
    cli._print_summary_statistics(with_rows)
    assert capsys.readouterr().out.splitlines()[0] == (
        "Calculating metrics for results.")


def test_switch_reaches_the_model_and_prints_the_table(monkeypatch, capsys):
    from scvae_amd.analyses.summary import format_summary_statistics
    calls = []
    received, plain = _run_evaluate(monkeypatch, capsys, calls)
    assert not calls and "summary_statistics" not in received[0]
    assert "metrics" not in plain.lower() and "Data set" not in plain
    # switched off explicitly, and a level without the switch: the same text
    for switches in ({"summary_statistics": False},
                     {"analysis_level": "extensive"}):
        received, out = _run_evaluate(monkeypatch, capsys, calls, **switches)
        assert out == plain and not calls
        assert "summary_statistics" not in received[0]

    received, out = _run_evaluate(monkeypatch, capsys, calls,
                                  summary_statistics=True)
    assert received[0]["summary_statistics"] == "normal"
    assert calls == [(("original", "reconstructed"), False)]
    lines, before = out.splitlines(), plain.splitlines()
    at = lines.index("    Test set (0s):  ELBO: -1.")
    table = format_summary_statistics(ROWS).splitlines()
    assert lines[at + 1:at + 4 + len(table)] == [
        "Calculating metrics for results.", "Metrics calculated (250 ms).",
        ""] + table
    assert len(table) == 3 and table[1].startswith("original ")
    # nothing else changed
    assert lines[:at + 1] + lines[at + 4 + len(table):] == before

    del calls[:]
    for level in ("limited", "normal"):
        received, again = _run_evaluate(
            monkeypatch, capsys, calls, summary_statistics=True,
            analysis_level=level)
        assert again == out and received[0]["summary_statistics"] == "normal"
    del calls[:]
    received, out = _run_evaluate(monkeypatch, capsys, calls,
                                  summary_statistics=True,
                                  analysis_level="extensive")
    assert received[0]["summary_statistics"] == "extensive"
    assert calls == [(("original", "reconstructed"), True)]
    lines = out.splitlines()
    at = lines.index("Metrics calculated (250 ms).")
    assert lines[at + 2:at + 7] == format_summary_statistics(
        ROWS + EXTRA).splitlines()
    assert lines[at + 5].startswith("differences ")
    assert lines[at + 6].startswith("log-ratios ")
    with pytest.raises(ValueError, match="Analysis level `all` not found"):
        _run_evaluate(monkeypatch, capsys, calls, summary_statistics=True,
                      analysis_level="all")
