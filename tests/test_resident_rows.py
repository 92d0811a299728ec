"""The resident training set, host side: the C ABI declares and exports the
row-index field and entries, and ``scvae train --resident-training-set``
reaches ``model.train`` (no GPU needed)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scvae_hip.h")


def _header():
    with open(HEADER) as stream:
        return stream.read()


def _struct_fields(text, name):
    body = re.search(r"typedef struct {0} \{{(.*?)\}} {0};".format(name), text,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*(\[[^\]]*\])?$", d.strip()).group(1)
            for d in body.split(";") if d.strip()]


def test_header_declares_the_row_index_entries():
    text = _header()
    assert re.search(
        r"int32_t\s+scvae_plan_accepts_counts_rows\(const scvae_plan\*[^)]*"
        r"int64_t cells,\s*int32_t training\);", text)
    assert re.search(
        r"int\s+scvae_gather_rows_u16\(const uint16_t\* src, int64_t ld_src,\s*"
        r"const int64_t\* rows, int64_t n,\s*int64_t cols, uint16_t\* out, "
        r"int64_t ld_out,\s*void\* stream\);", text)


def test_counts_rows_is_the_last_field_of_the_step_arguments():
    from scvae_amd import _lib
    fields = _struct_fields(_header(), "scvae_step_args")
    assert fields[-1] == "counts_rows"
    mirror = [name for name, _ in _lib.StepArgs._fields_]
    assert mirror[-1] == "counts_rows"
    assert mirror == fields
    # appended: every earlier field where it was
    assert fields[-2] == "side"
    assert _lib.StepArgs.counts_rows.offset == (
        _lib.StepArgs.side.offset + ctypes.sizeof(ctypes.c_void_p))
    assert ctypes.sizeof(_lib.StepArgs) == (
        _lib.StepArgs.counts_rows.offset + ctypes.sizeof(ctypes.c_void_p))


def test_library_exports_the_row_index_entries():
    from scvae_amd import _lib
    if not os.path.exists(_lib.LIBRARY_PATH):
        pytest.fail("libscvae_hip.so has not been built")
    # (no GPU needed to look a symbol up)
    lib = ctypes.CDLL(_lib.LIBRARY_PATH)
    for name in ("scvae_plan_accepts_counts_rows", "scvae_gather_rows_u16"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    accepts = lib.scvae_plan_accepts_counts_rows
    accepts.restype = ctypes.c_int32
    accepts.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]
    assert accepts(None, 4096, 1) == 0          # no plan: nothing is accepted


def _train_keywords(monkeypatch, extra):
    """What ``scvae train some-data-set <extra>`` hands to ``model.train``."""
    from scvae_amd import cli
    seen = {}

    class Model:
        description = parameters = ""

        def train(self, *args, **kwargs):
            seen.update(kwargs)
            return 0

    class Set:
        has_labels = False

    monkeypatch.setattr(
        cli, "_load_data",
        lambda *a, **k: (Set(), (Set(), None, None), "default", 0.9))
    monkeypatch.setattr(cli, "_setup_model", lambda **k: Model())
    monkeypatch.setattr(cli, "build_directory_path", lambda *a, **k: "unused")
    assert cli.main(["train", "some-data-set"] + extra) == 0
    return seen


def test_flag_reaches_model_train(monkeypatch):
    seen = _train_keywords(monkeypatch, ["--resident-training-set"])
    assert seen["resident_training_set"] is True


def test_flag_defaults_to_off(monkeypatch):
    seen = _train_keywords(monkeypatch, [])
    assert seen["resident_training_set"] is False


def test_model_train_takes_the_keyword_and_defaults_to_off():
    from scvae_amd.models.base import ModelBase
    parameter = inspect.signature(ModelBase.train).parameters[
        "resident_training_set"]
    assert parameter.default is False
