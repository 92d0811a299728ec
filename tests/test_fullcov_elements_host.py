"""tests/_fullcov_elements_oracle.py on the host: its fp64 closed forms pinned to
``_fullcov_oracle.latent_pair`` + autograd, the plain NumPy fp32 evaluation of
the kernels' formulation taken through the SAME ``hold`` on the SAME cases as
tests/test_gpu_fullcov_elements.py (a correct fp32 implementation meets every
derived bound), and the bounds shown to discriminate: each listed mutation of
the fp32 evaluation is rejected by at least one element."""
import numpy as np
import pytest

import _fullcov_elements_oracle as eo

RUN = eo.Fp32Evaluation()
OTHER_CASES = [c for c in eo.CASES if c[0] != "dominant"]


@pytest.fixture(scope="module")
def report():
    """(row, output) -> largest err / bound; printed when the module is done."""
    table = {}
    yield table
    eo.print_table(table, "the host fp32 evaluation")


@pytest.mark.parametrize("L", eo.GEOMETRY_L)
def test_fp32_geometry(report, L):
    for case in eo.CASES:
        if case[0] == "dominant" and case[4] == L:
            eo.check_pair(RUN, *case, report)


@pytest.mark.parametrize("case", OTHER_CASES, ids=lambda c: "{}-L{}".format(c[0], c[4]))
def test_fp32_probes_conditioning_and_clip(report, case):
    eo.check_pair(RUN, *case, report)


@pytest.mark.parametrize("K,L", eo.PRIOR_STATS_CASES)
def test_fp32_prior_stats(report, K, L):
    eo.check_prior_stats(RUN, K, L, report)


def test_fp32_prior_stats_clip(report):
    eo.check_prior_stats(RUN, eo.CLIP_SHAPE[0], eo.CLIP_SHAPE[3], report, kind="clip")


@pytest.mark.parametrize("case", [("dense", 2, 1, 5, 25), ("dominant", 3, 3, 7, 3),
                                  ("dominant", 1, 3, 7, 33), ("unit-u", 1, 1, 4, 1),
                                  ("clip",) + eo.CLIP_SHAPE, ("clip-overflow",) + eo.CLIP_SHAPE],
                         ids=lambda c: "{}-L{}".format(c[0], c[4]))
def test_closed_forms_are_latent_pair_and_autograd(case):
    """Every output, to fp64 rounding times the conditioning of the case (the
    dense triangles at L = 25 have a condition number of 1e3)."""
    kind, shape = case[0], case[1:]
    arrays = eo.inputs(kind, *shape)
    want = eo.autograd_pair(arrays, *shape)
    got, info = eo.pair(arrays, *shape)
    for name in eo.OUTPUTS:
        g = np.asarray(got[name].value).reshape(want[name].shape)
        # against the sum of term magnitudes, element by element
        mag = np.asarray(got[name].mag).reshape(want[name].shape)
        err = np.abs(g - want[name])
        assert (err <= 1e-12 * info["cond"].max() * (mag + 1e-300) + 1e-300).all(), \
            (name, float((err / (mag + 1e-300)).max()))
    # and the bounds are far above that: the comparison above is not what holds them
    assert (got["klz"].bound > 1e-9 * got["klz"].mag).all()


MUTATION_CASES = {
    "drop-last-logdet": [("logdet", 3, 1, 2, 64)],
    "half-wave-sum": [("logdet", 3, 1, 2, 33)],
    "swap-fill-sources": [("onehot", 1, 1, 6, 6)],
    "diagonal-with-P": [("dominant", 1, 3, 7, 25), ("dense", 2, 1, 5, 25)],
    "qcov-to-max": [("dense", 2, 1, 5, 25)],
    "skip-last-sample-in-GA": [("dominant", 1, 3, 7, 25)],
}


@pytest.mark.parametrize("mutation", eo.MUTATIONS)
def test_bounds_reject_mutation(mutation):
    """The unmutated evaluation passes these cases (above); the mutated one must
    have an element outside its bound in at least one of them."""
    rejected = []
    for case in MUTATION_CASES[mutation]:
        assert case in eo.CASES
        try:
            eo.check_pair(eo.Fp32Evaluation(mutation), *case, {})
        except AssertionError as e:
            rejected.append((case, str(e).splitlines()[0]))
    print(rejected)
    assert rejected, mutation


def test_product_with_zero_derivative_is_nan_where_the_quotient_overflows():
    """What the backward kernel did before it selected the zero: sum_s g / FLT_MIN
    overflows at (k, b) = (1, 4) of the clip-overflow case and inf * 0 is NaN; with
    |sum_s g| <= 1, as a step passes it, the product is a clean 0."""
    K, S, B, L = eo.CLIP_SHAPE
    for kind, nan in (("clip", False), ("clip-overflow", True)):
        arrays = eo.inputs(kind, K, S, B, L)
        before = eo.sim_pair(arrays, K, S, B, L, select_clipped=False)
        after = eo.sim_pair(arrays, K, S, B, L)
        old, new = before["dqsc"], after["dqsc"]
        assert np.isnan(old[1 * B + 4, 0]) == nan
        assert np.isfinite(new).all() and np.isnan(old).sum() == int(nan)
        # the same bits wherever the clip does not hold; +0 where it does
        info = eo.pair(arrays, K, S, B, L)[1]
        clipped = {"dqsc": info["clip_q"],
                   "dprior": np.concatenate([np.zeros((K * B, L), dtype=bool),
                                             np.repeat(info["clip_p"], B, axis=0)], axis=1)}
        for name in eo.OUTPUTS:
            o, n = before[name].view(np.uint32), after[name].view(np.uint32)
            c = clipped.get(name, np.zeros(o.shape, dtype=bool)).reshape(o.shape)
            assert (o[~c] == n[~c]).all() and (n[c] == 0).all(), name
