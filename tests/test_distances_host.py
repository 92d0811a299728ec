"""``scvae_amd/analyses/distances.py`` without a GPU: the exports, the
hierarchical order, the loop of ``analyse_matrices`` on the host path, the
oracle of the GPU tests against scikit-learn, and the files."""
import os
import re

import numpy
import pytest
import scipy.cluster.hierarchy
import scipy.spatial.distance
import sklearn.metrics

import _distances_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_bindings():
    from scvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "scvae_hip.h")).read()
    for name, arguments in (("scvae_pairwise_distances_workspace_bytes", 2),
                            ("scvae_pairwise_distances", 12)):
        assert re.search(r"\b{}\(".format(name), header), name
        assert len(_lib.SIGNATURES[name][1]) == arguments
    assert "matrices.py:124-130" in header
    assert "subanalyses.py:294-468" in header
    lib = _lib.load()
    for name in ("scvae_pairwise_distances_workspace_bytes",
                 "scvae_pairwise_distances"):
        assert hasattr(lib, name), name
    assert lib.scvae_pairwise_distances_workspace_bytes(1000, 32738) >= 8000
    for n, features in ((0, 5), (2 ** 16 + 1, 5), (5, 0), (5, 2 ** 20 + 1)):
        assert lib.scvae_pairwise_distances_workspace_bytes(n, features) == -1
        assert b"bad argument" in lib.scvae_last_error()
    assert lib.scvae_pairwise_distances_workspace_bytes(2 ** 16, 2 ** 20) > 0
    # no pointer is touched before the arguments are checked
    assert lib.scvae_pairwise_distances(
        None, 5, 5, 5, None, 5, 0, None, 5, None, 0, None) == -1
    assert b"bad argument" in lib.scvae_last_error()


def test_public_names():
    import scvae_amd.analyses as analyses
    for name in ("pairwise_distances", "hierarchical_order",
                 "distance_matrices", "evaluation_distances",
                 "write_distances"):
        assert callable(getattr(analyses, name)), name


def _points(n, features, seed):
    rng = numpy.random.default_rng(seed)
    return rng.standard_normal((n, features)).astype(numpy.float32)


def test_hierarchical_order_is_single_linkage():
    from scvae_amd.analyses.distances import hierarchical_order
    orders_differ = False
    for n, seed in ((2, 0), (3, 1), (40, 2), (200, 3)):
        # (fp64 points: 19 900 fp32 distances would hold ties)
        distances = sklearn.metrics.pairwise_distances(
            _points(n, 5, seed).astype(numpy.float64))
        condensed = scipy.spatial.distance.squareform(distances, checks=False)
        assert numpy.unique(condensed).size == condensed.size    # no ties
        single = scipy.cluster.hierarchy.dendrogram(
            scipy.cluster.hierarchy.linkage(condensed, method="single"),
            no_plot=True)["leaves"]
        got = hierarchical_order(distances)
        assert got.dtype == numpy.int64
        assert got.tolist() == single
        # what the reference writes, and what SciPy makes of it
        reference = scipy.cluster.hierarchy.dendrogram(
            scipy.cluster.hierarchy.linkage(condensed, metric="average"),
            no_plot=True)["leaves"]
        assert got.tolist() == reference
        average = scipy.cluster.hierarchy.dendrogram(
            scipy.cluster.hierarchy.linkage(condensed, method="average"),
            no_plot=True)["leaves"]
        orders_differ = orders_differ or average != single
    assert orders_differ
    assert hierarchical_order(numpy.zeros((1, 1))).tolist() == [0]


def test_hierarchical_order_differs_from_average_linkage():
    """A chain 0 - 1 - 2 - 3 with growing gaps and a far pair: single linkage
    joins along the chain, average linkage pairs up differently."""
    from scvae_amd.analyses.distances import hierarchical_order
    positions = numpy.array([0.0, 1.0, 2.1, 3.3, 4.6, 6.0, 20.0, 21.5])
    rng = numpy.random.default_rng(5)
    positions = positions[rng.permutation(positions.size)]
    distances = numpy.abs(positions[:, None] - positions[None, :])
    condensed = scipy.spatial.distance.squareform(distances, checks=False)
    single = scipy.cluster.hierarchy.leaves_list(
        scipy.cluster.hierarchy.linkage(condensed, method="single"))
    average = scipy.cluster.hierarchy.leaves_list(
        scipy.cluster.hierarchy.linkage(condensed, method="average"))
    assert single.tolist() != average.tolist()
    assert hierarchical_order(distances).tolist() == single.tolist()


@pytest.mark.parametrize("n", [999, 1000, 1001, 10001])
def test_sample_sizes_and_indices(n):
    from scvae_amd.analyses.distances import distance_matrices
    rng = numpy.random.default_rng(n)
    values = rng.standard_normal((n, 2)).astype(numpy.float32)
    labels = rng.integers(0, 4, n).astype(str)
    matrices = distance_matrices(values, labels=labels, version="z",
                                 on_device=False)
    assert [(m["sorting_method"], m["metric"]) for m in matrices] == [
        ("labels", "Euclidean"), ("labels", "cosine"),
        ("hierarchical_clustering", "Euclidean"),
        ("hierarchical_clustering", "cosine")]
    shuffled = numpy.random.RandomState(57).permutation(n)
    for matrix in matrices:
        by_labels = matrix["sorting_method"] == "labels"
        limit = 10000 if by_labels else 1000
        sample = shuffled[:limit] if n > limit else numpy.arange(n)
        assert matrix["sample_size"] == (limit if n > limit else None)
        indices = matrix["indices"]
        assert indices.dtype == numpy.int64
        assert sorted(indices.tolist()) == sorted(sample.tolist())
        assert matrix["distances"].shape == (sample.size, sample.size)
        assert matrix["distances"].dtype == numpy.float32
        assert matrix["duration"] >= 0
        if by_labels:     # the stable order of the sample's labels
            assert indices.tolist() == sample[numpy.argsort(
                labels[sample], kind="stable")].tolist()
        if n == 1001 or by_labels and n == 999:
            # the matrix is that of the rows in plotted order
            want = sklearn.metrics.pairwise_distances(
                values[indices], metric=matrix["metric"].lower())
            assert numpy.array_equal(matrix["distances"],
                                     want.astype(numpy.float32))


def test_loop_order_names_and_hierarchical_permutation():
    from scvae_amd.analyses.distances import (
        distance_matrices, hierarchical_order)
    values = _points(60, 7, 11)
    without = distance_matrices(values, version="reconstructed",
                                on_device=False)
    assert [m["name"] for m in without] == [
        "distances-reconstructed-euclidean-hierarchical_clustering",
        "distances-reconstructed-cosine-hierarchical_clustering"]
    labels = numpy.array(["b", "a", "c"])[numpy.arange(60) % 3]
    with_labels = distance_matrices(values, labels=labels, version="z",
                                    on_device=False)
    assert [m["name"] for m in with_labels] == [
        "distances-z-euclidean-labels", "distances-z-cosine-labels",
        "distances-z-euclidean-hierarchical_clustering",
        "distances-z-cosine-hierarchical_clustering"]
    # stable: inside a class the examples keep their order
    indices = with_labels[0]["indices"]
    assert indices.tolist() == (list(range(1, 60, 3)) + list(range(0, 60, 3))
                                + list(range(2, 60, 3)))
    for matrix in without:
        unsorted = sklearn.metrics.pairwise_distances(
            values, metric=matrix["metric"].lower()).astype(numpy.float32)
        order = hierarchical_order(unsorted)
        assert matrix["indices"].tolist() == order.tolist()
        assert numpy.array_equal(matrix["distances"],
                                 unsorted[order][:, order])
        assert matrix["sample_size"] is None
    with pytest.raises(ValueError, match="not found"):
        from scvae_amd.analyses.distances import pairwise_distances
        pairwise_distances(values, metric="manhattan", on_device=False)
    with pytest.raises(IndexError):
        pairwise_distances(values, rows=[0, 60], on_device=False)


def test_oracle_agrees_with_scikit_learn():
    """scikit-learn's expanded form on fp32 input: its error is that of the
    same formula with the unit roundoff of fp32 at worst."""
    rng = numpy.random.default_rng(3)
    x = (rng.poisson(3.0, (50, 33)) * rng.random((50, 33))
         * (rng.random((50, 33)) < 0.5)).astype(numpy.float32)
    x[7] = 0
    x[9] = x[4]
    for metric, reference, bound in (
            ("euclidean", oracle.euclidean_oracle, oracle.euclidean_bound),
            ("cosine", oracle.cosine_oracle, oracle.cosine_bound)):
        want = reference(x)
        theirs = sklearn.metrics.pairwise_distances(x, metric=metric)
        allowed = bound(x, want, u=oracle.U32)
        assert numpy.all(numpy.abs(theirs - want) <= allowed), metric
        assert numpy.all(numpy.diag(want) == 0)
        assert want[9, 4] <= 1e-15 and numpy.array_equal(want, want.T)
    assert numpy.all(numpy.delete(oracle.cosine_oracle(x)[7], 7) == 1.0)
    # the bound of the fp64 kernel is tight enough to tell fp32 arithmetic
    assert numpy.median(oracle.euclidean_bound(x, oracle.euclidean_oracle(x))
                        / numpy.maximum(oracle.euclidean_oracle(x), 1e-30)
                        ) < 2 ** -23


def test_write_distances_round_trip(tmp_path):
    from scvae_amd.analyses.distances import (
        evaluation_distances, write_distances)
    values = _points(30, 4, 2)
    names = numpy.array(["cell {}".format(i) for i in range(30)])
    labels = numpy.array(["x", "y"])[numpy.arange(30) % 2]
    result = evaluation_distances(values, latent_z=values[:, :2],
                                  labels=labels, example_names=names,
                                  on_device=False)
    assert sorted(result) == ["reconstructed", "z"]
    assert len(result["reconstructed"]) == len(result["z"]) == 4
    directory = str(tmp_path / "deep" / "distances")
    for matrix in result["reconstructed"] + result["z"]:
        matrix_path, table_path = write_distances(directory, matrix)
        assert os.path.basename(matrix_path) == matrix["name"] + ".npy"
        assert os.path.basename(table_path) == matrix["name"] + ".tsv"
        back = numpy.load(matrix_path)
        assert back.dtype == numpy.float32
        assert numpy.array_equal(back, matrix["distances"])
        rows = [line.split("\t")
                for line in open(table_path).read().splitlines()]
        assert rows[0] == ["position", "index", "example", "label"]
        assert [int(r[0]) for r in rows[1:]] == list(range(30))
        assert [int(r[1]) for r in rows[1:]] == matrix["indices"].tolist()
        assert [r[2] for r in rows[1:]] == names[matrix["indices"]].tolist()
        assert [r[3] for r in rows[1:]] == labels[matrix["indices"]].tolist()
    unlabelled = evaluation_distances(values, on_device=False)
    assert sorted(unlabelled) == ["reconstructed"]
    _, table_path = write_distances(directory, unlabelled["reconstructed"][0])
    assert open(table_path).readline() == "position\tindex\texample\n"
