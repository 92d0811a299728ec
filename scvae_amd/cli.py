"""Command-line interface: ``scvae train`` / ``scvae evaluate`` with the flag
names and defaults of the reference (``scvae/cli.py:698-1239``); the Python
functions ``train`` and ``evaluate`` keep the reference's call order
(``cli.py:111-264, 267-566``): data set -> (split) -> model directory ->
model -> ``model.train`` / ``model.evaluate``.

The ``analyse`` / ``cross-analyse`` commands and the plotting analyses
(``scvae/analyses``) are CPU post-processing outside the built hot path; the
flags that only feed them are accepted and ignored with a notice.
"""

import argparse
import contextlib
import os

from scvae_amd import __version__
from scvae_amd.data import DataSet
from scvae_amd.data.utilities import (
    build_directory_path, indices_for_evaluation_subset)
from scvae_amd.defaults import defaults
from scvae_amd.models import (
    GaussianMixtureVariationalAutoencoder, VariationalAutoencoder)
from scvae_amd.models.utilities import (
    better_model_exists, model_stopped_early)
from scvae_amd.utilities import (
    capitalise_string, format_duration, normalise_string, subtitle, title)


def _setup_model(data_set, model_type=None, latent_size=None,
                 hidden_sizes=None, number_of_importance_samples=None,
                 number_of_monte_carlo_samples=None,
                 inference_architecture=None, latent_distribution=None,
                 number_of_classes=None, parameterise_latent_posterior=False,
                 prior_probabilities_method=None, generative_architecture=None,
                 reconstruction_distribution=None,
                 number_of_reconstruction_classes=None, count_sum=None,
                 proportion_of_free_nats_for_y_kl_divergence=None,
                 minibatch_normalisation=None, batch_correction=None,
                 dropout_keep_probabilities=None,
                 number_of_warm_up_epochs=None, kl_weight=None,
                 models_directory=None):
    """Model factory (``cli.py:601-689``)."""
    if model_type is None:
        model_type = defaults["models"]["type"]
    if batch_correction is None:
        batch_correction = defaults["models"]["batch_correction"]
    feature_size = data_set.number_of_features
    number_of_batches = data_set.number_of_batches
    if not data_set.has_batches:
        batch_correction = False

    if normalise_string(model_type) == "vae":
        return VariationalAutoencoder(
            feature_size=feature_size, latent_size=latent_size,
            hidden_sizes=hidden_sizes,
            number_of_monte_carlo_samples=number_of_monte_carlo_samples,
            number_of_importance_samples=number_of_importance_samples,
            inference_architecture=inference_architecture,
            latent_distribution=latent_distribution,
            number_of_latent_clusters=number_of_classes,
            parameterise_latent_posterior=parameterise_latent_posterior,
            generative_architecture=generative_architecture,
            reconstruction_distribution=reconstruction_distribution,
            number_of_reconstruction_classes=number_of_reconstruction_classes,
            minibatch_normalisation=minibatch_normalisation,
            batch_correction=batch_correction,
            number_of_batches=number_of_batches,
            dropout_keep_probabilities=dropout_keep_probabilities,
            count_sum=count_sum,
            number_of_warm_up_epochs=number_of_warm_up_epochs,
            kl_weight=kl_weight, log_directory=models_directory)
    if normalise_string(model_type) == "gmvae":
        prior_probabilities = None
        method = prior_probabilities_method
        if prior_probabilities_method == "infer":
            method = "custom"
            prior_probabilities = getattr(
                data_set, "class_probabilities", None)
        return GaussianMixtureVariationalAutoencoder(
            feature_size=feature_size, latent_size=latent_size,
            hidden_sizes=hidden_sizes,
            number_of_monte_carlo_samples=number_of_monte_carlo_samples,
            number_of_importance_samples=number_of_importance_samples,
            prior_probabilities_method=method,
            prior_probabilities=prior_probabilities,
            latent_distribution=latent_distribution,
            number_of_latent_clusters=number_of_classes,
            proportion_of_free_nats_for_y_kl_divergence=(
                proportion_of_free_nats_for_y_kl_divergence),
            reconstruction_distribution=reconstruction_distribution,
            number_of_reconstruction_classes=number_of_reconstruction_classes,
            minibatch_normalisation=minibatch_normalisation,
            batch_correction=batch_correction,
            number_of_batches=number_of_batches,
            dropout_keep_probabilities=dropout_keep_probabilities,
            count_sum=count_sum,
            number_of_warm_up_epochs=number_of_warm_up_epochs,
            kl_weight=kl_weight, log_directory=models_directory)
    raise ValueError("Model type not found: `{}`.".format(model_type))


def _model_arguments(arguments):
    keys = (
        "model_type", "latent_size", "hidden_sizes",
        "number_of_importance_samples", "number_of_monte_carlo_samples",
        "inference_architecture", "latent_distribution", "number_of_classes",
        "parameterise_latent_posterior", "prior_probabilities_method",
        "generative_architecture", "reconstruction_distribution",
        "number_of_reconstruction_classes", "count_sum",
        "proportion_of_free_nats_for_y_kl_divergence",
        "minibatch_normalisation", "batch_correction",
        "dropout_keep_probabilities", "number_of_warm_up_epochs", "kl_weight")
    return {k: arguments.get(k) for k in keys}


def _load_data(data_set_file_or_name, data_format, data_directory,
               preprocessing_methods, noisy_preprocessing_methods,
               split_data_set, splitting_method, splitting_fraction,
               binarise_values=False, feature_selection=None,
               example_filter=None):
    data_set = DataSet(
        data_set_file_or_name, data_format=data_format,
        directory=data_directory,
        feature_selection=feature_selection,
        example_filter=example_filter,
        preprocessing_methods=preprocessing_methods,
        noisy_preprocessing_methods=noisy_preprocessing_methods)
    if binarise_values:   # targets of the Bernoulli likelihood (cli.py:144-160)
        data_set.load()
        data_set.binarise()
    if split_data_set:
        subsets = data_set.split(method=splitting_method,
                                 fraction=splitting_fraction)
    else:
        data_set.load()
        splitting_method = splitting_fraction = None
        subsets = (data_set, None, data_set)
    return data_set, subsets, splitting_method, splitting_fraction


def train(data_set_file_or_name, data_format=None, data_directory=None,
          feature_selection=None, example_filter=None,
          preprocessing_methods=None, noisy_preprocessing_methods=None,
          split_data_set=None, splitting_method=None, splitting_fraction=None,
          number_of_epochs=None, minibatch_size=None, learning_rate=None,
          run_id=None, new_run=False, reset_training=None,
          models_directory=None, caches_directory=None,
          analyses_directory=None, deterministic=False,
          resident_training_set=False, **keyword_arguments):
    """Train model on data set (``cli.py:111-264``).  ``deterministic`` (not in
    the reference): bit-repeatable accumulation of the decoder gradient.
    ``resident_training_set`` (not in the reference): keep the training set's
    dense uint16 rows on the device; steps read them through a row index."""
    if split_data_set is None:
        split_data_set = defaults["data"]["split_data_set"]
    if splitting_method is None:
        splitting_method = defaults["data"]["splitting_method"]
    if splitting_fraction is None:
        splitting_fraction = defaults["data"]["splitting_fraction"]
    if models_directory is None:
        models_directory = defaults["models"]["directory"]

    print(title("Data"))
    data_set, subsets, splitting_method, splitting_fraction = _load_data(
        data_set_file_or_name, data_format, data_directory,
        preprocessing_methods, noisy_preprocessing_methods, split_data_set,
        splitting_method, splitting_fraction,
        binarise_values=normalise_string(str(keyword_arguments.get(
            "reconstruction_distribution"))) == "bernoulli",
        feature_selection=feature_selection, example_filter=example_filter)
    training_set, validation_set, _ = subsets

    models_directory = build_directory_path(
        models_directory, data_set=data_set,
        splitting_method=splitting_method,
        splitting_fraction=splitting_fraction)
    model_caches_directory = None
    if caches_directory:
        model_caches_directory = build_directory_path(
            os.path.join(caches_directory, "log"), data_set=data_set,
            splitting_method=splitting_method,
            splitting_fraction=splitting_fraction)

    print(title("Model"))
    model_arguments = _model_arguments(keyword_arguments)
    if (model_arguments["number_of_classes"] is None
            and training_set.has_labels):
        model_arguments["number_of_classes"] = training_set.number_of_classes
    model = _setup_model(data_set=training_set,
                         models_directory=models_directory, **model_arguments)
    print(model.description)
    print()
    print(model.parameters)
    print()

    print(subtitle("Training"))
    if analyses_directory:
        print("Intermediate analyses (plots) are not part of this build; "
              "`--analyses-directory` is ignored.")
    model.train(
        training_set, validation_set, number_of_epochs=number_of_epochs,
        minibatch_size=minibatch_size, learning_rate=learning_rate,
        intermediate_analyser=None, run_id=run_id, new_run=new_run,
        reset_training=reset_training,
        temporary_log_directory=model_caches_directory,
        deterministic=deterministic,
        resident_training_set=bool(resident_training_set))
    return 0


def evaluate(data_set_file_or_name, data_format=None, data_directory=None,
             feature_selection=None, example_filter=None,
             preprocessing_methods=None, noisy_preprocessing_methods=None,
             split_data_set=None, splitting_method=None,
             splitting_fraction=None, minibatch_size=None, run_id=None,
             models_directory=None, evaluation_set_kind=None,
             sample_size=None, model_versions=None, prediction_method=None,
             prediction_training_set_kind=None, prediction_on_device=False,
             silhouette_score=False, silhouette_space="latent",
             summary_statistics=False, analysis_level=None,
             decompositions=False, decomposition_methods=None,
             latent_space=False, distributions=False, distances=False,
             analyses_directory=None, **keyword_arguments):
    """Evaluate model on data set (``cli.py:267-566``).

    ``decompositions`` (not in the reference's ``evaluate``, which leaves it
    to ``analyse_results``): after the evaluation of each model version the
    two-component PCA of the reconstructed set (``analyses.py:1237-1252``),
    fitted on the GPU on the reconstruction where it lies
    (``analyses/decomposition.py``); with ``analysis_level="extensive"`` also
    the reconstructions in the space of the originals
    (``analyses.py:1267-1280``).  The coordinates go to tab-separated files
    under ``analyses_directory``.  ``decomposition_methods`` (the reference's
    option): only ``pca`` is built.

    ``latent_space`` (not in the reference's ``evaluate``, which leaves it to
    ``analyse_results``): after the evaluation of each model version, the
    two-dimensional maps of every latent set with more than two features
    (``analyses.py:1405-1416``, ``subanalyses.py:595-673``), one for every
    method in ``decomposition_methods``: ``pca`` as above, ``t-SNE`` exact
    over every pair of cells on the GPU (``analyses/tsne.py``) where the
    reference fits the Barnes-Hut approximation on the host.  The coordinates
    go to tab-separated files under ``analyses_directory``.  With several
    ranks only rank 0 fits and writes (not tested on more than one GPU).

    ``distributions`` (not in the reference's ``evaluate``, which leaves it
    to ``analyse_results``): after the evaluation of each model version the
    histograms of its "Distributions" (``analyses.py:1226-1235``,
    ``subanalyses.py:50-291``) of the reconstructed set -- counts, counts
    shifted by one, and count sums -- computed on the GPU on the
    reconstruction where it lies (``analyses/distributions.py``); with
    ``analysis_level="extensive"`` also those of the evaluation set.  Each
    goes to a tab-separated file under ``analyses_directory``.

    ``distances`` (not in the reference's ``evaluate``, which leaves it to
    ``analyse_results``): after the evaluation of each model version the
    pairwise distance matrices of its "Distances" (``analyses.py:1351-1362``,
    ``subanalyses.py:294-468``) of the reconstructed set and of the ``z``
    latent values -- Euclidean and cosine, sorted by labels (where the set
    has labels) and by hierarchical clustering, over 10 000 and 1 000
    sampled examples at most -- computed on the GPU on the reconstruction
    where it lies (``analyses/distances.py``).  Each goes to a ``.npy`` file
    with a ``.tsv`` table of its examples under ``analyses_directory``; a
    matrix of 10 000 examples is 400 MB.

    ``summary_statistics`` (not in the reference's ``evaluate``, which leaves
    it to ``analyse_results``): after the evaluation of each model version
    print the metrics table of ``analyses/analyses.py:873-895, 1040`` -- mean,
    standard deviation, dispersion, minimum, maximum and sparsity of the
    evaluation set and of the reconstructed set -- computed on the GPU in one
    pass over the reconstruction where it lies (``analyses/summary.py``).
    ``analysis_level`` (the reference's option, read only with
    ``summary_statistics``): ``"extensive"`` adds the rows ``differences`` and
    ``log-ratios``.

    ``prediction_on_device`` (not in the reference): run the k-means of the
    prediction on the GPU (``analyses/kmeans.py``: exact Lloyd for every
    number of cells) instead of scikit-learn on the host.

    ``silhouette_score``: also print the silhouette score of the predicted
    clusters (and of the predicted labels), the third clustering metric of
    the reference (``analyses/metrics/clustering.py:120-142``), computed on
    the GPU (``analyses/silhouette.py``).  The reference scores the
    clustering in count space (cells x genes) and samples it down to 20 000
    cells; this scores it in the latent space the clustering was made in,
    exactly, over every cell.

    ``silhouette_space`` (read only with ``silhouette_score``): ``"latent"``,
    the above, or ``"counts"``, the reference's own quantity: the score over
    the values of the evaluation set in count space, 20 000 cells sampled
    above 20 000, with exact distances on the GPU
    (``analyses/count_silhouette.py``)."""
    silhouette_space = normalise_string(str(silhouette_space))
    if silhouette_score and silhouette_space not in ("latent", "counts"):
        raise ValueError("Silhouette space `{}` not found.".format(
            silhouette_space))
    summary_level = decomposition_level = distributions_level = None
    if summary_statistics or decompositions or distributions:
        if analysis_level is None:
            analysis_level = defaults["analyses"]["analysis_level"]
        analysis_level = normalise_string(str(analysis_level))
        if analysis_level not in ("limited", "normal", "extensive"):
            raise ValueError("Analysis level `{}` not found.".format(
                analysis_level))
        level = "extensive" if analysis_level == "extensive" else "normal"
        if summary_statistics:
            summary_level = level
        if decompositions:
            decomposition_level = level
        if distributions:
            distributions_level = level
    if (distributions_level or distances) and analyses_directory is None:
        analyses_directory = defaults["analyses"]["directory"]
    if decomposition_level or latent_space:
        from scvae_amd.analyses.decomposition import method_name
        if decomposition_methods is None:
            decomposition_methods = [
                defaults["analyses"]["decomposition_method"]]
        elif not isinstance(decomposition_methods, (list, tuple)):
            decomposition_methods = [decomposition_methods]
        decomposition_methods = [method_name(m) for m in decomposition_methods]
        if analyses_directory is None:
            analyses_directory = defaults["analyses"]["directory"]
    if prediction_method is None:
        prediction_method = defaults["evaluation"]["prediction_method"]
    if prediction_training_set_kind is None:
        prediction_training_set_kind = defaults["evaluation"][
            "prediction_training_set_kind"]
    prediction_training_set_kind = normalise_string(
        prediction_training_set_kind)
    if sample_size is None:
        sample_size = defaults["models"]["sample_size"]
    if split_data_set is None:
        split_data_set = defaults["data"]["split_data_set"]
    if splitting_method is None:
        splitting_method = defaults["data"]["splitting_method"]
    if splitting_fraction is None:
        splitting_fraction = defaults["data"]["splitting_fraction"]
    if models_directory is None:
        models_directory = defaults["models"]["directory"]
    if evaluation_set_kind is None:
        evaluation_set_kind = defaults["evaluation"]["data_set_kind"]
    if model_versions is None:
        model_versions = defaults["evaluation"]["model_versions"]
    if not isinstance(model_versions, list):
        model_versions = [model_versions]
    evaluation_set_kind = normalise_string(evaluation_set_kind)

    print(title("Data"))
    data_set, subsets, splitting_method, splitting_fraction = _load_data(
        data_set_file_or_name, data_format, data_directory,
        preprocessing_methods, noisy_preprocessing_methods, split_data_set,
        splitting_method, splitting_fraction,
        binarise_values=normalise_string(str(keyword_arguments.get(
            "reconstruction_distribution"))) == "bernoulli",
        feature_selection=feature_selection, example_filter=example_filter)
    training_set, validation_set, test_set = subsets
    if split_data_set:
        kinds = {"training": training_set, "validation": validation_set,
                 "test": test_set, "full": data_set}
        if evaluation_set_kind not in kinds:
            raise ValueError(
                "Evaluation set kind `{}` not found.".format(
                    evaluation_set_kind))
        evaluation_set = kinds[evaluation_set_kind]
        prediction_training_set = kinds.get(prediction_training_set_kind)
        if prediction_method and prediction_training_set is None:
            raise ValueError(
                "Prediction training set kind `{}` not found.".format(
                    prediction_training_set_kind))
    else:
        evaluation_set = data_set
        prediction_training_set = data_set
    evaluation_subset_indices = indices_for_evaluation_subset(evaluation_set)

    models_directory = build_directory_path(
        models_directory, data_set=data_set,
        splitting_method=splitting_method,
        splitting_fraction=splitting_fraction)

    print(title("Model"))
    model_arguments = _model_arguments(keyword_arguments)
    if (model_arguments["number_of_classes"] is None
            and training_set.has_labels):
        model_arguments["number_of_classes"] = training_set.number_of_classes
    model = _setup_model(data_set=evaluation_set,
                         models_directory=models_directory, **model_arguments)
    if not model.has_been_trained(run_id=run_id):
        raise Exception(
            "Model not found. Either it has not been trained or "
            "scVAE is looking in the wrong directory. "
            "The models directory resulting from the data set specification "
            "is: \"{}\"".format(models_directory))
    if "all" in model_versions:
        model_versions = ["end_of_training"]
        if better_model_exists(model, run_id=run_id):
            model_versions.append("best_model")
        if model_stopped_early(model, run_id=run_id):
            model_versions.append("early_stopping")
    print(model.description)
    print()

    prediction_specifications = None
    if prediction_method:   # cli.py:450-461
        from scvae_amd.analyses.prediction import PredictionSpecifications
        number_of_clusters = model_arguments["number_of_classes"]
        if number_of_clusters is None:
            number_of_clusters = getattr(
                model, "number_of_latent_clusters", None)
        prediction_specifications = PredictionSpecifications(
            method=prediction_method, number_of_clusters=number_of_clusters,
            training_set_kind=prediction_training_set.kind)
        print("Prediction method: {}.".format(
            prediction_specifications.method))
        print("Number of clusters: {}.".format(
            prediction_specifications.number_of_clusters))
        print("Prediction training set: {} set.".format(
            prediction_specifications.training_set_kind))
        print()

    results = {}
    for model_version in model_versions:
        use_best_model = model_version == "best_model"
        use_early_stopping_model = model_version == "early_stopping"
        print(subtitle("Evaluation ({})".format(
            model_version.replace("_", " "))))
        results[model_version] = model.evaluate(
            evaluation_set=evaluation_set,
            evaluation_subset_indices=evaluation_subset_indices,
            minibatch_size=minibatch_size, run_id=run_id,
            use_best_model=use_best_model,
            use_early_stopping_model=use_early_stopping_model,
            output_versions="all",
            **({"summary_statistics": summary_level} if summary_level
               else {}),
            **({"decompositions": decomposition_level}
               if decomposition_level and "PCA" in decomposition_methods
               else {}),
            **({"distributions": distributions_level}
               if distributions_level else {}),
            **({"distances": True} if distances else {}))
        if summary_level:   # analyses.py:873-899, 1040-1041
            _print_summary_statistics(results[model_version][1])
        print()
        sample_reconstruction_set = None
        if sample_size:   # cli.py:494-505
            print(subtitle("Sampling ({})".format(
                model_version.replace("_", " "))))
            sample_reconstruction_set, _ = model.sample(
                sample_size=sample_size, minibatch_size=minibatch_size,
                run_id=run_id, use_best_model=use_best_model,
                use_early_stopping_model=use_early_stopping_model)
            results[model_version] = (
                results[model_version], sample_reconstruction_set)
            print()
        if (decomposition_level or latent_space or distributions_level
                or distances):
            evaluation_results = (results[model_version][0] if sample_size
                                  else results[model_version])
            version_directory = _decompositions_directory(
                build_directory_path(
                    analyses_directory, data_set=data_set,
                    splitting_method=splitting_method,
                    splitting_fraction=splitting_fraction),
                model, evaluation_set, run_id, use_best_model,
                use_early_stopping_model)
        if decomposition_level:   # analyses.py:1237-1280
            _report_decompositions(
                evaluation_results[1], decomposition_methods,
                sample_reconstruction_set, version_directory)
        if latent_space:   # analyses.py:1405-1416
            _report_latent_space(
                evaluation_results[2], decomposition_methods,
                version_directory)
        if distributions_level:   # analyses.py:1226-1235
            _report_distributions(
                evaluation_results[1], evaluation_set, version_directory)
        if distances:   # analyses.py:1351-1362
            _report_distances(
                evaluation_results[1], evaluation_results[2],
                version_directory)
        if prediction_specifications is not None:   # cli.py:509-543
            _predict(model, results[model_version], prediction_training_set,
                     prediction_specifications, minibatch_size, run_id,
                     use_best_model, use_early_stopping_model, model_version,
                     on_device=bool(prediction_on_device),
                     silhouette_score=bool(silhouette_score),
                     silhouette_space=silhouette_space)
    return results


def _print_summary_statistics(reconstructed_set):
    """The metrics table of ``analyse_results`` (``analyses.py:873, 898-899,
    1040``) from the rows ``model.evaluate`` attached to the reconstructed
    set.  The rows were computed inside the evaluation, before the
    reconstruction left the device; the duration is that of the pass.  With
    several ranks only rank 0 has them: the others print nothing."""
    from scvae_amd.analyses.summary import format_summary_statistics
    statistics = getattr(reconstructed_set, "summary_statistics", None)
    if statistics is None:
        return
    print("Calculating metrics for results.")
    print("Metrics calculated ({}).".format(format_duration(
        getattr(reconstructed_set, "summary_statistics_duration", 0.0))))
    print()
    print(format_summary_statistics(statistics))


def _decompositions_directory(base_directory, model, evaluation_set, run_id,
                              best_model, early_stopping):
    """Where the analyses of one evaluation go, laid out as the reference
    lays them out (``analyses.py:804-830, 1609-1630``):
    ``<base>/<model>/[run_<id>/]e_<epochs>[-early_stopping|-best_model]-mc_<n>
    -iw_<n>/[<kind>/]``, the kind for every set but the test set."""
    from scvae_amd.models.utilities import (
        check_run_id, load_number_of_epochs_trained)
    if run_id is None:
        run_id = defaults["models"]["run_id"]
    parts = ["e_{}".format(load_number_of_epochs_trained(
        model, run_id=run_id, early_stopping=early_stopping,
        best_model=best_model))]
    if early_stopping:
        parts.append("early_stopping")
    elif best_model:
        parts.append("best_model")
    parts.append("mc_{}".format(
        model.number_of_monte_carlo_samples["evaluation"]))
    parts.append("iw_{}".format(
        model.number_of_importance_samples["evaluation"]))
    directory = os.path.join(base_directory, model.name)
    if run_id:
        directory = os.path.join(
            directory, "run_{}".format(check_run_id(run_id)))
    directory = os.path.join(directory, "-".join(parts))
    if evaluation_set.kind != "test":
        directory = os.path.join(directory, evaluation_set.kind)
    return directory


def _write_coordinates(path, data_set, coordinates, column_label="PC"):
    """Example name, the two coordinates (``PC 1``, ``PC 2``) and, where the
    set has labels, the label: tab-separated."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    names = getattr(data_set, "example_names", None)
    labels = (data_set.labels if getattr(data_set, "has_labels", False)
              else None)
    with open(path, "w") as file:
        file.write("\t".join(["example", column_label + " 1",
                              column_label + " 2"]
                             + (["label"] if labels is not None else []))
                   + "\n")
        for i, row in enumerate(coordinates):
            fields = [str(names[i]) if names is not None else str(i),
                      repr(float(row[0])), repr(float(row[1]))]
            if labels is not None:
                fields.append(str(labels[i]))
            file.write("\t".join(fields) + "\n")


def _report_decompositions(reconstructed_set, methods, sampled_set,
                           directory):
    """The lines of ``analyse_decompositions`` (``subanalyses.py:655-674``)
    for the fits ``model.evaluate`` attached to the reconstructed set, one
    line with the explained-variance ratios and the iteration count of each,
    and the files of coordinates.  With several ranks only rank 0 has the
    fits: the others print nothing."""
    for method in methods:
        if method != "PCA":
            print("Decomposition method `{}` is not built: skipped.".format(
                method))
    if "PCA" not in methods:
        return
    fits = [
        ("decomposition", "reconstructions set", "reconstructions"),
        ("decomposition_in_original_space",
         "reconstructed set values in originals set",
         "reconstructed-originals")]
    for attribute, fit_title, name in fits:
        fit = getattr(reconstructed_set, attribute, None)
        if fit is None:
            continue
        print("Decomposing {} using PCA.".format(fit_title))
        print("{} decomposed ({}).".format(
            capitalise_string(fit_title), format_duration(fit["duration"])))
        print("    Explained variance ratios: {}; {} iterations{}.".format(
            ", ".join("{:.5g}".format(ratio)
                      for ratio in fit["explained_variance_ratio"]),
            fit["iterations"],
            "" if fit["converged"] else " (not converged)"))
        print()
        _write_coordinates(os.path.join(directory, name, "pca.tsv"),
                           reconstructed_set, fit["coordinates"])
        if sampled_set is not None and attribute == "decomposition":
            # (analyses.py:1244: the sampled set in the fitted space)
            _write_coordinates(
                os.path.join(directory, name, "pca-sampled.tsv"), sampled_set,
                fit["model"].transform(sampled_set.values))


def _report_distributions(reconstructed_set, evaluation_set, directory):
    """The lines of ``analyse_distributions`` (``subanalyses.py:64-72,
    145-146, 191-192, 291``) for the histograms ``model.evaluate`` attached
    to the reconstructed set, three per set, and one tab-separated file for
    each, ``histograms/<figure name>.tsv``.  With several ranks only rank 0
    has them: the others print and write nothing."""
    from scvae_amd.analyses.distributions import write_histogram
    histograms = getattr(reconstructed_set, "distributions", None)
    if histograms is None:
        return
    set_titles = ["reconstructed {} set".format(evaluation_set.kind),
                  "{} set".format(evaluation_set.kind)]
    for first in range(0, len(histograms), 3):
        counts, log_counts, count_sum = histograms[first:first + 3]
        print("Plotting distributions for {}.".format(
            set_titles[first // 3]))
        print("    Count distribution plotted and saved ({}).".format(
            format_duration(counts["duration"] + log_counts["duration"])))
        print("    Count sum distribution plotted and saved ({}).".format(
            format_duration(count_sum["duration"])))
        print()
        for histogram in (counts, log_counts, count_sum):
            write_histogram(
                os.path.join(directory, "histograms",
                             histogram["name"] + ".tsv"), histogram)


def _report_distances(reconstructed_set, latent_sets, directory):
    """The lines of ``analyse_matrices(..., plot_distances=True)``
    (``subanalyses.py:369-372, 437-468``) for the distance matrices
    ``model.evaluate`` attached to the reconstructed set and to the latent
    set ``z``, and two files for each under ``distances/``: the matrix in
    plotted order as ``<figure name>.npy`` and the table of its examples as
    ``<figure name>.tsv``.  With several ranks only rank 0 has them: the
    others print and write nothing."""
    from scvae_amd.analyses.distances import write_distances
    for data_set in (reconstructed_set, (latent_sets or {}).get("z")):
        matrices = getattr(data_set, "distance_matrices", None)
        if matrices is None:
            continue
        print("Plotting pairwise distances in {} space.".format(
            data_set.version))
        for matrix in matrices:
            write_distances(os.path.join(directory, "distances"), matrix)
            print("    " + " ".join(s for s in [
                "{} distances in {} space".format(
                    matrix["metric"].capitalize(), data_set.version),
                ("for {} randomly sampled examples".format(
                    matrix["sample_size"]) if matrix["sample_size"] else ""),
                "sorted using {}".format(
                    matrix["sorting_method"].replace("_", " ")),
                "plotted and saved",
                "({})".format(format_duration(matrix["duration"]))
            ] if s) + ".")
        print()


def _report_latent_space(latent_sets, methods, directory):
    """The "latent space" group of ``analyse_results``
    (``analyses.py:1405-1416``): for every latent set with more than two
    features and every method the lines of ``analyse_decompositions``
    (``subanalyses.py:595-674``), for t-SNE one line with the KL divergence
    and the iteration count, and the file of coordinates,
    ``latent_space-<version>/<method>.tsv``.  With several ranks only rank 0
    fits and writes."""
    import torch.distributed as dist
    from scvae_amd.analyses.decomposition import DECOMPOSITION_METHOD_LABEL
    from scvae_amd.analyses.tsne import decompose_latent
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return
    for method in methods:
        if method not in ("PCA", "t-SNE"):
            print("Decomposition method `{}` is not built: skipped.".format(
                method))
    for version, latent_set in latent_sets.items():
        if latent_set.values.shape[1] <= 2:
            continue
        set_title = "latent space for {} set".format(version)
        for method in methods:
            if method not in ("PCA", "t-SNE"):
                continue
            fit = decompose_latent(latent_set.values, method, set_title)
            if fit is None:
                continue
            model = fit["model"]
            if hasattr(model, "kl_divergence_"):
                print("    KL divergence: {:.5g}; {} iterations.".format(
                    model.kl_divergence_, model.n_iter_ + 1))
            print()
            _write_coordinates(
                os.path.join(directory, "latent_space-{}".format(version),
                             normalise_string(method) + ".tsv"),
                latent_set, fit["coordinates"],
                column_label=DECOMPOSITION_METHOD_LABEL[method])


def _predict(model, version_results, prediction_training_set, specifications,
             minibatch_size, run_id, use_best_model, use_early_stopping_model,
             model_version, on_device=False, silhouette_score=False,
             silhouette_space="latent"):
    """Cluster the latent representation and attach the predicted labels to
    every version of the evaluation set (``cli.py:509-543``).  With
    ``silhouette_score`` the silhouette scores of the predicted clusters and
    labels over the latent values of the evaluation set follow the metrics
    (a set without labels gets the header and these lines alone).  With
    ``silhouette_space="counts"`` they are taken over the values of the
    evaluation set in count space instead -- the transformed evaluation set,
    which is what the reference's metric receives (``cli.py:548-550`` hands it
    to ``analyse_results``, ``analyses.py:894-895`` to
    ``compute_clustering_metrics``, ``clustering.py:73-82`` takes its
    ``values``)."""
    from scvae_amd.analyses.prediction import (
        MAXIMUM_NUMBER_OF_EXAMPLES_BEFORE_SAMPLING_SILHOUETTE_SCORE,
        clustering_metrics, count_silhouette_metric, predict_labels,
        silhouette_metric)
    print(subtitle("Prediction ({})".format(model_version.replace("_", " "))))
    evaluation_results = (version_results[0]
                          if isinstance(version_results, tuple)
                          else version_results)
    transformed, reconstructed, latent_sets = evaluation_results
    latent_training_sets = model.evaluate(
        evaluation_set=prediction_training_set, minibatch_size=minibatch_size,
        run_id=run_id, use_best_model=use_best_model,
        use_early_stopping_model=use_early_stopping_model,
        output_versions="latent", log_results=False)
    print()
    cluster_ids, predicted_labels, predicted_superset_labels = predict_labels(
        training_set=latent_training_sets["z"],
        evaluation_set=latent_sets["z"], specifications=specifications,
        on_device=on_device)
    for version in [transformed, reconstructed] + list(latent_sets.values()):
        version.update_predictions(
            prediction_specifications=specifications,
            predicted_cluster_ids=cluster_ids,
            predicted_labels=predicted_labels)
    if cluster_ids is not None and transformed.has_labels:
        metrics = clustering_metrics(
            transformed.labels, cluster_ids, predicted_labels,
            transformed.excluded_classes)
        print("Clustering of the {} set ({}):".format(
            transformed.kind, specifications.name))
        for name, value in metrics.items():
            print("    {}: {:.4f}".format(name, value))
    if silhouette_score and cluster_ids is not None:
        if not transformed.has_labels:
            print("Clustering of the {} set ({}):".format(
                transformed.kind, specifications.name))
        if silhouette_space == "counts":
            count_values = transformed.values
            cells = count_values.shape[0]
            limit = MAXIMUM_NUMBER_OF_EXAMPLES_BEFORE_SAMPLING_SILHOUETTE_SCORE
            if cells > limit:
                print("    (count space: {} of {} cells sampled)".format(
                    limit, cells))
            print("    silhouette score (clusters; count space): {:.4f}"
                  .format(count_silhouette_metric(count_values, cluster_ids)))
            if predicted_labels is not None:
                print("    silhouette score (labels; count space): {:.4f}"
                      .format(count_silhouette_metric(
                          count_values, predicted_labels)))
        else:
            latent_values = latent_sets["z"].values
            print("    silhouette score (clusters): {:.4f}".format(
                silhouette_metric(latent_values, cluster_ids)))
            if predicted_labels is not None:
                print("    silhouette score (labels): {:.4f}".format(
                    silhouette_metric(latent_values, predicted_labels)))
    print()


def _parse_default(default):
    if not isinstance(default, bool) and default != 0 and not default:
        default = None
    return default


def build_parser():
    """The argument parser of ``main`` (``cli.py:668-1230``)."""
    parser = argparse.ArgumentParser(
        prog="scvae", description="Model single-cell transcript counts "
        "using deep learning (MI355X build of the training/evaluation path).",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument(
        "--version", "-V", action="version",
        version="%(prog)s {}".format(__version__))
    subparsers = parser.add_subparsers(help="commands", dest="command")
    subparsers.required = True

    parser_train = subparsers.add_parser(
        name="train",
        description="Train model on single-cell transcript counts.",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser_train.set_defaults(func=train)
    parser_evaluate = subparsers.add_parser(
        name="evaluate",
        description="Evaluate model on single-cell transcript counts.",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser_evaluate.set_defaults(func=evaluate)

    dd, dm = defaults["data"], defaults["models"]
    for sub in (parser_train, parser_evaluate):
        sub.add_argument(dest="data_set_file_or_name",
                         help="data set name or path to data set file")
        sub.add_argument("--format", "-f", dest="data_format",
                         metavar="FORMAT",
                         default=_parse_default(dd["format"]),
                         help="format of the data set")
        sub.add_argument("--data-directory", "-D", metavar="DIRECTORY",
                         default=_parse_default(dd["directory"]),
                         help="directory where data are placed or copied")
        sub.add_argument("--feature-selection", "-F", metavar="SELECTION",
                         nargs="+",
                         default=_parse_default(dd["feature_selection"]),
                         help="method for selecting features")
        sub.add_argument("--example-filter", "-E", metavar="FILTER",
                         nargs="+",
                         default=_parse_default(dd["example_filter"]),
                         help="method for filtering examples, optionally "
                              "followed by parameters")
        sub.add_argument("--preprocessing-methods", "-p", metavar="METHOD",
                         nargs="+",
                         default=_parse_default(dd["preprocessing_methods"]),
                         help="methods for preprocessing data (applied in "
                              "order)")
        sub.add_argument("--noisy-preprocessing-methods", "--np",
                         metavar="METHOD", nargs="+",
                         default=_parse_default(
                             dd["noisy_preprocessing_methods"]),
                         help="methods for noisily preprocessing data at "
                              "every epoch (applied in order)")
        sub.add_argument("--split-data-set", action="store_true",
                         default=_parse_default(dd["split_data_set"]),
                         help="split data set into training, validation, "
                              "and test sets")
        sub.add_argument("--splitting-method", metavar="METHOD",
                         default=_parse_default(dd["splitting_method"]),
                         help="method for splitting data into training, "
                              "validation, and test sets")
        sub.add_argument("--splitting-fraction", metavar="FRACTION",
                         type=float,
                         default=_parse_default(dd["splitting_fraction"]),
                         help="fraction to use when splitting data into "
                              "training, validation, and test sets")
        sub.add_argument("--model-type", "-m", metavar="TYPE",
                         default=_parse_default(dm["type"]),
                         help="type of model; either VAE or GMVAE")
        sub.add_argument("--latent-size", "-l", metavar="SIZE", type=int,
                         default=_parse_default(dm["latent_size"]),
                         help="size of latent space")
        sub.add_argument("--hidden-sizes", "-H", metavar="SIZE", type=int,
                         nargs="+",
                         default=_parse_default(dm["hidden_sizes"]),
                         help="sizes of hidden layers")
        sub.add_argument("--number-of-importance-samples", metavar="NUMBER",
                         type=int, nargs="+",
                         default=_parse_default(dm["number_of_samples"]),
                         help="the number of importance weighted samples "
                              "(if two numbers are given, the first will be "
                              "used for training and the second for "
                              "evaluation)")
        sub.add_argument("--number-of-monte-carlo-samples", metavar="NUMBER",
                         type=int, nargs="+",
                         default=_parse_default(dm["number_of_samples"]),
                         help="the number of Monte Carlo samples (if two "
                              "numbers are given, the first will be used for "
                              "training and the second for evaluation)")
        sub.add_argument("--inference-architecture", metavar="KIND",
                         default=_parse_default(
                             dm["inference_architecture"]),
                         help="architecture of the inference model")
        sub.add_argument("--latent-distribution", "-q",
                         metavar="DISTRIBUTION",
                         help="distribution for the latent variable(s)")
        sub.add_argument("--number-of-classes", "-K", metavar="NUMBER",
                         type=int, help="number of proposed clusters in data "
                                        "set")
        sub.add_argument("--parameterise-latent-posterior",
                         action="store_true",
                         default=_parse_default(
                             dm["parameterise_latent_posterior"]),
                         help="parameterise latent posterior parameters, if "
                              "possible")
        sub.add_argument("--generative-architecture", metavar="KIND",
                         default=_parse_default(
                             dm["generative_architecture"]),
                         help="architecture of the generative model")
        sub.add_argument("--reconstruction-distribution", "-r",
                         metavar="DISTRIBUTION",
                         default=_parse_default(
                             dm["reconstruction_distribution"]),
                         help="distribution for the reconstructions")
        sub.add_argument("--number-of-reconstruction-classes", "-k",
                         metavar="NUMBER", type=int,
                         default=_parse_default(
                             dm["number_of_reconstruction_classes"]),
                         help="the maximum count for which to use "
                              "classification")
        sub.add_argument("--prior-probabilities-method", metavar="METHOD",
                         default=_parse_default(
                             dm["prior_probabilities_method"]),
                         help="method to set prior probabilities")
        sub.add_argument("--number-of-warm-up-epochs", "-w",
                         metavar="NUMBER", type=int,
                         default=_parse_default(
                             dm["number_of_warm_up_epochs"]),
                         help="number of initial epochs with a linear "
                              "weight on the KL divergence")
        sub.add_argument("--kl-weight", metavar="WEIGHT", type=float,
                         default=_parse_default(dm["kl_weight"]),
                         help="weighting of KL divergence")
        sub.add_argument("--proportion-of-free-nats-for-y-kl-divergence",
                         metavar="PROPORTION", type=float,
                         default=_parse_default(dm[
                             "proportion_of_free_nats_for_y_kl_divergence"]),
                         help="proportion of maximum y KL divergence, which "
                              "has constant term and zero gradients, for the "
                              "GMVAE (free-bits method)")
        # as in the reference, a store_true flag whose default is True:
        # batch normalisation cannot be switched off from the command line
        sub.add_argument("--minibatch-normalisation", "-b",
                         action="store_true",
                         default=_parse_default(
                             dm["minibatch_normalisation"]),
                         help="use batch normalisation for minibatches")
        sub.add_argument("--batch-correction", "--bc", action="store_true",
                         default=_parse_default(dm["batch_correction"]),
                         help="use batch correction in models")
        sub.add_argument("--dropout-keep-probabilities", metavar="PROBABILITY",
                         type=float, nargs="+",
                         default=_parse_default(
                             dm["dropout_keep_probabilities"]),
                         help="list of probabilities, p, of keeping "
                              "connections when using dropout (interval: "
                              "]0, 1[, where p in {0, 1, False} means no "
                              "dropout)")
        sub.add_argument("--count-sum", action="store_true",
                         default=_parse_default(dm["count_sum"]),
                         help="use count sum")
        sub.add_argument("--minibatch-size", "-B", metavar="SIZE", type=int,
                         default=_parse_default(dm["minibatch_size"]),
                         help="minibatch size for stochastic optimisation "
                              "algorithm")
        sub.add_argument("--run-id", metavar="ID", type=str,
                         default=_parse_default(dm["run_id"]),
                         help="ID for separate run of the model (can only "
                              "contain alphanumeric characters)")
        sub.add_argument("--models-directory", "-M", metavar="DIRECTORY",
                         default=_parse_default(dm["directory"]),
                         help="directory where models are stored")
        sub.add_argument("--analyses-directory", "-A", metavar="DIRECTORY",
                         default=None,
                         help="directory where analyses are saved (plots are "
                              "not part of this build)")

    parser_train.add_argument(
        "--number-of-epochs", "-e", metavar="NUMBER", type=int,
        default=_parse_default(dm["number_of_epochs"]),
        help="number of epochs for which to train")
    parser_train.add_argument(
        "--learning-rate", metavar="RATE", type=float,
        default=_parse_default(dm["learning_rate"]),
        help="learning rate when training")
    parser_train.add_argument(
        "--new-run", action="store_true",
        default=_parse_default(dm["new_run"]),
        help="train a model anew as a separate run with an automatically "
             "generated ID")
    parser_train.add_argument(
        "--reset-training", action="store_true",
        default=_parse_default(dm["reset_training"]),
        help="reset already trained model")
    parser_train.add_argument(
        "--caches-directory", "-C", metavar="DIRECTORY",
        help="directory for temporary storage")
    parser_train.add_argument(
        "--deterministic", action="store_true", default=False,
        help="(this build) bit-repeatable training steps: sum the decoder "
             "gradient over the gene strips in a fixed order instead of with "
             "fp32 atomics (about 5 %% slower at large minibatches)")

    parser_train.add_argument(
        "--resident-training-set", action="store_true", default=False,
        help="(this build) keep the training set as dense uint16 rows on the "
             "device (4.5 GB for 68 579 x 32 738) and let the training steps "
             "read their minibatch out of it through a row index instead of "
             "densifying its CSR rows every step; integer count matrices "
             "without noisy preprocessing, same results bit for bit")

    parser_evaluate.add_argument(
        "--evaluation-set-kind", metavar="KIND",
        default=_parse_default(defaults["evaluation"]["data_set_kind"]),
        help="kind of subset to evaluate and analyse")
    parser_evaluate.add_argument(
        "--sample-size", metavar="SIZE", type=int,
        default=_parse_default(defaults["models"]["sample_size"]),
        help="sample size for sampling model")
    parser_evaluate.add_argument(
        "--prediction-method", "-P", metavar="METHOD",
        default=_parse_default(defaults["evaluation"]["prediction_method"]),
        help="method for predicting labels (k-means, or model for the "
             "clusters of a GMVAE)")
    parser_evaluate.add_argument(
        "--prediction-training-set-kind", metavar="KIND",
        default=_parse_default(
            defaults["evaluation"]["prediction_training_set_kind"]),
        help="kind of subset to fit the prediction method on: training, "
             "validation, test, or full")
    parser_evaluate.add_argument(
        "--prediction-on-device", action="store_true", default=False,
        help="(this build) run the k-means of -P k-means on the GPU: exact "
             "Lloyd iterations for every number of cells (scikit-learn's "
             "mini-batch k-means takes over above 10 000 cells otherwise); at "
             "most 256 clusters, 256 latent values and 8192 centre values, "
             "else scikit-learn as without the switch")
    parser_evaluate.add_argument(
        "--silhouette-score", action="store_true", default=False,
        help="(this build) with -P, also print the silhouette score of the "
             "predicted clusters and labels: exact over every cell, on the "
             "GPU, in the latent space (the reference scores a sample of "
             "20 000 cells in count space); at most 256 latent values, else "
             "scikit-learn on the host")
    parser_evaluate.add_argument(
        "--silhouette-space", choices=["latent", "counts"], default="latent",
        help="(this build) with --silhouette-score: latent, the above, or "
             "counts, the reference's own quantity: the score over the "
             "counts of the evaluation set, 20 000 cells sampled above "
             "20 000, with exact distances on the GPU (integer counts below "
             "65 536, at most 65 536 genes, else scikit-learn on the host)")
    parser_evaluate.add_argument(
        "--summary-statistics", action="store_true", default=False,
        help="(this build) after the evaluation of each model version, print "
             "the metrics table of the reference's analyses: mean, standard "
             "deviation, dispersion, minimum, maximum and sparsity of the "
             "evaluation set and of the reconstructed set, computed on the "
             "GPU in one pass before the reconstruction leaves it")
    parser_evaluate.add_argument(
        "--analysis-level",
        choices=["limited", "normal", "extensive"],
        default=_parse_default(defaults["analyses"]["analysis_level"]),
        help="with --summary-statistics: limited, normal, or extensive, "
             "which adds the rows of the differences and of the log-ratios "
             "between the reconstructed and the evaluation set; with "
             "--decompositions: extensive adds the reconstructions in the "
             "space of the originals; with --distributions: extensive adds "
             "the histograms of the evaluation set")
    parser_evaluate.add_argument(
        "--decompositions", action="store_true", default=False,
        help="(this build) after the evaluation of each model version, fit "
             "the two-component PCA of the reconstructed set on the GPU "
             "before the reconstruction leaves it (the converged exact PCA "
             "where the reference fits an incremental one), print its "
             "explained-variance ratios and write the coordinates of every "
             "example to a tab-separated file under --analyses-directory")
    parser_evaluate.add_argument(
        "--distributions", action="store_true", default=False,
        help="(this build) after the evaluation of each model version, the "
             "histograms of the reconstructed set (counts, counts shifted "
             "by one, count sums), exact over NumPy's bin edges, on the GPU "
             "before the reconstruction leaves it, each written as a "
             "tab-separated table under --analyses-directory; with "
             "--analysis-level extensive also those of the evaluation set")
    parser_evaluate.add_argument(
        "--distances", action="store_true", default=False,
        help="(this build) after the evaluation of each model version, the "
             "pairwise distance matrices of the reconstructed set and of the "
             "z latent values (Euclidean and cosine; sorted by labels, where "
             "there are labels, over at most 10 000 sampled examples, and by "
             "hierarchical clustering over at most 1 000), on the GPU before "
             "the reconstruction leaves it, each written as a .npy matrix "
             "with a .tsv table of its examples under --analyses-directory; "
             "a matrix of 10 000 examples is 400 MB per file")
    parser_evaluate.add_argument(
        "--decomposition-methods", metavar="METHOD", nargs="+",
        default=_parse_default(defaults["analyses"]["decomposition_method"]),
        help="with --decompositions: methods to decompose with (only pca is "
             "built); with --latent-space: pca and t-SNE")
    parser_evaluate.add_argument(
        "--latent-space", action="store_true", default=False,
        help="(this build) after the evaluation of each model version, the "
             "two-dimensional maps of every latent set with more than two "
             "features, one for every method in --decomposition-methods: "
             "pca, or t-SNE exact over every pair of cells on the GPU "
             "(scikit-learn's exact objective and schedule where the "
             "reference fits the Barnes-Hut approximation on the host; 4 to "
             "200 000 cells), their coordinates in tab-separated files "
             "under --analyses-directory")
    parser_evaluate.add_argument(
        "--model-versions", metavar="VERSION", nargs="+",
        default=_parse_default(defaults["evaluation"]["model_versions"]),
        help="model versions to evaluate: end-of-training, best-model, "
             "early-stopping")

    return parser


def main(arguments=None):
    parsed = build_parser().parse_args(arguments)
    started = _start_data_parallel()
    try:
        import torch.distributed as dist
        quiet = (dist.is_available() and dist.is_initialized()
                 and dist.get_rank() != 0)
        if quiet:   # one voice: rank 0 prints, writes logs and checkpoints
            with open(os.devnull, "w") as sink, \
                    contextlib.redirect_stdout(sink):
                status = parsed.func(**vars(parsed))
        else:
            status = parsed.func(**vars(parsed))
    finally:
        if started:
            _stop_data_parallel()
    return status


def _start_data_parallel():
    """One process per GPU: when the command was started by
    ``python -m torch.distributed.run --nproc-per-node N -m scvae_amd train ...``
    (``WORLD_SIZE`` / ``RANK`` / ``LOCAL_RANK`` / ``MASTER_*`` in the
    environment), join the process group before any model is built -- the
    model classes shard every minibatch over the group (``models/base.py``,
    ``dataparallel.py``: contiguous row shards, gradient all-reduce over RCCL,
    synchronised batch norm) -- and leave it afterwards.  The reference is a
    single process (va:887); nothing here changes a run without that
    environment.  ``SCVAE_DIST_BACKEND=gloo`` moves the bytes over the host
    (tests on a box with fewer GPUs than ranks).  Returns whether this call
    created the group."""
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world <= 1:
        return False
    import torch
    import torch.distributed as dist
    if not dist.is_available() or dist.is_initialized():
        return False
    backend = os.environ.get("SCVAE_DIST_BACKEND", "nccl")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    keyword_arguments = {}
    if torch.cuda.is_available():
        device = torch.device("cuda", local_rank % torch.cuda.device_count())
        torch.cuda.set_device(device)
        if backend == "nccl":
            keyword_arguments["device_id"] = device
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend, rank=rank, world_size=world,
                            **keyword_arguments)
    return True


def _stop_data_parallel():
    import torch.distributed as dist
    if dist.is_initialized():
        try:
            dist.barrier()
        finally:
            dist.destroy_process_group()
