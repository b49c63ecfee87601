"""Model artefacts: safe on-disk format + CPU/GPU prediction.

The reference pickles every fitted sklearn model into the worker's local
``./models/<subtask>_model.pkl`` (aws-prod/worker/worker.py:351-356) and the master
tries to ``send_file`` a path that only exists on the worker (D18).  Here artefacts
live in one shared model store as ``.npz`` (arrays + a JSON metadata string; loaded
with ``allow_pickle=False``, so downloading and loading a model executes nothing).

Kinds: ``forest`` (pool layout of ops/forest_ops.py + bin edges),
``linear_logistic``, ``linear_regression``, ``knn`` (training rows), ``gbrt`` (stage trees),
``svm`` (support vectors + dual coefficients per one-vs-one machine), ``pca`` (mean,
components, explained variances, noise variance).

``load_predictor(path)`` wraps an artefact in an estimator-like object (``predict``,
``predict_proba`` / ``decision_function`` for classifiers, ``score``, ``transform`` for
PCA) -- what the reference's pickled sklearn estimator gives its user after
``download_best_model`` (DistributedLibrary/src/distributed_ml/core.py:201-206,
aws-prod/worker/worker.py:351-356), without unpickling anything.
"""
from __future__ import annotations

import json
import os
import re
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np

_ARRAY_KEYS = ("nodes", "vals", "edges", "coef", "intercept", "X", "y", "init", "stage_offsets", "scale", "mean",
               "components", "var", "min", "max", "value", "roots", "feature_importances", "oob_rows",
               "oob_decision_function", "oob_prediction", "permutation_importances", "permutation_importances_mean",
               "permutation_importances_std", "permutation_baseline_score", "permutation_rows", "pd_features",
               "pd_grid_off", "pd_grid_values", "pd_average", "pd_rows", "train_score", "oob_scores", "oob_improvement",
               "staged_test_score", "staged_test_loss")


def save_model(model: Dict[str, Any], path: str) -> str:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    arrays = {k: np.asarray(v) for k, v in model.items() if k in _ARRAY_KEYS and v is not None}
    meta = {k: v for k, v in model.items() if k not in _ARRAY_KEYS}
    tmp = path + ".tmp.npz"
    np.savez(tmp, __meta__=np.array(json.dumps(meta, default=_jdefault)), **arrays)
    os.replace(tmp, path)
    return path


def _jdefault(o):
    if isinstance(o, np.generic):
        return o.item()
    if isinstance(o, np.ndarray):
        return o.tolist()
    return str(o)


def load_model(path: str) -> Dict[str, Any]:
    with np.load(path, allow_pickle=False) as z:
        meta = json.loads(str(z["__meta__"]))
        for k in z.files:
            if k != "__meta__":
                meta[k] = z[k]
    return meta


_SAFE = re.compile(r"^[A-Za-z0-9_.\-]+$")


class ModelStore:
    def __init__(self, root: str):
        self.root = os.path.abspath(root)
        os.makedirs(self.root, exist_ok=True)

    def path_for(self, model_id: str) -> str:
        if not _SAFE.match(model_id):
            raise ValueError(f"invalid model id {model_id!r}")
        return os.path.join(self.root, f"{model_id}.npz")

    def save(self, model_id: str, model: Dict[str, Any]) -> str:
        return save_model(model, self.path_for(model_id))

    def resolve(self, model_path: Optional[str], model_id: Optional[str]) -> Optional[str]:
        """Only paths inside the store are served (no arbitrary file read)."""
        cands = []
        if model_id:
            try:
                cands.append(self.path_for(model_id))
            except ValueError:
                pass
        if model_path:
            p = os.path.abspath(model_path)
            if p.startswith(self.root + os.sep):
                cands.append(p)
        for c in cands:
            if os.path.isfile(c):
                return c
        return None


def predict(model: Dict[str, Any], X: np.ndarray) -> np.ndarray:
    """Predict raw feature rows on the CPU with the saved artefact."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    kind = model["kind"]
    classes = model.get("classes")
    if kind == "forest":
        from ..ops import forest_ops

        Xb = _bin_rows(model, X)
        fb = _forest_build(model)
        rows = np.arange(X.shape[0], dtype=np.int32)
        out = forest_ops.predict(fb, Xb, np.array([0, fb.n_trees]), np.array([0, X.shape[0]]), rows)
        return np.asarray(classes)[out] if (classes is not None and not fb.is_reg) else out
    if kind == "linear_logistic":
        z = X @ np.asarray(model["coef"]).T + np.asarray(model["intercept"])
        idx = (z[:, 0] > 0).astype(int) if z.shape[1] == 1 else z.argmax(1)
        return np.asarray(classes)[idx]
    if kind == "linear_regression":
        return X @ np.asarray(model["coef"]) + float(model["intercept"])
    if kind == "knn":
        from ..models.neighbors import knn_predict_numpy

        return knn_predict_numpy(model, X)
    if kind == "gbrt":
        from ..models.boosting import gbrt_predict_numpy

        return gbrt_predict_numpy(model, X)
    if kind == "svm":
        from ..models.svm import svm_predict_numpy

        return svm_predict_numpy(model, X)
    if kind == "pca":
        from ..models.transformers import pca_transform_numpy

        return pca_transform_numpy(model, X)   # a transformer's "prediction" is its projection
    raise ValueError(f"unknown model kind {kind!r}")


def _sigmoid(z: np.ndarray) -> np.ndarray:
    return 0.5 * (1.0 + np.tanh(0.5 * z))   # overflow-free logistic


def _softmax(z: np.ndarray) -> np.ndarray:
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(1, keepdims=True)


_REGRESSOR_KINDS = ("linear_regression",)


@dataclass
class PermutationImportance:
    """``Predictor.permutation_importance_``: sklearn's Bunch fields, plus what they were computed
    on.  ``importances`` [d, K] is in the holdout fit's artefact only (None in a refit one)."""

    importances_mean: np.ndarray
    importances_std: np.ndarray
    baseline_score: float
    rows: np.ndarray                 # dataset row ids that were scored (the fit's held-out rows)
    importances: Optional[np.ndarray] = None
    scoring: Optional[str] = None
    n_repeats: Optional[int] = None
    random_state: Optional[int] = None


@dataclass
class PartialDependence:
    """``Predictor.partial_dependence(feature)``: sklearn's Bunch fields for ``kind="average"``."""

    average: np.ndarray              # [n_targets, G]
    grid_values: list                # [array(G)]
    feature: int = -1
    n_rows: Optional[int] = None     # training rows that were averaged over


class Predictor:
    """An estimator over a stored artefact (CPU; nothing from the file is executed).

    * ``predict(X)`` -- labels (classifiers, in the dataset's original label values) or values;
    * ``predict_proba(X)`` -- classifiers whose sklearn counterpart has it (forest, logistic,
      gradient boosting, k-NN, and an SVC fitted with ``probability=True``: Platt scaling +
      pairwise coupling, models/svm.py ``svm_proba_numpy``); an SVC fitted with sklearn's
      default ``probability=False`` has ``decision_function`` only;
    * ``score(X, y)`` -- accuracy (classifiers), R^2 (regressors), mean log-likelihood (PCA),
      the default ``score`` of the sklearn estimator and what a job reports as
      ``accuracy`` / ``r2_score`` / ``score``;
    * ``transform(X)`` -- PCA projection (whitened if the model was).
    """

    def __init__(self, model: Dict[str, Any]):
        self.model = model
        self.kind = str(model["kind"])
        self.model_type = str(model.get("model_type", self.kind))
        cl = model.get("classes")
        self.classes_ = None if cl is None else np.asarray(cl)
        if self.kind == "forest":
            self.is_classifier = not bool(model["is_reg"])
        elif self.kind == "svm":
            self.is_classifier = not bool(model["svr"])
        elif self.kind in ("pca",) + _REGRESSOR_KINDS:
            self.is_classifier = False
        else:
            self.is_classifier = self.classes_ is not None

    def __repr__(self) -> str:
        return f"Predictor({self.model_type}, kind={self.kind})"

    # ---- prediction --------------------------------------------------------------------
    def predict(self, X) -> np.ndarray:
        if self.kind == "pca":
            raise AttributeError("PCA has no predict; use transform / score")
        return predict(self.model, X)

    def decision_function(self, X) -> np.ndarray:
        X = np.ascontiguousarray(X, dtype=np.float32)
        if self.kind == "linear_logistic":
            z = X.astype(np.float64) @ np.asarray(self.model["coef"], dtype=np.float64).T + np.asarray(
                self.model["intercept"], dtype=np.float64)
            return z[:, 0] if z.shape[1] == 1 else z
        if self.kind == "gbrt" and self.is_classifier:
            from ..models.boosting import gbrt_raw_numpy

            raw = gbrt_raw_numpy(self.model, X)
            return raw[:, 0] if raw.shape[1] == 1 else raw
        if self.kind == "svm" and self.is_classifier and int(self.model["n_classes"]) == 2:
            from ..models.svm import _kernel_matrix
            import torch

            m = self.model["machines"][0]
            Xt = torch.from_numpy(X)
            sv = torch.from_numpy(np.asarray(m["sv"], dtype=np.float32).reshape(-1, X.shape[1]))
            K = _kernel_matrix(Xt, sv, int(self.model["kernel"]), float(self.model["gamma"]),
                               float(self.model["coef0"]), int(self.model["degree"]))
            dv = (K @ torch.from_numpy(np.asarray(m["coef"], dtype=np.float64)).to(K.dtype) - m["rho"]).numpy()
            return -dv   # sklearn's binary sign: positive -> classes_[1]
        raise AttributeError(f"{self.model_type} artefact has no decision_function")

    def predict_proba(self, X) -> np.ndarray:
        if not self.is_classifier:
            raise AttributeError(f"{self.model_type} is not a classifier")
        X = np.ascontiguousarray(X, dtype=np.float32)
        kind = self.kind
        if kind == "forest":
            from ..ops import forest_ops

            Xb = _bin_rows(self.model, X)
            fb = _forest_build(self.model)
            rows = np.arange(X.shape[0], dtype=np.int32)
            _, proba = forest_ops.predict(fb, Xb, np.array([0, fb.n_trees]), np.array([0, X.shape[0]]), rows,
                                          want_proba=True)
            return np.asarray(proba, dtype=np.float64)
        if kind == "linear_logistic":
            from ..models.linear import KIND_BINARY, KIND_OVR

            z = np.atleast_2d(self.decision_function(X).T).T
            link = int(self.model.get("link", KIND_BINARY))
            if z.shape[1] == 1:
                p1 = _sigmoid(z[:, 0])
                return np.stack([1.0 - p1, p1], 1)
            if link == KIND_OVR:   # sklearn one-vs-rest: normalised per-class sigmoids
                p = _sigmoid(z)
                return p / p.sum(1, keepdims=True)
            return _softmax(z)
        if kind == "gbrt":
            from ..models.boosting import LOSS_EXP, gbrt_raw_numpy

            raw = gbrt_raw_numpy(self.model, X)
            if raw.shape[1] == 1:
                p1 = _sigmoid(2.0 * raw[:, 0] if int(self.model["loss"]) == LOSS_EXP else raw[:, 0])
                return np.stack([1.0 - p1, p1], 1)
            return _softmax(raw)
        if kind == "knn":
            import torch

            from ..models.neighbors import finish_distance, knn_search_torch, vote

            m = self.model
            Xtr = torch.from_numpy(np.asarray(m["X"], dtype=np.float32))
            ytr = torch.from_numpy(np.asarray(m["y"]))
            Q = torch.from_numpy(X)
            n = Xtr.shape[0]
            metric, p, k = int(m["metric"]), float(m["p"]), int(m["n_neighbors"])
            acc, idx = knn_search_torch(torch.cat([Xtr, Q]), torch.arange(n, n + Q.shape[0]), torch.arange(n), k,
                                        metric, p)
            _, proba = vote(finish_distance(acc, metric, p), ytr[idx], k, m["weights"], int(m.get("n_classes", 1)),
                            True)
            return proba.numpy()
        if kind == "svm":
            from ..models.svm import svm_has_proba, svm_proba_numpy

            if svm_has_proba(self.model):   # fitted with probability=True: probA / probB per machine
                return svm_proba_numpy(self.model, X)
        raise AttributeError(f"{self.model_type} has no predict_proba (sklearn's default probability=False)")

    # ---- fitted forest attributes (sklearn's names; AttributeError when the artefact lacks one) ----
    @property
    def feature_importances_(self) -> np.ndarray:
        """Mean decrease in impurity (ops/forest_ops.py ``feature_importances``).  A forest
        artefact saved without the vector computes it from its nodes and node sums."""
        if self.kind == "gbrt":   # sklearn's GradientBoosting rule, accumulated during the fit
            fi = self.model.get("feature_importances")
            if fi is None:
                raise AttributeError(f"{self.model_type} artefact has no feature_importances_ (it was saved before "
                                     f"gradient-boosting artefacts carried them, or by a row-sharded fit)")
            return np.asarray(fi, dtype=np.float64)
        if self.kind != "forest":
            raise AttributeError(f"{self.model_type} artefact has no feature_importances_")
        fi = self.model.get("feature_importances")
        if fi is None:
            from ..ops import forest_ops

            crit = self.model.get("params", {}).get("criterion")
            if crit in (forest_ops.POISSON, forest_ops.MAE):
                name = "poisson" if crit == forest_ops.POISSON else "absolute_error"
                raise AttributeError(f"feature_importances_ is not available for criterion={name!r}: the artefact "
                                     f"does not hold that impurity's node sums")
            if crit is None:
                crit = forest_ops.MSE if self.model["is_reg"] else forest_ops.GINI
            fi = forest_ops.feature_importances(np.asarray(self.model["nodes"]), np.asarray(self.model["vals"]),
                                                int(self.model["n_trees"]), int(self.model["n_features"]),
                                                bool(self.model["is_reg"]), int(crit))
            self.model["feature_importances"] = fi
        return np.asarray(fi, dtype=np.float64)

    def _oob(self, key: str, name: str):
        v = self.model.get(key) if self.kind == "forest" else None
        if v is None:
            raise AttributeError(f"{self.model_type} artefact has no {name} (fit with oob_score=True, bootstrap=True)")
        return v

    # ---- fitted linear-regression attributes (LinearRegression, Ridge, Lasso, ElasticNet) -----
    def _linreg(self, name: str):
        if self.kind != "linear_regression":
            raise AttributeError(f"{self.model_type} artefact has no {name}")
        return self.model

    @property
    def coef_(self) -> np.ndarray:
        return np.asarray(self._linreg("coef_")["coef"], dtype=np.float64)

    @property
    def intercept_(self) -> float:
        return float(self._linreg("intercept_")["intercept"])

    @property
    def n_iter_(self) -> int:
        """Lasso / ElasticNet: coordinate-descent sweeps run (docs/ELASTIC_NET.md)."""
        v = self._linreg("n_iter_").get("n_iter")
        if v is None:
            raise AttributeError(f"{self.model_type} artefact has no n_iter_")
        return int(v)

    @property
    def dual_gap_(self) -> float:
        """Lasso / ElasticNet: the last duality gap divided by the training rows (sklearn's)."""
        v = self._linreg("dual_gap_").get("dual_gap")
        if v is None:
            raise AttributeError(f"{self.model_type} artefact has no dual_gap_")
        return float(v)

    @property
    def oob_score_(self) -> float:
        """Forests: the out-of-bag score.  GradientBoosting: the last ``oob_scores_`` (a loss)."""
        if self.kind == "gbrt":
            return float(self._gbrt_stage("oob_score", "oob_score_", True))
        return float(self._oob("oob_score", "oob_score_"))

    # ---- fitted gradient-boosting attributes (docs/GBRT_STAGED.md) ------------------------
    def _gbrt_stage(self, key: str, name: str, oob: bool = False):
        v = self.model.get(key) if self.kind == "gbrt" else None
        if v is None:
            why = "fit with subsample < 1" if oob and self.kind == "gbrt" else \
                "a GradientBoosting artefact saved with its per-stage statistics"
            raise AttributeError(f"{self.model_type} artefact has no {name} ({why})")
        return v

    @property
    def n_estimators_(self) -> int:
        """Stages actually fitted (early stopping may end before ``n_estimators``)."""
        if self.kind != "gbrt":
            raise AttributeError(f"{self.model_type} artefact has no n_estimators_")
        return int(np.asarray(self.model["roots"]).shape[0])

    @property
    def train_score_(self) -> np.ndarray:
        """sklearn's ``train_score_`` [n_estimators_]: the loss of the in-bag rows after every stage."""
        return np.asarray(self._gbrt_stage("train_score", "train_score_"), dtype=np.float64)

    @property
    def oob_scores_(self) -> np.ndarray:
        return np.asarray(self._gbrt_stage("oob_scores", "oob_scores_", True), dtype=np.float64)

    @property
    def oob_improvement_(self) -> np.ndarray:
        return np.asarray(self._gbrt_stage("oob_improvement", "oob_improvement_", True), dtype=np.float64)

    def staged_decision_function(self, X):
        """sklearn's generator: the raw scores [n, k] after every stage (k = 1 for binary
        classification and regression), on the host from the stage trees."""
        if self.kind != "gbrt":
            raise AttributeError(f"{self.model_type} artefact has no staged_decision_function")
        from ..models.boosting import gbrt_staged_raw_numpy

        return gbrt_staged_raw_numpy(self.model, X)

    def staged_predict(self, X):
        """sklearn's generator: the prediction after every stage, with ``predict``'s rule."""
        def label(raw):
            if self.classes_ is None:
                return raw[:, 0]
            return self.classes_[(raw[:, 0] >= 0).astype(int) if raw.shape[1] == 1 else raw.argmax(1)]

        return (label(raw) for raw in self.staged_decision_function(X))

    def staged_predict_proba(self, X):
        """sklearn's generator: the class probabilities after every stage."""
        if not self.is_classifier:
            raise AttributeError(f"{self.model_type} is not a classifier")
        from ..models.boosting import LOSS_EXP

        def proba(raw):
            if raw.shape[1] == 1:
                p1 = _sigmoid(2.0 * raw[:, 0] if int(self.model["loss"]) == LOSS_EXP else raw[:, 0])
                return np.stack([1.0 - p1, p1], 1)
            return _softmax(raw)

        return (proba(raw) for raw in self.staged_decision_function(X))

    @property
    def oob_decision_function_(self) -> np.ndarray:
        """[len(oob_rows_), n_classes] in ``classes_`` order; rows no tree left out are zeros."""
        return np.asarray(self._oob("oob_decision_function", "oob_decision_function_"))

    @property
    def oob_prediction_(self) -> np.ndarray:
        return np.asarray(self._oob("oob_prediction", "oob_prediction_"))

    @property
    def oob_rows_(self) -> np.ndarray:
        """Dataset row ids the out-of-bag arrays are aligned with (the fit's training rows)."""
        return np.asarray(self._oob("oob_rows", "oob_rows_"))

    @property
    def permutation_importance_(self) -> "PermutationImportance":
        """sklearn's ``permutation_importance`` result on the fit's held-out rows
        (docs/PERMUTATION_IMPORTANCE.md); a refit artefact carries its holdout fit's values."""
        m = self.model if self.kind == "forest" else {}
        if m.get("permutation_importances_mean") is None:
            raise AttributeError(f"{self.model_type} artefact has no permutation_importance_ (train with "
                                 f"train_params[\"permutation_importance\"])")
        meta = m.get("permutation_meta") or {}
        imp = m.get("permutation_importances")
        return PermutationImportance(
            importances_mean=np.asarray(m["permutation_importances_mean"], dtype=np.float64),
            importances_std=np.asarray(m["permutation_importances_std"], dtype=np.float64),
            baseline_score=float(m["permutation_baseline_score"]),
            rows=np.asarray(m["permutation_rows"]),
            importances=None if imp is None else np.asarray(imp, dtype=np.float64),
            scoring=meta.get("scoring"), n_repeats=meta.get("n_repeats"), random_state=meta.get("random_state"))

    def partial_dependence(self, feature) -> "PartialDependence":
        """One-way partial dependence of ``feature`` (a column position, or a name when the
        artefact has ``feature_names``) on the fit's training rows, as the job computed it
        (docs/PARTIAL_DEPENDENCE.md): sklearn's ``partial_dependence(..., method="brute",
        kind="average")`` fields."""
        m = self.model if self.kind == "forest" else {}
        if m.get("pd_features") is None:
            raise AttributeError(f"{self.model_type} artefact has no partial_dependence (train with "
                                 f"train_params[\"partial_dependence\"])")
        f = feature
        if isinstance(f, str):
            names = list(m.get("feature_names") or [])
            if f not in names:
                raise KeyError(f"no feature named {f!r} in this artefact")
            f = names.index(f)
        feats = [int(x) for x in np.asarray(m["pd_features"])]
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or int(f) not in feats:
            raise KeyError(f"partial dependence was not computed for feature {feature!r} (computed: {feats})")
        j = feats.index(int(f))
        off = np.asarray(m["pd_grid_off"], dtype=np.int64)
        return PartialDependence(
            average=np.asarray(m["pd_average"], dtype=np.float64)[:, off[j]:off[j + 1]].copy(),
            grid_values=[np.asarray(m["pd_grid_values"], dtype=np.float64)[off[j]:off[j + 1]].copy()],
            feature=int(f), n_rows=int(len(m["pd_rows"])))

    # ---- transformers ------------------------------------------------------------------
    def transform(self, X) -> np.ndarray:
        if self.kind != "pca":
            raise AttributeError(f"{self.model_type} has no transform")
        from ..models.transformers import pca_transform_numpy

        return pca_transform_numpy(self.model, X)

    def score_samples(self, X) -> np.ndarray:
        """PCA: per-row log-likelihood under the probabilistic PCA model (sklearn
        ``PCA.score_samples``): variance ``var_i`` (whitened: ``var_i (var_i - noise) + noise``)
        along each kept component, ``noise`` in the orthogonal complement."""
        if self.kind != "pca":
            raise AttributeError(f"{self.model_type} has no score_samples")
        m = self.model
        Xc = np.asarray(X, dtype=np.float64) - np.asarray(m["mean"], dtype=np.float64)
        comp = np.asarray(m["components"], dtype=np.float64)
        var = np.asarray(m["var"], dtype=np.float64)
        noise = float(m["noise_variance"])
        d, k = Xc.shape[1], comp.shape[0]
        if noise == 0.0 and k < d:
            return np.full(Xc.shape[0], -np.inf)
        lam = var * np.maximum(var - noise, 0.0) + noise if m.get("whiten") else np.where(var > noise, var, noise)
        Z = Xc @ comp.T
        resid = np.maximum((Xc * Xc).sum(1) - (Z * Z).sum(1), 0.0)
        quad = ((Z * Z) / lam).sum(1) + (resid / noise if k < d else 0.0)
        logdet = np.log(lam).sum() + ((d - k) * np.log(noise) if k < d else 0.0)
        return -0.5 * quad - 0.5 * (d * np.log(2 * np.pi) + logdet)

    def score(self, X, y=None) -> float:
        if self.kind == "pca":
            return float(np.mean(self.score_samples(X)))
        pred = self.predict(X)
        y = np.asarray(y)
        if self.is_classifier:
            return float(np.mean(pred == y))
        yv = y.astype(np.float64)
        ss_res = float(np.sum((yv - np.asarray(pred, dtype=np.float64)) ** 2))
        ss_tot = float(np.sum((yv - yv.mean()) ** 2))
        if ss_tot == 0.0:
            return 1.0 if ss_res == 0.0 else 0.0
        return 1.0 - ss_res / ss_tot


def _bin_rows(model: Dict[str, Any], X: np.ndarray) -> np.ndarray:
    from ..utils import native

    edges = np.ascontiguousarray(model["edges"], dtype=np.float32)
    Xb = np.empty(X.shape, dtype=np.uint8)
    native.cpu_lib().dml_cpu_bin(native.ptr(X), X.shape[0], X.shape[1], native.ptr(edges), native.ptr(Xb), X.shape[1])
    return Xb


def _forest_build(model: Dict[str, Any]):
    from ..ops import forest_ops

    return forest_ops.ForestBuild(np.ascontiguousarray(model["nodes"]), np.ascontiguousarray(model["vals"]),
                                  int(model["n_trees"]), int(model["vals"].shape[1]), bool(model["is_reg"]),
                                  int(model["n_classes"]))


def load_predictor(path: str) -> Predictor:
    """A downloaded ``.npz`` artefact as an estimator-like :class:`Predictor`."""
    return Predictor(load_model(path))
