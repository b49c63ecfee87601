"""Fit executor: turns a job's candidates into device-batched fit tasks and results.

This is the MI355X replacement for the reference worker's per-task hot path
(aws-prod/worker/worker.py:289-363 ``train_model``): one ``fit`` on a holdout split +
``cross_val_score(cv=5)`` per candidate, each re-reading the CSV.  Here:

1. splits (CV folds + holdout) become one role tensor on the device (search/cv.py);
2. every (candidate, split) becomes a ``FitTask`` with resolved parameters;
3. tasks are grouped by estimator family and run in as few device batches as memory
   allows (models/*.py);
4. predictions are scored on-device (search/scoring.py) and folded into the
   reference's per-candidate result dict (J4 ``R``), with the intended semantics of
   defects D1/D2/D5/D6 (holdout actually works, cv/scoring honoured, failures terminal).

``run_candidates`` is what a worker rank executes for the candidate slice the
scheduler assigned to it.
"""
from __future__ import annotations

import math
import time
import traceback
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from ..models.base import FitOutput, FitTask, ParamError, family_of, is_classifier
from ..search import scoring as scoring_mod
from ..utils import trace
from ..search.cv import make_split_roles


@dataclass
class JobSpec:
    """Everything a worker needs to run a job's fits (derived from J1/J2)."""

    model_type: str
    candidates: List[Dict[str, Any]]          # full estimator params per candidate (base + point)
    cv: int = 5
    # a scorer name, or for a multi-metric job the resolved (label, scorer name) pairs
    # (service.job_plan scoring_labels / scoring_names) with ``refit_metric`` naming the primary label
    scoring: Any = None
    refit_metric: Optional[str] = None
    holdout: bool = True
    test_size: Any = 0.2
    random_state: Any = 42
    error_score: Any = float("nan")
    return_train_score: bool = False
    keep_models: str = "best"                 # none | best | all
    seed: int = 0
    raise_batch_errors: bool = False          # device errors propagate (the caller retries the batch)
    # train_params["permutation_importance"] as service.job_plan resolved it (RandomForest* only):
    # with candidates == "all" every candidate's holdout fit computes it; "best" is one extra fit
    # after aggregation (holdout_permutation)
    permutation: Optional[Dict[str, Any]] = None
    # train_params["partial_dependence"] as service.job_plan resolved it (RandomForest* only).  The
    # refit computes it (service.refit_model sets FitTask.partial_dependence); here it only names
    # the tables on which the refit will compute nothing
    partial_dependence: Optional[Dict[str, Any]] = None
    # train_params["staged_scores"] as service.job_plan resolved it (GradientBoosting* only): every
    # CV and holdout fit records its held-out score after every stage (FitTask.staged), and a
    # candidate's result gains ``staged_scores`` (staged_entry)
    staged: Optional[Dict[str, Any]] = None

    def split_key(self):
        return (self.cv, self.holdout, str(self.test_size), str(self.random_state), is_classifier(self.model_type))


@dataclass
class CandidateResult:
    candidate: int
    ok: bool
    result: Dict[str, Any] = field(default_factory=dict)   # J4 R
    error: Optional[str] = None
    model: Any = None
    fit_seconds: float = 0.0


def prepare_splits(data, spec: JobSpec) -> List[str]:
    key = spec.split_key()
    if key is not None and getattr(data, "_split_key", None) == key and getattr(data, "split_names", None):
        return list(data.split_names)   # the resident split roles are this job's (every slice re-asks)
    roles, names = make_split_roles(data.y_host, spec.cv if spec.cv else 0, is_classifier(spec.model_type),
                                    holdout=spec.holdout, test_size=spec.test_size,
                                    random_state=spec.random_state)
    data.set_splits(roles, names, key=spec.split_key())
    return names


def build_tasks(data, spec: JobSpec, candidate_ids: Sequence[int]):
    fam = family_of(spec.model_type)
    tasks: List[FitTask] = []
    errors: Dict[int, str] = {}
    tid = 0
    for c in candidate_ids:
        params = spec.candidates[c]
        try:
            for s in range(len(data.split_names)):
                rp = fam.resolve(spec.model_type, params, data.train_counts[s], data.d, data.n_classes)
                tasks.append(FitTask(task_id=tid, candidate=c, split=s, model_type=spec.model_type, params=rp,
                                     seed=(spec.seed * 1000003 + c) & 0xFFFFFFFF))
                tid += 1
        except (ParamError, ValueError, TypeError) as e:
            errors[c] = f"{type(e).__name__}: {e}"
            tasks = [t for t in tasks if t.candidate != c]
    return tasks, errors


def _batched_scores(data, tasks, outputs: Dict[int, FitOutput], scorer: str) -> Dict[int, float]:
    """Accuracy of every device fit in a few launches and ONE device->host read: fits are
    grouped by split (same held-out rows), their predictions stacked and scored together --
    instead of one reduction and one host sync per fit (a 2,560-fit LogisticRegression batch
    spent 0.27 s per search in per-fit syncs).  Exact: a mean of 0/1 counts is the same
    double whatever the reduction order.  roc_auc, roc_auc_ovr and roc_auc_ovr_weighted are
    batched too (``_rank_proba_scores``): their statistics are integers.  Every other scorer is
    a floating-point sum whose last place would move, and stays per fit."""
    if scorer in _EXACT_RANK and getattr(data, "is_gpu", False):
        # roc_auc*: one division of exact integer rank statistics, done as torch does it for device
        # tensors (score_from_rank_stats device_division): the bits of scoring._auc on this data
        # path (docs/RANK_SCORES.md); fits that are not batched are scored per fit as before
        return {tid: v[scorer] for tid, v in _rank_proba_scores(data, tasks, outputs, [scorer], True).items()}
    if scorer != "accuracy" or not getattr(data, "is_gpu", False):
        return {}
    by_split: Dict[int, List[FitTask]] = {}
    for t in tasks:
        o = outputs.get(t.task_id)
        if o is None or o.error or not isinstance(o.pred, torch.Tensor) or not o.pred.is_cuda:
            continue
        by_split.setdefault(t.split, []).append(t)
    ids, vals = [], []
    for sp, ts in by_split.items():
        y = data.test_targets(sp)
        if y.numel() == 0 or any(outputs[t.task_id].pred.numel() != y.numel() for t in ts):
            continue
        P = torch.stack([outputs[t.task_id].pred.reshape(-1) for t in ts])
        vals.append((P.long() == y.long().view(1, -1)).double().mean(1))
        ids.extend(t.task_id for t in ts)
    if not vals:
        return {}
    return dict(zip(ids, torch.cat(vals).cpu().tolist()))


_EXACT_RANK = ("roc_auc", "roc_auc_ovr", "roc_auc_ovr_weighted")


def _rank_proba_scores(data, tasks, outputs: Dict[int, FitOutput], names,
                       device_division: bool = False) -> Dict[int, Dict[str, float]]:
    """The ranking and probability scorers among ``names`` (``scoring.RANK_SCORERS``,
    ``scoring.PROBA_SUM_SCORERS``) for every fit that hands over float32 scores on the targets'
    device: {task_id: {scorer name: score}}.  The binary column (``proba[:, 1]``, or the decision
    values when there are no probabilities) of those fits is concatenated once and
    ``scoring.rank_statistics`` runs once on it; the whole probability matrices are concatenated
    once for one ``rank_statistics`` call (roc_auc_ovr*) and one ``proba_statistics`` call.  A fit
    that is absent from the result -- float64 scores (SVC), another length or device, more classes
    than the kernels take, a row-sharded table -- is scored by ``scoring.score`` as before."""
    names = [nm for nm in dict.fromkeys(names) if nm in scoring_mod.RANK_SCORERS or nm in scoring_mod.PROBA_SUM_SCORERS]
    C = int(getattr(data, "n_classes", 0) or 0)
    if not names or C < 2 or getattr(data, "is_row_shard", False):
        return {}
    y_all = data.y_cls
    col_names = [nm for nm in names if nm in ("roc_auc", "average_precision")] if C == 2 else []
    ovr_names = [nm for nm in names if nm.startswith("roc_auc_ovr")]
    sum_names = [nm for nm in names if nm in scoring_mod.PROBA_SUM_SCORERS]
    if C > scoring_mod.MAX_STAT_CLASSES:
        ovr_names, sum_names = [], []

    def f32(v, shape):
        return isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.device == y_all.device and \
            tuple(v.shape) == shape

    col, mat = [], []
    for t in tasks:
        o = outputs.get(t.task_id)
        m = int(data.test_rows[t.split].numel())
        if o is None or o.error or m == 0:
            continue
        if f32(o.proba, (m, C)):
            mat.append((t, o.proba))
            col.append((t, o.proba[:, 1]))
        elif o.proba is None and f32(o.decision, (m,)):
            col.append((t, o.decision))
    res: Dict[int, Dict[str, float]] = {}

    def cat(group):
        rows = torch.cat([data.test_rows[t.split] for t, _s in group])
        off = np.concatenate([[0], np.cumsum([int(s.shape[0]) for _t, s in group])]).astype(np.int64)
        return rows, off, torch.cat([s for _t, s in group])

    try:
        if col and col_names:
            rows, off, s = cat(col)
            st = scoring_mod.rank_statistics(rows, off, s, y_all, C, pos0=1, want=scoring_mod.rank_want(col_names))
            for i, (t, _s) in enumerate(col):
                res.setdefault(t.task_id, {}).update(
                    {nm: scoring_mod.score_from_rank_stats(nm, st[i], C, device_division) for nm in col_names})
        if mat and (ovr_names or sum_names):
            rows, off, P = cat(mat)
            if ovr_names:
                st = scoring_mod.rank_statistics(rows, off, P, y_all, C, pos0=0)
                for i, (t, _s) in enumerate(mat):
                    res.setdefault(t.task_id, {}).update(
                        {nm: scoring_mod.score_from_rank_stats(nm, st[i], C, device_division) for nm in ovr_names})
            if sum_names:
                ps = scoring_mod.proba_statistics(rows, off, P, y_all, C, want=scoring_mod.proba_want(sum_names))
                for i, (t, _s) in enumerate(mat):
                    res.setdefault(t.task_id, {}).update(
                        {nm: scoring_mod.score_from_rank_stats(nm, ps[i], C) for nm in sum_names})
    except ValueError:
        # entries the statistics refuse (a NaN score, a target outside the classes): the per-fit
        # scorers keep their behaviour on such data
        return {}
    return res


def _scores_for(data, task: FitTask, out: FitOutput, scorer: str, pre: Optional[Dict[int, float]] = None):
    if pre is not None and task.task_id in pre:
        return pre[task.task_id]
    if scorer == "score":
        return float(out.info["score"])
    y = data.test_targets(task.split)
    return scoring_mod.score(scorer, y, out.pred, data.n_classes, out.proba, decision=out.decision)


def _multi_scores(data, tasks, outputs: Dict[int, FitOutput], pairs, clf: bool) -> Dict[int, Dict[str, float]]:
    """Every metric of a multi-metric job for every successful fit, CV and holdout together:
    {task_id: {label: score}}.  The predictions of the whole family batch are stacked and
    ``scoring.fit_statistics`` runs once (one launch, one device->host read); every metric in
    ``scoring.STAT_SCORERS`` is derived from that read-back, and the ranking and probability
    scorers from the batched rank and probability statistics (``_rank_proba_scores``).  The median
    scorers and roc_auc_ovo* go through ``scoring.score`` per fit, as in a single-metric job -- and so does a fit
    whose predictions are not the kernel's types (float64 regression predictions are scored in
    float64, not rounded to float32), and every fit of a row-sharded table (its resident targets
    are one rank's)."""
    y_all = data.y_cls if clf else data.y_reg
    C = int(data.n_classes) if clf else 0
    stat_names = sorted({nm for _l, nm in pairs if nm in scoring_mod.STAT_SCORERS})
    if getattr(data, "is_row_shard", False):
        stat_names = []
    live, batched = [], []
    for t in tasks:
        o = outputs.get(t.task_id)
        if o is None or o.error or not isinstance(o.pred, torch.Tensor):
            continue
        live.append(t)
        p = o.pred
        fits = p.numel() == data.test_rows[t.split].numel() and p.device == y_all.device
        typed = (not p.is_floating_point() and C >= 2) if clf else p.dtype == torch.float32
        if stat_names and fits and typed:
            batched.append(t)
    stats: Dict[int, Any] = {}
    if batched:
        rows = torch.cat([data.test_rows[t.split] for t in batched])
        preds = [outputs[t.task_id].pred.reshape(-1) for t in batched]
        pred = torch.cat([p.to(torch.int32) for p in preds] if clf else preds)
        off = np.concatenate([[0], np.cumsum([p.numel() for p in preds])]).astype(np.int64)
        st = scoring_mod.fit_statistics(rows, off, pred, y_all, C, want=scoring_mod.stats_want(stat_names))
        stats = {t.task_id: st[i] for i, t in enumerate(batched)}
    ranked = _rank_proba_scores(data, live, outputs, [nm for _l, nm in pairs]) if clf else {}
    res: Dict[int, Dict[str, float]] = {}
    for t in live:
        o = outputs[t.task_id]
        y = None
        vals: Dict[str, float] = {}
        for label, nm in pairs:
            if nm in scoring_mod.STAT_SCORERS and t.task_id in stats:
                vals[label] = scoring_mod.score_from_stats(nm, stats[t.task_id], data.n_classes)
            elif nm in ranked.get(t.task_id, ()):
                vals[label] = ranked[t.task_id][nm]
            else:
                if y is None:
                    y = data.test_targets(t.split)
                vals[label] = scoring_mod.score(nm, y, o.pred, data.n_classes, o.proba, decision=o.decision)
        res[t.task_id] = vals
    return res


def _cv_summary(cv_scores: List[float], error_score) -> tuple:
    """(mean_cv_score, std_cv_score) of one metric's fold scores."""
    finite = [x for x in cv_scores if x is not None and not math.isnan(x)]
    mean = float(np.mean(cv_scores)) if len(finite) == len(cv_scores) else (
        float(np.mean(finite)) if finite and error_score is None else float("nan"))
    return mean, (float(np.std(cv_scores)) if finite else float("nan"))


def run_candidates(data, spec: JobSpec, candidate_ids: Sequence[int]) -> List[CandidateResult]:
    """Run every split of the given candidates; returns one result per candidate."""
    with trace.range("run_prepare"):
        names = prepare_splits(data, spec)
    clf = is_classifier(spec.model_type)
    fam = family_of(spec.model_type)
    self_scored = spec.model_type in getattr(fam, "self_scored", ())
    pairs = None   # multi-metric: (label, scorer name) in the order asked
    if self_scored:
        # estimators scored by their own ``score`` method (sklearn GridSearchCV with scoring=None)
        if spec.scoring not in (None, "None", "", "score"):
            raise ValueError(f"scoring {spec.scoring!r} needs predictions; {spec.model_type} only has score()")
        scorer = "score"
    elif isinstance(spec.scoring, (list, tuple)):
        pairs = [(str(label), scoring_mod.validate_scoring(nm, clf)) for label, nm in spec.scoring]
        if not pairs:
            raise ValueError("multi-metric scoring needs at least one metric")
        primary = spec.refit_metric if spec.refit_metric is not None else pairs[0][0]
        if primary not in dict(pairs):
            raise ValueError(f"refit metric {primary!r} is not one of the scorer keys {[lb for lb, _n in pairs]}")
        scorer = dict(pairs)[primary]   # the single-metric keys of the result describe the primary metric
    else:
        scorer = scoring_mod.validate_scoring(spec.scoring, clf)
    if not clf and not self_scored and not getattr(data, "y_is_numeric", True):
        raise ValueError(f"{spec.model_type} needs a numeric target column; this target is categorical")
    streamable = getattr(fam, "streams_rows", False) and getattr(data, "can_stream_rows", lambda: False)()
    if getattr(data, "binned_only", False) and not getattr(fam, "binned_ok", False) and not streamable:
        if getattr(fam, "host_ok", False) and getattr(data, "can_stream_rows", lambda: False)():
            # a family with a host solver (SVC/SVR) fits on the host rows of the table, which the
            # reference also requires to fit in RAM; same splits, same scorer, CPU predictions
            data = data.host_view()
            with trace.range("run_prepare"):
                names = prepare_splits(data, spec)
        else:
            raise ValueError(f"{spec.model_type} needs the float32 rows; this table is resident only in binned "
                             f"form (too large for HBM) -- tree models only")
    sharded = getattr(data, "is_row_shard", False)
    if sharded and not getattr(fam, "data_parallel", False):
        raise ValueError(f"{spec.model_type} has no row-sharded (data-parallel) fit; run it task-parallel")
    with trace.range("run_tasks"):
        tasks, errors = build_tasks(data, spec, candidate_ids)
    if pairs is not None:
        from ..models.svm import _NOT_FROM_PROBA

        # probabilities when any metric needs them; FitTask.scorer names one that reads
        # FitOutput.proba if there is one, so svm._asks_proba is true exactly then
        asks = [nm for _l, nm in pairs if scoring_mod.needs_proba(nm)]
        if asks:
            reads = [nm for nm in asks if nm not in _NOT_FROM_PROBA]
            for t in tasks:
                t.need_proba = True
                t.scorer = reads[0] if reads else asks[0]
    elif scoring_mod.needs_proba(scorer):   # families that only predict labels by default add probabilities
        for t in tasks:
            t.need_proba = True
            t.scorer = scorer
    if data.is_gpu and not getattr(fam, "uses_forest_arena", False):
        from ..ops import forest_ops

        forest_ops.ARENA.clear(data.device)   # idle forest buffers back to the device for this family
    perm_all = bool(spec.permutation) and spec.permutation.get("candidates") == "all" and "holdout" in names
    keep = spec.keep_models in ("all", "best") or perm_all   # the importances ride on the holdout fit's model
    if keep and "holdout" in names:   # only the holdout fit's model is reported (J4 model_path)
        hold = names.index("holdout")
        for t in tasks:
            t.keep = t.split == hold
            if perm_all and t.keep:
                t.permutation = spec.permutation
    if spec.staged:
        for t in tasks:
            t.staged = spec.staged
    outputs: Dict[int, FitOutput] = {}
    if tasks:
        try:
            with trace.range("run_family"):
                fam_out = fam.run(data, tasks, keep_models=keep)
            for o in fam_out:
                outputs[o.task_id] = o
            if sharded:   # rank-local held-out predictions -> the global prediction vectors
                data.gather_outputs(tasks, outputs)
        except ParamError as e:
            for t in tasks:
                errors.setdefault(t.candidate, f"ParamError: {e}")
        except Exception as e:  # device/kernel failure: every candidate of the batch fails
            if spec.raise_batch_errors:
                raise
            msg = f"{type(e).__name__}: {e}"
            for t in tasks:
                errors.setdefault(t.candidate, msg)
            traceback.print_exc()
    by_cand: Dict[int, List[FitTask]] = {}
    for t in tasks:
        by_cand.setdefault(t.candidate, []).append(t)
    cv_idx = [i for i, n in enumerate(names) if n.startswith("cv")]
    hold_idx = names.index("holdout") if "holdout" in names else None
    multi: Dict[int, Dict[str, float]] = {}
    with trace.range("run_scores"):
        if pairs is not None:
            multi = _multi_scores(data, tasks, outputs, pairs, clf)
            pre = {tid: v[primary] for tid, v in multi.items()}
        else:
            pre = _batched_scores(data, [t for t in tasks if t.split in cv_idx], outputs, scorer)
    results: List[CandidateResult] = []
    for c in candidate_ids:
        if c in errors and c not in by_cand:
            results.append(_failed(c, spec, errors[c]))
            continue
        if c in errors:
            results.append(_failed(c, spec, errors[c]))
            continue
        ts = by_cand.get(c, [])
        split_out = {t.split: (t, outputs.get(t.task_id)) for t in ts}
        cv_scores: List[float] = []
        label_cv: Dict[str, List[float]] = {label: [] for label, _nm in pairs or ()}
        warnings: List[str] = []
        failed_fits = 0
        for s in cv_idx:
            t, o = split_out[s]
            if o is None or o.error:
                failed_fits += 1
                if spec.error_score == "raise":
                    results.append(_failed(c, spec, o.error if o else "fit failed"))
                    break
                cv_scores.append(float(spec.error_score) if spec.error_score is not None else float("nan"))
                for v in label_cv.values():   # a failed fold takes error_score for every metric
                    v.append(cv_scores[-1])
                continue
            with trace.range("run_scores"):
                cv_scores.append(_scores_for(data, t, o, scorer, pre))
            for label, v in label_cv.items():
                v.append(multi[t.task_id][label])
            for w in o.info.get("warnings", []):
                if w not in warnings:
                    warnings.append(w)
        else:
            R: Dict[str, Any] = {}
            fit_s = sum((split_out[s][1].fit_seconds if split_out[s][1] else 0.0) for s in split_out)
            model = None
            hold_out = split_out[hold_idx][1] if hold_idx is not None else None
            if (hold_idx is not None and (hold_out is None or hold_out.error)) or (cv_idx and failed_fits == len(cv_idx)):
                errs = [o.error for _t, o in split_out.values() if o is not None and o.error]
                results.append(_failed(c, spec, errs[0] if errs else "fit failed"))
                continue
            if hold_idx is not None:
                t, o = split_out[hold_idx]
                if self_scored:
                    R["score"] = _scores_for(data, t, o, "score")
                elif clf:
                    R["accuracy"] = _scores_for(data, t, o, "accuracy")
                else:
                    R["r2_score"] = _scores_for(data, t, o, "r2")
                    R["mean_squared_error"] = -_scores_for(data, t, o, "neg_mean_squared_error")
                R["training_time"] = o.fit_seconds
                model = o.model
                if isinstance(model, dict) and model.get("kind") == "forest" and \
                        model.get("oob_score") is not None:   # RandomForest* oob_score=True
                    R["oob_score"] = float(model["oob_score"])
                    for w in o.info.get("warnings", []):   # the kept fit's own (rows no tree left out)
                        if w not in warnings:
                            warnings.append(w)
                entry = permutation_entry(model)
                if entry is not None:
                    R["permutation_importance"] = entry
                if spec.permutation:
                    from ..models.forest import PERM_SHARDED

                    if sharded and PERM_SHARDED not in warnings:
                        warnings.append(PERM_SHARDED)
                    if spec.keep_models not in ("all", "best"):   # kept for the importances only
                        model = None
                if spec.partial_dependence:
                    from ..models.forest import PD_BINNED, PD_SHARDED

                    off = PD_SHARDED if sharded else (PD_BINNED if getattr(data, "X", None) is None else None)
                    if off and off not in warnings:
                        warnings.append(off)
            else:
                R["training_time"] = fit_s
            if cv_idx:
                R["cv_scores"] = cv_scores
                R["mean_cv_score"], R["std_cv_score"] = _cv_summary(cv_scores, spec.error_score)
            else:
                main = "score" if self_scored else ("accuracy" if clf else "r2_score")
                R["cv_scores"] = []
                R["mean_cv_score"] = R.get(main, float("nan"))
            if pairs is not None:   # every metric, the primary one included (docs/MULTIMETRIC.md)
                held = multi.get(split_out[hold_idx][0].task_id) if hold_idx is not None else None
                R["scores"] = {}
                for label, nm in pairs:
                    e: Dict[str, Any] = {"scorer": nm, "cv_scores": label_cv[label]}
                    if cv_idx:
                        e["mean_cv_score"], e["std_cv_score"] = _cv_summary(label_cv[label], spec.error_score)
                    else:   # no folds: the job ranks by the held-out score
                        e["mean_cv_score"] = held[label] if held else float("nan")
                        e["std_cv_score"] = float("nan")
                    if held is not None:
                        e["holdout_score"] = held[label]
                    R["scores"][label] = e
                if not cv_idx:
                    R["mean_cv_score"] = R["scores"][primary]["mean_cv_score"]
            if spec.staged:
                entry = staged_entry([split_out[s][1] for s in cv_idx], hold_out)
                if entry is not None:
                    R["staged_scores"] = entry
            R["scoring"] = scorer
            R["fit_time_total"] = fit_s
            its = [split_out[s][1].info.get("n_iter") for s in cv_idx if split_out[s][1] is not None]
            if its and all(i is not None for i in its):   # iterative solvers: per-fold n_iter (sklearn n_iter_)
                R["n_iter"] = [int(i) for i in its]
            R["n_fits"] = len(split_out)
            if failed_fits:
                R["failed_fits"] = failed_fits
            if warnings:
                R["warnings"] = warnings
            R["parameters"] = spec.candidates[c]
            results.append(CandidateResult(candidate=c, ok=True, result=R, model=model, fit_seconds=fit_s))
    return results


PERM_MODEL_KEYS = ("permutation_importances_mean", "permutation_importances_std", "permutation_baseline_score",
                   "permutation_rows", "permutation_meta")


def permutation_entry(model) -> Optional[Dict[str, Any]]:
    """The ``permutation_importance`` entry of a J4 result from a model that carries the arrays."""
    if not isinstance(model, dict) or model.get("permutation_importances_mean") is None:
        return None
    meta = model.get("permutation_meta") or {}
    return {"importances_mean": [float(v) for v in model["permutation_importances_mean"]],
            "importances_std": [float(v) for v in model["permutation_importances_std"]],
            "baseline_score": float(model["permutation_baseline_score"]),
            "scoring": meta.get("scoring"), "n_repeats": meta.get("n_repeats"),
            "random_state": meta.get("random_state")}


def staged_entry(cv_outs, hold_out) -> Optional[Dict[str, Any]]:
    """The ``staged_scores`` entry of a J4 result from the fits' ``info["staged"]`` curves: the CV
    score after every stage as plain lists.  Folds that early stopping ended at different stages
    are cut to the shortest (``n_stages``); ``best_stage`` is 1-based, the first maximum of
    ``mean_cv_score``.  None when no fit carries a curve (row-sharded jobs)."""
    curves = [o.info["staged"] for o in cv_outs if o is not None and not o.error and o.info.get("staged")]
    hold = hold_out.info.get("staged") if hold_out is not None and not hold_out.error else None
    if not curves and hold is None:
        return None
    S = min(len(c["score"]) for c in curves + ([hold] if hold is not None else []))
    entry: Dict[str, Any] = {"scoring": (curves[0] if curves else hold)["scoring"], "n_stages": int(S)}
    if curves:
        sc = np.asarray([c["score"][:S] for c in curves], dtype=np.float64)
        entry["cv_scores"] = sc.tolist()
        entry["mean_cv_score"] = sc.mean(0).tolist()
        entry["std_cv_score"] = sc.std(0).tolist()
        entry["mean_cv_loss"] = np.asarray([c["loss"][:S] for c in curves], dtype=np.float64).mean(0).tolist()
        best = int(np.argmax(sc.mean(0))) if S else 0
        entry["best_stage"] = best + 1
        entry["best_stage_score"] = float(sc.mean(0)[best]) if S else float("nan")
    if hold is not None:
        entry["holdout_score"] = list(hold["score"][:S])
        entry["holdout_loss"] = list(hold["loss"][:S])
    return entry


PD_MODEL_KEYS = ("pd_features", "pd_grid_off", "pd_grid_values", "pd_average", "pd_rows", "pd_meta")


def partial_dependence_entry(model) -> Optional[Dict[str, Any]]:
    """The ``partial_dependence`` entry of a J4 result from a model that carries the arrays: per
    computed feature its grid values [G] and its averages [n_targets][G], as plain lists."""
    if not isinstance(model, dict) or model.get("pd_features") is None:
        return None
    meta = model.get("pd_meta") or {}
    off = np.asarray(model["pd_grid_off"], dtype=np.int64)
    grid = np.asarray(model["pd_grid_values"], dtype=np.float64)
    avg = np.asarray(model["pd_average"], dtype=np.float64)
    F = len(off) - 1
    entry = {"features": [int(f) for f in model["pd_features"]],
             "grid_values": [grid[off[j]:off[j + 1]].tolist() for j in range(F)],
             "average": [avg[:, off[j]:off[j + 1]].tolist() for j in range(F)],
             "n_rows": int(len(model["pd_rows"])), "grid_resolution": meta.get("grid_resolution"),
             "percentiles": meta.get("percentiles"), "max_rows": meta.get("max_rows"),
             "random_state": meta.get("random_state")}
    if meta.get("warnings"):
        entry["warnings"] = list(meta["warnings"])
    return entry


def holdout_permutation(data, spec: JobSpec, candidate: int) -> Optional[Dict[str, Any]]:
    """``candidates == "best"``: fit one candidate once more on the job's holdout split, with the
    seed its first holdout fit had (the same trees, so the baseline is the holdout score already
    in its result), and return that fit's model with the permutation arrays.  None under a row
    shard, where nothing is computed."""
    if getattr(data, "is_row_shard", False):
        return None
    names = prepare_splits(data, spec)
    tasks, errors = build_tasks(data, spec, [candidate])
    if errors or "holdout" not in names:
        return None
    hold = names.index("holdout")
    task = [t for t in tasks if t.split == hold][0]
    task.keep, task.permutation = True, spec.permutation
    out = family_of(spec.model_type).run(data, [task], keep_models=True)[0]
    return None if out.error else out.model


def _failed(c: int, spec: JobSpec, err: str) -> CandidateResult:
    return CandidateResult(candidate=c, ok=False, error=err, result={"parameters": spec.candidates[c]})
