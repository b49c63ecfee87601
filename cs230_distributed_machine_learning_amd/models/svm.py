"""SVC / SVR — every dual problem of a job solved in one batched SMO launch.

Reference: both are whitelisted (aws-prod/worker/worker.py:40,47); sklearn fits them per
(candidate, fold) with libsvm (``svm/_libsvm``, C++ SMO), one-vs-one for multiclass.

Here each (candidate, split[, class pair]) is one dual problem for the batched solver
(csrc/kernels/svm.hip on the GPU, csrc/runtime/svm_cpu.cpp on the host), which runs
libsvm's algorithm (WSS3 selection, same update / stopping rule / tie rules), so the
support vectors and decision values match libsvm up to float round-off in the kernel
values.  Rows of each (split, class pair) are gathered ONCE into a feature-major block
shared by every candidate using it.  Decision values for held-out rows are kernel
matrix x coefficient products (library GEMM).  Supported: C, kernel
(linear/poly/rbf/sigmoid), degree, gamma ('scale'/'auto'/float), coef0, tol, max_iter,
class_weight (dict / 'balanced'), epsilon (SVR).  ``shrinking`` / ``cache_size`` only
affect libsvm's speed and are accepted and ignored; ``break_ties=True`` predicts the argmax of
sklearn's one-vs-rest decision function (votes + squashed summed confidences).

``probability=True`` is libsvm's: per machine, 5 more dual problems (an unstratified inner
5-fold CV, solved in the same launch sequence as the outer problems), a sigmoid fitted to
the held-out decision values (Platt scaling, csrc/kernels/svm_prob.hip ``k_platt_fit``) and
pairwise coupling per held-out row (``k_pair_proba``).  Only fits whose scorer reads
probabilities, or whose model is kept, pay for it; ``predict`` stays the vote.  The inner
shuffle is seeded from ``random_state`` -- libsvm's scheme, not sklearn's random stream
(docs/SVC_PROBABILITY.md).
"""
from __future__ import annotations

import ctypes
import math
import os
import time
from typing import Any, Dict, List, Tuple

import numpy as np
import torch

from ..utils import native
from .base import Family, FitOutput, FitTask, ParamError, as_bool, as_float, as_int, register, seed_of

_SVC = "SVC"
_SVR = "SVR"
KLIN, KPOLY, KRBF, KSIG = 0, 1, 2, 3
_KERNELS = {"linear": KLIN, "poly": KPOLY, "rbf": KRBF, "sigmoid": KSIG}

_SVC_DEFAULTS = {"C": 1.0, "kernel": "rbf", "degree": 3, "gamma": "scale", "coef0": 0.0, "shrinking": True,
                 "probability": False, "tol": 1e-3, "cache_size": 200, "class_weight": None, "verbose": False,
                 "max_iter": -1, "decision_function_shape": "ovr", "break_ties": False, "random_state": None}
_SVR_DEFAULTS = {"kernel": "rbf", "degree": 3, "gamma": "scale", "coef0": 0.0, "tol": 1e-3, "C": 1.0,
                 "epsilon": 0.1, "shrinking": True, "cache_size": 200, "verbose": False, "max_iter": -1}

PROB_DTYPE = np.dtype([("xoff", "<i8"), ("roff", "<i8"), ("nrows", "<i8"), ("L", "<i8"), ("voff", "<i8"),
                       ("koff", "<i8"), ("kernel", "<i8"), ("degree", "<i8"), ("gamma", "<f8"), ("coef0", "<f8"),
                       ("eps", "<f8"), ("max_iter", "<i8"), ("iters", "<i8"), ("status", "<i8"), ("svr", "<i8"),
                       ("coff", "<i8"), ("moff", "<i8")])
CHUNK_ITERS = 20000
SPLIT_CHUNK_ITERS = 50000
CACHE_FRACTION = 0.25        # of free HBM for the kernel-column caches (libsvm cache_size analogue) ...
CACHE_MAX_GB = 48.0          # ... and at most this much (DML_SVM_CACHE_GB; 288 GB of HBM per MI355X)
MIN_ROWS_PER_WG = 1024       # split a problem over workgroups only down to this slice size

# ---- SVC(probability=True): libsvm's Platt scaling + pairwise coupling (docs/SVC_PROBABILITY.md) ----
PLATT_FOLDS = 5              # libsvm's inner cross-validation
PLATT_CONVERGED, PLATT_ITER_CAP, PLATT_LINE_SEARCH_FAILED = 0, 1, 2   # csrc/kernels/svm_prob.hip
PAIR_KERNEL_MAX_K = 64       # k_pair_proba: one lane per class
_NO_PROBA = "predict_proba is not available when probability=False"
# scorers that sklearn serves from SVC's decision_function (roc_auc, average_precision: the
# binary decision values, search/scoring.py) or that stay rejected for SVC (top_k_accuracy)
_NOT_FROM_PROBA = ("roc_auc", "average_precision", "top_k_accuracy")


def _asks_proba(t: FitTask) -> bool:
    """The fit's scorer reads ``FitOutput.proba`` (a task built without a scorer name and with
    ``need_proba`` set asks for it too)."""
    return bool(t.need_proba) and getattr(t, "scorer", None) not in _NOT_FROM_PROBA


def platt_seed(seed: int, pair_index: int) -> int:
    """Seed of one machine's inner-CV shuffle: the candidate's ``random_state`` (the task's
    seed when that is None) combined with the class-pair index, so pairs shuffle differently."""
    return (int(seed) * 1000003 + int(pair_index)) & 0xFFFFFFFF


def _task_platt_seed(t: FitTask, pair_index: int) -> int:
    seed = t.params.get("seed")
    return platt_seed(t.seed if seed is None else seed, pair_index)


def platt_folds(nr: int, seed: int) -> List[np.ndarray]:
    """Held-out positions of libsvm's 5 unstratified inner folds over a machine's ``nr`` rows:
    fold i = perm[i*nr//5 : (i+1)*nr//5] of ``RandomState(seed).permutation(nr)``.  Each fold's
    model is fitted on the other positions in ascending order."""
    perm = np.random.RandomState(seed).permutation(nr)
    return [perm[i * nr // PLATT_FOLDS:(i + 1) * nr // PLATT_FOLDS] for i in range(PLATT_FOLDS)]



def _ovr_argmax(dec, ti, pairs, m, C, dev) -> torch.Tensor:
    """sklearn SVC(break_ties=True): argmax of the one-vs-rest decision function built from
    the one-vs-one values (sklearn.utils.multiclass._ovr_decision_function: votes plus
    summed confidences squashed into (-1/3, 1/3))."""
    votes = torch.zeros((m, C), dtype=torch.float64, device=dev)
    conf = torch.zeros((m, C), dtype=torch.float64, device=dev)
    for pi, (a_, b_) in enumerate(pairs):
        dv = dec.get((ti, pi))
        if dv is None:
            continue
        dv = dv.double()
        conf[:, a_] += dv
        conf[:, b_] -= dv
        votes[:, a_] += (dv >= 0).double()
        votes[:, b_] += (dv < 0).double()
    return (votes + conf / (3 * (conf.abs() + 1))).argmax(1).to(torch.int32)

class SVMFamily(Family):
    model_types = (_SVC, _SVR)
    # binned-only tables (float32 rows too large for HBM): the fits run on the host rows with
    # the host SMO -- the reference trains SVC/SVR on any table that fits in RAM
    # (aws-prod/worker/worker.py:40,47,406-425); engine/executor.py run_candidates
    host_ok = True
    classifiers = (_SVC,)

    def resolve(self, model_type, params, n_train, n_features, n_classes) -> Dict[str, Any]:
        defaults = _SVC_DEFAULTS if model_type == _SVC else _SVR_DEFAULTS
        p = dict(defaults)
        p.update({k: v for k, v in params.items() if k in defaults})
        warn = []
        unknown = sorted(k for k in params if k not in defaults)
        if unknown:
            warn.append(f"ignored unknown parameters {unknown}")
        kernel = p["kernel"]
        if kernel not in _KERNELS:
            raise ParamError(f"kernel {kernel!r} is not supported (linear/poly/rbf/sigmoid)")
        C = as_float(p["C"], "C")
        if C <= 0:
            raise ParamError("C <= 0")
        gamma = p["gamma"]
        if isinstance(gamma, str):
            if gamma not in ("scale", "auto"):
                raise ParamError(f"gamma {gamma!r} invalid")
        else:
            gamma = as_float(gamma, "gamma", lo=0.0)
        out = {"C": C, "kernel": _KERNELS[kernel], "degree": as_int(p["degree"], "degree", lo=0),
               "gamma": gamma, "coef0": as_float(p["coef0"], "coef0"), "tol": as_float(p["tol"], "tol", lo=0.0),
               "max_iter": as_int(p["max_iter"], "max_iter", lo=-1), "warnings": warn}
        if model_type == _SVR:
            out["epsilon"] = as_float(p["epsilon"], "epsilon", lo=0.0)
        else:
            cw = p["class_weight"]
            if cw not in (None, "balanced") and not isinstance(cw, dict):
                raise ParamError("class_weight must be None, 'balanced' or a dict")
            out["class_weight"] = cw
            out["probability"] = as_bool(p["probability"], "probability")
            out["seed"] = seed_of(p["random_state"])   # None: the task's seed (inner-CV shuffle)
            out["break_ties"] = as_bool(p["break_ties"], "break_ties")
            if out["break_ties"] and p["decision_function_shape"] == "ovo":
                raise ParamError("break_ties must be False when decision_function_shape is 'ovo'")
        return out

    def cost(self, model_type, rp, n_train, n_features, n_classes) -> float:
        pairs = n_classes * (n_classes - 1) / 2 if model_type == _SVC and n_classes > 2 else 1
        per = n_train / max(1, pairs) if pairs > 1 else n_train
        inner = 1 + PLATT_FOLDS * 0.8 ** 2 if rp.get("probability") else 1   # five four-fifths problems more
        return inner * pairs * per * per * max(1, n_features) * 2e-11 + 1e-2

    # ------------------------------------------------------------------------------------
    def run(self, data, tasks: List[FitTask], keep_models: bool = False) -> List[FitOutput]:
        if not tasks:
            return []
        t0 = time.perf_counter()
        dev = data.device
        svr = not data.classification
        C_cls = data.n_classes
        if not svr:
            # a probability scorer on probability=False fails that candidate alone (sklearn's message)
            bad = {t.task_id for t in tasks if _asks_proba(t) and not t.params.get("probability")}
            if bad:
                done = {o.task_id: o for o in self.run(data, [t for t in tasks if t.task_id not in bad], keep_models)}
                return [done.get(t.task_id) or FitOutput(task_id=t.task_id, error=f"ParamError: {_NO_PROBA}")
                        for t in tasks]
        pairs = [(None, None)] if svr else [(a, b) for a in range(C_cls) for b in range(a + 1, C_cls)]
        # fits that owe class probabilities; every other fit does no extra work at all
        wants = [bool(not svr and t.params.get("probability") and (_asks_proba(t) or (keep_models and t.keep)))
                 for t in tasks]
        # ---- rowsets (split, pair) shared by candidates ----------------------------------
        rowsets: Dict[Tuple, torch.Tensor] = {}
        for t in tasks:
            tr = data.train_rows[t.split].long()
            for pr in pairs:
                key = (t.split, pr)
                if key in rowsets:
                    continue
                if svr:
                    rowsets[key] = tr
                else:
                    yt = data.y_cls[tr]
                    rowsets[key] = tr[(yt == pr[0]) | (yt == pr[1])]
        # ---- Platt scaling: the four-fifths rowsets of the inner 5-fold CV, gathered once per
        # (split, pair, seed); held[key] = the held-out fifths as positions in the machine's rows
        held: Dict[Tuple, List[torch.Tensor]] = {}
        for ti, t in enumerate(tasks):
            if not wants[ti]:
                continue
            for pi, pr in enumerate(pairs):
                sd = _task_platt_seed(t, pi)
                key = (t.split, pr, sd)
                rows = rowsets[(t.split, pr)]
                if key in held or rows.numel() == 0:
                    continue
                folds = platt_folds(rows.numel(), sd)
                held[key] = [torch.from_numpy(f).to(dev) for f in folds]
                for f, ho in enumerate(folds):
                    rest = np.setdiff1d(np.arange(rows.numel()), ho)   # ascending: the rows keep their order
                    rowsets[key + (f,)] = rows[torch.from_numpy(rest).to(dev)]
        keys = list(rowsets)
        xoff, off = {}, 0
        blocks = []
        for k in keys:
            r = rowsets[k]
            blocks.append(data.X[r].t().contiguous().reshape(-1))
            xoff[k] = off
            off += r.numel() * data.d
        Xrs = torch.cat(blocks) if blocks else torch.zeros(1, device=dev)
        norm2 = {k: (data.X[rowsets[k]].double() ** 2).sum(1) for k in keys}
        # ---- problems --------------------------------------------------------------------
        probs, prob_of, ys, Cs, Gs, qds = [], [], [], [], [], []
        voff = roff = koff = 0
        gammas: Dict[int, float] = {}
        const_dec: Dict[Tuple[int, int, int], float] = {}   # inner folds that need no solve
        for ti, t in enumerate(tasks):
            rp = t.params
            gamma = self._gamma(data, t, rp["gamma"], gammas)
            for pi, pr in enumerate(pairs):
                if rowsets[(t.split, pr)].numel() == 0:
                    continue
                todo = [((t.split, pr), -1)]
                if wants[ti]:   # the inner problems ride in the same launch sequence as the outer ones
                    sd = _task_platt_seed(t, pi)
                    todo += [((t.split, pr, sd, f), f) for f in range(PLATT_FOLDS)]
                for key, fold in todo:
                    rows = rowsets[key]
                    nr = rows.numel()
                    if svr:
                        yv = data.y_reg[rows].double()
                        L = 2 * nr
                        y_t = torch.cat([torch.ones(nr), -torch.ones(nr)]).to(dev)
                        G0 = torch.cat([rp["epsilon"] - yv, rp["epsilon"] + yv])
                        C_t = torch.full((L,), rp["C"], dtype=torch.float64, device=dev)
                    else:
                        cls = data.y_cls[rows]
                        if fold >= 0:
                            n_a = int((cls == pr[0]).sum())
                            if n_a == 0 or n_a == nr:   # one class (or no row) left: libsvm's +1 / -1 / 0
                                const_dec[(ti, pi, fold)] = 0.0 if nr == 0 else (1.0 if n_a else -1.0)
                                continue
                        L = nr
                        y_t = torch.where(cls == pr[0], 1.0, -1.0).to(dev)
                        G0 = torch.full((L,), -1.0, dtype=torch.float64, device=dev)
                        w = self._class_weights(data, t, rp["class_weight"])
                        C_t = rp["C"] * torch.where(cls == pr[0], w[pr[0]], w[pr[1]]).double()
                    qd = self._diag(norm2[key], rp["kernel"], gamma, rp["coef0"], rp["degree"])
                    mi = rp["max_iter"] if rp["max_iter"] > 0 else max(10_000_000, 100 * L)
                    probs.append((xoff[key], roff, nr, L, voff, koff, rp["kernel"], rp["degree"], gamma,
                                  rp["coef0"], rp["tol"], mi, 0, 0, int(svr), 0, 0))
                    prob_of.append((ti, pi, key, fold))
                    ys.append(y_t.float()); Cs.append(C_t); Gs.append(G0); qds.append(qd.float())
                    voff += L; roff += nr; koff += 2 * nr
        P = np.array(probs, dtype=PROB_DTYPE)
        y_all = torch.cat(ys).float().contiguous()
        C_all = torch.cat(Cs).double().contiguous()
        G_all = torch.cat(Gs).double().contiguous()
        qd_all = torch.cat(qds).float().contiguous()
        a_all = torch.zeros_like(G_all)
        self._solve(data, P, Xrs, y_all, C_all, qd_all, a_all, G_all, koff)
        # ---- rho, decision values, predictions --------------------------------------------
        dec: Dict[Tuple[int, int], torch.Tensor] = {}
        cvdec: Dict[Tuple[int, int], torch.Tensor] = {}   # Platt: held-out values in the machine's row order
        models: Dict[int, list] = {}
        for k, (ti, pi, key, fold) in enumerate(prob_of):
            t = tasks[ti]
            rec = P[k]
            v0, L, nr = int(rec["voff"]), int(rec["L"]), int(rec["nrows"])
            a = a_all[v0:v0 + L]
            g = G_all[v0:v0 + L]
            y = y_all[v0:v0 + L].double()
            Cv = C_all[v0:v0 + L]
            rho = _rho(a, g, y, Cv)
            coef = (a[:nr] - a[nr:]) if svr else a * y
            sv = coef != 0
            rows = rowsets[key]
            Xsv = data.X[rows[sv]]
            if fold >= 0:   # an inner problem scores its held-out fifth of the machine's rows
                mrows = rowsets[key[:2]]
                ho = held[key[:3]][fold]
                te = mrows[ho]
            else:
                te = data.test_rows[t.split].long()
            K = _kernel_matrix(data.X[te], Xsv, int(rec["kernel"]), float(rec["gamma"]), float(rec["coef0"]),
                               int(rec["degree"]))
            dv = K @ coef[sv].to(K.dtype) - rho
            if fold >= 0:
                if (ti, pi) not in cvdec:
                    cvdec[(ti, pi)] = torch.zeros(mrows.numel(), dtype=torch.float64, device=dev)
                cvdec[(ti, pi)][ho] = dv.double()
            else:
                dec[(ti, pi)] = dv
                if keep_models:
                    models.setdefault(ti, []).append({"sv": Xsv.cpu().numpy(), "coef": coef[sv].cpu().numpy(),
                                                      "rho": float(rho), "pair": pairs[pi]})
            if int(rec["status"]) == 2:
                w = f"Solver terminated early (max_iter={int(rec['max_iter'])})"
                if w not in t.params["warnings"]:
                    t.params["warnings"].append(w)
        for (ti, pi, fold), v in const_dec.items():
            t, pr = tasks[ti], pairs[pi]
            mrows = rowsets[(t.split, pr)]
            sd = _task_platt_seed(t, pi)
            if (ti, pi) not in cvdec:
                cvdec[(ti, pi)] = torch.zeros(mrows.numel(), dtype=torch.float64, device=dev)
            cvdec[(ti, pi)][held[(t.split, pr, sd)][fold]] = v
        proba = self._probabilities(data, tasks, wants, pairs, rowsets, dec, cvdec, models)
        data.sync()
        dt = time.perf_counter() - t0
        outs = []
        for ti, t in enumerate(tasks):
            te = data.test_rows[t.split]
            if svr:
                pred = dec[(ti, 0)].float() if (ti, 0) in dec else torch.zeros(te.numel(), device=dev)
            else:
                votes = torch.zeros((te.numel(), C_cls), dtype=torch.int32, device=dev)
                for pi, (a_, b_) in enumerate(pairs):
                    dv = dec.get((ti, pi))
                    if dv is None:
                        continue
                    votes[:, a_] += (dv > 0).int()
                    votes[:, b_] += (dv <= 0).int()
                pred = votes.argmax(1).to(torch.int32)      # first max = lowest class (libsvm vote)
                if t.params.get("break_ties") and C_cls > 2:
                    pred = _ovr_argmax(dec, ti, pairs, te.numel(), C_cls, dev)
            o = FitOutput(task_id=t.task_id, pred=pred, fit_seconds=dt / len(tasks),
                          info={"warnings": t.params["warnings"]})
            if not svr and C_cls == 2 and (ti, 0) in dec:
                o.decision = -dec[(ti, 0)]   # sklearn's binary decision_function: positive -> classes_[1]
            if wants[ti] and _asks_proba(t):
                o.proba = proba[ti]
            if keep_models:
                rp = t.params
                o.model = {"kind": "svm", "svr": svr, "machines": models.get(ti, []), "kernel": rp["kernel"],
                           "gamma": float(self._gamma(data, t, rp["gamma"], {})), "coef0": rp["coef0"],
                           "degree": rp["degree"], "n_classes": C_cls,
                           "classes": None if svr else np.asarray(data.classes).tolist(), "model_type": t.model_type}
                if wants[ti]:
                    o.model["probability"] = True
            outs.append(o)
        return outs

    def _probabilities(self, data, tasks, wants, pairs, rowsets, dec, cvdec, models) -> Dict[int, torch.Tensor]:
        """Platt scaling + pairwise coupling of the fits in ``wants``: ONE sigmoid-fit launch
        over all their machines (csrc/kernels/svm_prob.hip ``k_platt_fit``; the host twin on
        the CPU), then one coupling launch per fit.  Stores probA / probB in the kept
        machines; returns {task index: [n_test, C] float64 probabilities}."""
        mach = [(ti, pi) for ti in range(len(tasks)) if wants[ti] for pi in range(len(pairs))]
        if not mach:
            return {}
        dev = data.device
        empty = torch.zeros(0, dtype=torch.float64, device=dev)
        decs, labs, off_len, off = [], [], [], 0
        for ti, pi in mach:
            dv = cvdec.get((ti, pi), empty)
            rows = rowsets[(tasks[ti].split, pairs[pi])]
            labs.append(torch.where(data.y_cls[rows] == pairs[pi][0], 1.0, -1.0).double().to(dev) if dv.numel()
                        else empty)
            decs.append(dv)
            off_len.append((off, dv.numel()))
            off += dv.numel()
        dec_all = torch.cat(decs).contiguous()
        lab_all = torch.cat(labs).contiguous()
        n = len(mach)
        ol = torch.tensor(off_len, dtype=torch.int64).reshape(n, 2).contiguous()
        AB = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        st = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        if data.is_gpu:
            lib = native.hip_lib()
            for fn in ("dml_svm_platt_fit", "dml_svm_pair_proba"):
                if getattr(lib, fn, None) is None:
                    raise RuntimeError(f"{fn} is missing from the HIP kernel library (stale build?)")
            ol = ol.to(dev)
            if dec_all.numel() == 0:   # keep the base pointers valid when every machine is empty
                dec_all = lab_all = torch.zeros(1, dtype=torch.float64, device=dev)
            if lib.dml_svm_platt_fit(native.ptr(dec_all), native.ptr(lab_all), native.ptr(ol), n, native.ptr(AB),
                                     native.ptr(st), native.stream_handle(dev)):
                raise RuntimeError("dml_svm_platt_fit launch failed")
        else:
            native.cpu_lib().dml_cpu_svm_platt_fit(native.ptr(dec_all), native.ptr(lab_all), native.ptr(ol), n,
                                                   native.ptr(AB), native.ptr(st))
        st_h, AB_h = st.cpu().numpy(), AB.cpu().numpy()
        kept = {(ti, tuple(m["pair"])): m for ti, ms in models.items() for m in ms}
        for q, (ti, pi) in enumerate(mach):
            if int(st_h[q, 1]) != PLATT_CONVERGED:
                w = ("Platt scaling: sigmoid fit reached the iteration limit (100)"
                     if int(st_h[q, 1]) == PLATT_ITER_CAP else "Platt scaling: sigmoid fit line search failed")
                if w not in tasks[ti].params["warnings"]:
                    tasks[ti].params["warnings"].append(w)
            m = kept.get((ti, tuple(pairs[pi])))
            if m is not None:
                m["probA"], m["probB"] = float(AB_h[q, 0]), float(AB_h[q, 1])
        # ---- coupling: one launch per fit ---------------------------------------------------
        out: Dict[int, torch.Tensor] = {}
        C_cls, npairs, q0 = data.n_classes, len(pairs), 0
        for ti, t in enumerate(tasks):
            if not wants[ti]:
                continue
            ABt = AB[q0:q0 + npairs].contiguous()
            q0 += npairs
            if not _asks_proba(t):
                continue   # a kept model only stores probA / probB
            m = int(data.test_rows[t.split].numel())
            D = torch.zeros((npairs, m), dtype=torch.float64, device=dev)
            for pi in range(npairs):
                if (ti, pi) in dec:
                    D[pi] = dec[(ti, pi)].double()
            pr = torch.empty((m, C_cls), dtype=torch.float64, device=dev)
            if data.is_gpu and C_cls <= PAIR_KERNEL_MAX_K:
                if m and native.hip_lib().dml_svm_pair_proba(native.ptr(D), native.ptr(ABt), m, C_cls, native.ptr(pr),
                                                             0, native.stream_handle(dev)):
                    raise RuntimeError("dml_svm_pair_proba launch failed")
            else:
                if data.is_gpu:
                    w = (f"pairwise coupling of {C_cls} classes (> {PAIR_KERNEL_MAX_K}) ran on the host from the "
                         f"copied decision values")
                    if w not in t.params["warnings"]:
                        t.params["warnings"].append(w)
                Dh, ABh, prh = D.cpu().contiguous(), ABt.cpu().contiguous(), torch.empty((m, C_cls), dtype=torch.float64)
                native.cpu_lib().dml_cpu_svm_pair_proba(native.ptr(Dh), native.ptr(ABh), m, C_cls, native.ptr(prh), 0)
                pr = prh.to(dev)
            out[ti] = pr
        return out

    def _solve(self, data, P, Xrs, y, C, qd, alpha, G, kbuf_len):
        if data.is_gpu:
            lib = native.hip_lib()
            if lib.dml_svm_sizeof_prob() != PROB_DTYPE.itemsize:
                raise RuntimeError("SvmProb layout mismatch")
            if os.environ.get("DML_SVM_SPLIT", "1") != "0" and self._solve_split(data, lib, P, Xrs, y, C, qd, alpha, G):
                return
            kbuf = torch.empty(max(1, kbuf_len), dtype=torch.float32, device=data.device)
            Pd = torch.from_numpy(P.view(np.uint8).copy()).to(data.device)
            while True:
                rc = lib.dml_svm_smo(native.ptr(Xrs), data.d, native.ptr(Pd), len(P), native.ptr(y), native.ptr(C),
                                     native.ptr(qd), native.ptr(alpha), native.ptr(G), native.ptr(kbuf), CHUNK_ITERS,
                                     native.stream_handle(data.device))
                if rc:
                    raise RuntimeError("dml_svm_smo launch failed")
                P[:] = Pd.cpu().numpy().view(PROB_DTYPE)
                if (P["status"] != 0).all():
                    break
            self.last_solve_stats = {"solver": "one workgroup per problem", "problems": len(P),
                                     "iterations_max": int(P["iters"].max())}
        else:
            lib = native.cpu_lib()
            if lib.dml_cpu_svm_sizeof_prob() != PROB_DTYPE.itemsize:
                raise RuntimeError("SvmProb layout mismatch")
            lib.dml_cpu_svm_smo(native.ptr(Xrs), data.d, native.ptr(P), len(P), native.ptr(y), native.ptr(C),
                                native.ptr(qd), native.ptr(alpha), native.ptr(G))
            self.last_solve_stats = {"solver": "host", "problems": len(P),
                                     "iterations_max": int(P["iters"].max()) if len(P) else 0}

    def _solve_split(self, data, lib, P, Xrs, y, C, qd, alpha, G) -> bool:
        """B workgroups per problem + per-problem LRU kernel-column caches
        (csrc/kernels/svm.hip ``k_smo_split``).  Every launch (a chunk of SMO iterations)
        re-splits the still-running problems over the resident workgroups, so the last
        hard problems (large C) end up with the most workgroups.  False: the split solver
        cannot run here (the caller uses the one-workgroup kernel)."""
        dev = data.device
        nprob = len(P)
        max_b, max_slots, wide_res = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        resident = int(lib.dml_svm_split_limits(ctypes.byref(max_b), ctypes.byref(max_slots), ctypes.byref(wide_res)))
        wide_ok = os.environ.get("DML_SVM_WIDE", "1") != "0"
        nr = P["nrows"].astype(np.int64)
        if resident <= 0 or nprob == 0:
            return False
        MB = int(max_b.value)
        free = torch.cuda.mem_get_info(dev)[0]
        cache_bytes = min(CACHE_FRACTION * free, float(os.environ.get("DML_SVM_CACHE_GB", CACHE_MAX_GB)) * 1e9)
        S = int(min(max_slots.value, int(nr.max()), cache_bytes // max(1, 4 * int(nr.sum()))))
        if os.environ.get("DML_SVM_CACHE_SLOTS"):   # tests: force evictions
            S = min(S, int(os.environ["DML_SVM_CACHE_SLOTS"]))
        if S < 2:
            return False
        P["coff"] = np.concatenate([[0], np.cumsum(nr * S)[:-1]])
        rep = nr + 2 * S                               # one workgroup's map: slot_of [nr], row_of [S], stamp [S]
        P["moff"] = np.concatenate([[0], np.cumsum(MB * rep)[:-1]])
        meta_np = np.full(int((MB * rep).sum()), -1, dtype=np.int32)
        for p in range(nprob):   # stamps start at 0: unused slots are the first victims
            for w in range(MB):
                st = int(P["moff"][p]) + w * int(rep[p]) + int(nr[p]) + S
                meta_np[st:st + S] = 0
        meta = torch.from_numpy(meta_np).to(dev)
        kc = torch.empty(int((nr * S).sum()), dtype=torch.float32, device=dev)
        prof = torch.zeros(8, dtype=torch.int64, device=dev) if os.environ.get("DML_SVM_PROFILE") else None
        launches, B_prev, B_hist, wide_n = 0, 0, [], 0
        while True:
            run = np.nonzero(P["status"] == 0)[0]
            if run.size == 0:
                break
            B = int(min(MB, max(1, resident // run.size), max(1, int(nr[run].max()) // MIN_ROWS_PER_WG)))
            if run.size * B > resident:
                B = 1   # no cross-workgroup waits at B = 1: any grid size is safe
            if launches and B != B_prev:
                # every replica of a problem's cache map is identical and every cached column
                # is complete (the old slices covered all rows): copy replica 0 to the new ones
                for p in run:
                    o, r_ = int(P["moff"][p]), int(rep[p])
                    view = meta[o:o + MB * r_].view(MB, r_)
                    view[1:B] = view[0]
            Pr = np.ascontiguousarray(P[run])
            Pd = torch.from_numpy(Pr.view(np.uint8).copy()).to(dev)
            recs = torch.zeros(run.size * 2 * B * 12, dtype=torch.int64, device=dev)   # svm.hip kRecW
            out_state = torch.zeros(2 * run.size, dtype=torch.int64, device=dev)
            # the wide sweep (8 variables per thread per step: one round trip per sweep for a
            # slice of <= 2048 rows) once the remaining problems fit its lower occupancy
            wide = int(wide_ok and (B == 1 or run.size * B <= int(wide_res.value))
                       and int(nr[run].max()) <= 8 * 256 * B)
            rc = lib.dml_svm_smo_split(native.ptr(Xrs), data.d, native.ptr(Pd), run.size, B, S, native.ptr(y),
                                       native.ptr(C), native.ptr(qd), native.ptr(alpha), native.ptr(G), native.ptr(kc),
                                       native.ptr(meta), native.ptr(recs), native.ptr(out_state), SPLIT_CHUNK_ITERS,
                                       native.ptr(prof), wide, native.stream_handle(dev))
            if rc == 4 and launches == 0:
                return False
            if rc:
                raise RuntimeError(f"dml_svm_smo_split failed ({rc})")
            launches += 1
            wide_n += wide
            B_prev = B
            B_hist.append(B)
            st = out_state.view(run.size, 2).cpu().numpy()
            P["iters"][run] = st[:, 0]
            P["status"][run] = st[:, 1]
            if (P["status"] == 3).any():
                raise RuntimeError("SMO workgroups of a problem lost contact (not co-resident?)")
        self.last_solve_stats = {"solver": "split", "problems": nprob, "workgroups_per_problem": max(B_hist),
                                 "wide_launches": wide_n,
                                 "workgroups_per_launch": B_hist, "cache_slots": S, "launches": launches,
                                 "iterations_max": int(P["iters"].max()), "iterations_sum": int(P["iters"].sum())}
        if prof is not None:   # first running problem, workgroup 0: 100 MHz ticks -> microseconds per phase
            pr = prof.cpu().numpy()
            names = ("i_reduce", "xchg_i", "col_i", "j_sweep", "xchg_j", "col_j_update", "g_sweep")
            self.last_solve_stats["phase_us"] = {k: round(float(pr[q]) / 100.0, 1) for q, k in enumerate(names)}
            self.last_solve_stats["cache_misses"] = int(pr[7])
        return True

    @staticmethod
    def _gamma(data, t: FitTask, gamma, cache: Dict[int, float]) -> float:
        if not isinstance(gamma, str):
            return float(gamma)
        if gamma == "auto":
            return 1.0 / data.d
        if t.split not in cache:
            Xt = data.X[data.train_rows[t.split].long()].double()
            var = float(Xt.var(unbiased=False)) if Xt.numel() else 0.0
            cache[t.split] = 1.0 / (data.d * var) if var != 0 else 1.0
        return cache[t.split]

    @staticmethod
    def _class_weights(data, t: FitTask, cw) -> torch.Tensor:
        C = data.n_classes
        w = torch.ones(C, dtype=torch.float64, device=data.device)
        if cw is None:
            return w
        if cw == "balanced":
            yt = data.y_cls[data.train_rows[t.split].long()].long()
            cnt = torch.bincount(yt, minlength=C).double()
            return torch.where(cnt > 0, yt.numel() / (C * cnt.clamp_min(1)), torch.ones_like(cnt))
        lookup = {str(c): i for i, c in enumerate(np.asarray(data.classes).tolist())}
        for k, v in cw.items():
            if str(k) in lookup:
                w[lookup[str(k)]] = float(v)
        return w

    @staticmethod
    def _diag(norm2: torch.Tensor, kernel: int, gamma: float, coef0: float, degree: int) -> torch.Tensor:
        if kernel == KRBF:
            return torch.ones_like(norm2)
        if kernel == KLIN:
            return norm2
        if kernel == KPOLY:
            return (gamma * norm2 + coef0) ** degree
        return torch.tanh(gamma * norm2 + coef0)


def _rho(a, g, y, C) -> float:
    """libsvm Solver::calculate_rho."""
    yG = y * g
    upper = a >= C
    lower = a <= 0
    free = ~upper & ~lower
    if bool(free.any()):
        return float(yG[free].mean())
    ub_mask = (upper & (y < 0)) | (lower & (y > 0))
    lb_mask = (upper & (y > 0)) | (lower & (y < 0))
    ub = float(yG[ub_mask].min()) if bool(ub_mask.any()) else math.inf
    lb = float(yG[lb_mask].max()) if bool(lb_mask.any()) else -math.inf
    return (ub + lb) / 2


def _kernel_matrix(A: torch.Tensor, B: torch.Tensor, kernel: int, gamma: float, coef0: float, degree: int):
    dt = torch.float64 if A.shape[0] * max(1, B.shape[0]) <= 50_000_000 else torch.float32
    A, B = A.to(dt), B.to(dt)
    if kernel == KRBF:
        d2 = (A * A).sum(1, keepdim=True) + (B * B).sum(1)[None, :] - 2.0 * (A @ B.t())
        return torch.exp(-gamma * d2.clamp_min(0))
    dot = A @ B.t()
    if kernel == KLIN:
        return dot
    if kernel == KPOLY:
        return (gamma * dot + coef0) ** degree
    return torch.tanh(gamma * dot + coef0)


def _machine_decisions(model: Dict[str, Any], X: np.ndarray) -> List[np.ndarray]:
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    decs = []
    for m in model["machines"]:
        sv = torch.from_numpy(np.asarray(m["sv"], dtype=np.float32).reshape(-1, Xt.shape[1]))
        K = _kernel_matrix(Xt, sv, int(model["kernel"]), float(model["gamma"]), float(model["coef0"]),
                           int(model["degree"]))
        decs.append((K @ torch.from_numpy(np.asarray(m["coef"], dtype=np.float64)).to(K.dtype) - m["rho"]).numpy())
    return decs


def svm_has_proba(model: Dict[str, Any]) -> bool:
    """The artefact was fitted with probability=True (its machines carry probA / probB)."""
    ms = model.get("machines") or []
    return not model.get("svr") and bool(ms) and all("probA" in m and "probB" in m for m in ms)


def svm_proba_numpy(model: Dict[str, Any], X: np.ndarray) -> np.ndarray:
    """Class probabilities [len(X), n_classes] of an SVC artefact on the CPU: each machine's
    decision value through its sigmoid, then the pairwise coupling of the host routine
    (csrc/runtime/svm_prob_cpu.cpp).  Columns follow ``model['classes']``."""
    if not svm_has_proba(model):
        raise AttributeError(_NO_PROBA)
    k, m = int(model["n_classes"]), len(X)
    pair_index = {(a, b): i for i, (a, b) in enumerate((a, b) for a in range(k) for b in range(a + 1, k))}
    D = np.zeros((len(pair_index), m), dtype=np.float64)   # a pair without a machine: r = 1/2
    AB = np.zeros((len(pair_index), 2), dtype=np.float64)
    for mach, dv in zip(model["machines"], _machine_decisions(model, X)):
        i = pair_index[tuple(int(c) for c in mach["pair"])]
        D[i] = dv
        AB[i] = (float(mach["probA"]), float(mach["probB"]))
    out = np.empty((m, k), dtype=np.float64)
    native.cpu_lib().dml_cpu_svm_pair_proba(native.ptr(D), native.ptr(AB), m, k, native.ptr(out), 0)
    return out


def svm_predict_numpy(model: Dict[str, Any], X: np.ndarray) -> np.ndarray:
    decs = _machine_decisions(model, X)
    if model["svr"]:
        return decs[0] if decs else np.zeros(len(X))
    C = int(model["n_classes"])
    votes = np.zeros((len(X), C), dtype=np.int64)
    for m, dv in zip(model["machines"], decs):
        a, b = m["pair"]
        votes[:, a] += dv > 0
        votes[:, b] += dv <= 0
    return np.asarray(model["classes"])[votes.argmax(1)]


register(SVMFamily())
