"""Synthetic inputs for the gradient-boosting stage statistics (shared by test_gbrt_staged.py and
test_gbrt_staged_gpu.py; not a test module).  ``make_case`` draws raw scores, targets, split
roles, in-bag and validation masks for several fits of one data set; ``run_case`` runs
``gbrt_ops.stage_stats`` on them on a device and returns the host copies of ``stats`` and of the
block partials."""
import numpy as np
import torch

from cs230_distributed_machine_learning_amd.ops import gbrt_ops

SQ, ABS, HUBER, QUANT, LOG, EXP = range(6)
CLS_MIX = [LOG, EXP, LOG, EXP, LOG]
REG_MIX = [SQ, ABS, HUBER, QUANT, HUBER]


def make_case(n, K, losses, seed=0, mode="normal", empty_oob=False, with_val=True, n_splits=3):
    """mode: "normal" (N(0, 3^2) raw scores), "big" (|raw| up to 800; 700 for fits of the
    exponential loss, whose term exp(|raw|) is not finite above 709), "ties" (multiples of 0.25
    from a small range: exact zeros for the binary rule, exact ties for the first-maximum rule)."""
    rng = np.random.RandomState(seed)
    F = len(losses)
    is_cls = losses[0] in (LOG, EXP)
    assert all((l in (LOG, EXP)) == is_cls for l in losses) and (K == 1 or all(l == LOG for l in losses))
    if mode == "big":
        raw = rng.uniform(-800.0, 800.0, size=(F, K, n))
        raw[:, :, : min(n, 2 * K)] = np.where(rng.rand(F, K, min(n, 2 * K)) < 0.5, 800.0, -800.0)
        for f, l in enumerate(losses):
            if l == EXP:
                raw[f] = np.clip(raw[f], -700.0, 700.0)
    elif mode == "ties":
        raw = rng.randint(-3, 4, size=(F, K, n)) * 0.25
    else:
        raw = rng.normal(size=(F, K, n)) * 3.0
    if is_cls:
        y = rng.randint(0, max(2, K), size=n).astype(np.int32)
    else:
        y = (rng.normal(size=n) * (300.0 if mode == "big" else 3.0)).astype(np.float64)
        if mode == "ties":
            y = np.round(y * 4) / 4
    roles = rng.randint(0, 3, size=(n_splits, n)).astype(np.uint8)
    inbag = np.ones((F, n), np.uint8) if empty_oob else (rng.rand(F, n) < 0.6).astype(np.uint8)
    val = (rng.rand(F, n) < 0.15).astype(np.uint8)   # drawn either way: the later draws do not depend on with_val
    val = val if with_val else None
    fit_val = np.array([f if (with_val and f % 2 == 0) else -1 for f in range(F)])
    return {"n": n, "K": K, "F": F, "loss": np.asarray(losses), "is_cls": is_cls, "raw": raw.reshape(F * K, n), "y": y,
            "roles": roles, "inbag": inbag, "val": val, "fit_val": fit_val, "fit_role": rng.randint(0, n_splits, size=F),
            "alpha": rng.uniform(0.1, 0.9, size=F), "delta": rng.uniform(0.5, 2.0, size=F) * (100.0 if mode == "big" else 1.0),
            "n_splits": n_splits}


def categories(c, f):
    """Boolean row masks (in-bag, out-of-bag, held-out) of fit f."""
    role = c["roles"][c["fit_role"][f]]
    isval = c["val"][c["fit_val"][f]] != 0 if (c["val"] is not None and c["fit_val"][f] >= 0) else np.zeros(c["n"], bool)
    tr = (role == 1) & ~isval
    return [tr & (c["inbag"][f] != 0), tr & (c["inbag"][f] == 0), role == 2]


def run_case(c, device, stage=1, n_stages=3, part=None):
    """(stats int64 [F][n_stages][3][3], part int64 [blocks][F][3][3]) as numpy arrays."""
    F, K, n = c["F"], c["K"], c["n"]
    dev = torch.device(device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev).contiguous()   # noqa: E731
    plan = gbrt_ops.stats_plan(np.arange(F) * K, c["loss"], c["fit_role"], np.arange(F), c["fit_val"], np.arange(F),
                               np.arange(F), c["alpha"], K=K, raw_rows=F * K, role_rows=c["n_splits"], inbag_rows=F,
                               val_rows=0 if c["val"] is None else F, stat_fits=F, delta_len=F, device=dev)
    stats = gbrt_ops.new_stats(F, n_stages, dev)
    y = t(c["y"], torch.int32 if c["is_cls"] else torch.float64)
    part = gbrt_ops.stage_stats(t(c["raw"], torch.float64), y, t(c["roles"], torch.uint8), t(c["inbag"], torch.uint8),
                                None if c["val"] is None else t(c["val"], torch.uint8), plan,
                                t(c["delta"], torch.float64), stats, stage, part)
    blocks = (n + 255) // 256
    return stats.cpu().numpy(), part[:blocks * F * 9].cpu().numpy().reshape(blocks, F, 3, 3)
