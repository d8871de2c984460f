"""Strategic classification (the reference's strategic.py: cost functions, best response, strategic loss, robustness
evaluation) with the best-response search and the strategic loss on MI355X (csrc/strategic.hip, ac_head_fwd_bwd_strategic).

The reference tries the candidate moves of `_generate_candidates` one single-row head forward at a time.  Here a whole batch of
queries is searched in one native call (`best_response_batch`): the candidate table is shared (x itself, then x[i] += delta for
i = 0, 1, ... and the ten values of torch.linspace(-2, 2, 10) (none is 0), cut at 50), the utilities are
max(softmax(head(y))) - cost(x, y) and the FIRST maximum wins, as in the reference's strict `>` scan.  With fewer than 5
features the reference pads the table with torch.randn candidates; that form is not built (NativeError).

Cost functions keep the reference's public formulas (`compute_cost`).  In the search both cost types reduce to
relu(c_f * dy) for a single-coordinate move (csrc/strategic.hip documents the bound against the reference's two fp32 dots).
"""
import ctypes
import logging
from abc import ABC, abstractmethod
from typing import Dict, List, Optional, Union

import torch

from . import _native as nv

logger = logging.getLogger(__name__)

NUM_CANDIDATES = 50
COST_SEPARABLE, COST_LINEAR = 0, 1                    # AC_STRAT_COST_*
MASK_NONE, MASK_EXPLICIT, MASK_SEED = 0, 1, 2         # AC_STRAT_MASK_*


def candidate_table(dim: int, num_candidates: int = NUM_CANDIDATES):
    """(features int32 [M], deltas fp32 [M]) of the reference's deterministic candidates for a `dim`-feature input: entry 0 is
    x itself (feature -1), then (i, delta) for i = 0, 1, ... and delta in torch.linspace(-2, 2, 10) without 0, cut at
    num_candidates.  Raises NativeError where the reference would draw random candidates (fewer than that many moves)."""
    deltas = [d for d in torch.linspace(-2.0, 2.0, 10) if d != 0]
    feats, vals = [-1], [0.0]
    for i in range(dim):
        for d in deltas:
            if len(feats) >= num_candidates:
                break
            feats.append(i)
            vals.append(float(d))
        if len(feats) >= num_candidates:
            break
    if len(feats) < num_candidates:
        raise nv.NativeError("strategic best response: %d features give only %d deterministic candidates; the reference fills "
                             "the table with random ones, which this build does not implement (needs >= 5 features)"
                             % (dim, len(feats)))
    return torch.tensor(feats, dtype=torch.int32), torch.tensor(vals, dtype=torch.float32)


_TABLES = {}


def _device_table(dim, device):
    key = (dim, str(device))
    t = _TABLES.get(key)
    if t is None:
        f, d = candidate_table(dim)
        t = _TABLES[key] = (f.to(device), d.to(device))
    return t


def best_response_batch(X: torch.Tensor, head=None, num_classes: Optional[int] = None, coef: torch.Tensor = None,
                        cost_type: int = COST_SEPARABLE, mask_mode: int = MASK_NONE, masks=None, seed: int = 0,
                        dropout_p: float = 0.1, want_logits: bool = False, want_all: bool = False):
    """Best responses of the rows of X [b, D] (one `ac_strategic_best_response` call) against `head` (an AdaptiveHead;
    None = uniform f over num_classes).  masks: (uint8 [b, M, H1], uint8 [b, M, H2]) for MASK_EXPLICIT; seed for MASK_SEED.
    Returns dict(choice int32 [b], util [b], Y [b, D], util_all [b, M] | None, logits [b, C] | None)."""
    nv.require_gpu()
    if head is not None:
        flat = head.flat_params()
        dev = flat.device
        dims = head.native_dims()
        if dims is None:
            raise nv.NativeError("strategic best response needs an AdaptiveHead with two hidden layers")
    else:
        dev = X.device if X.is_cuda else torch.device("cuda")
        flat = None
        D = X.shape[1]
        dims = nv.ac_head_dims(D, 1, 1, int(num_classes or 1))
    X = X.to(device=dev, dtype=torch.float32).contiguous()
    b, D = X.shape
    if D != dims.D:
        raise nv.NativeError("strategic best response: rows have %d features, the head takes %d" % (D, dims.D))
    coef = _check_coef(coef, D).to(dev)
    feat, delta = _device_table(D, dev)
    M = int(feat.numel())
    out = {"choice": torch.empty(b, dtype=torch.int32, device=dev), "util": torch.empty(b, dtype=torch.float32, device=dev),
           "Y": torch.empty(b, D, dtype=torch.float32, device=dev),
           "util_all": torch.empty(b, M, dtype=torch.float32, device=dev) if want_all else None,
           "logits": torch.empty(b, dims.C, dtype=torch.float32, device=dev) if (want_logits and head is not None) else None}
    m1 = m2 = None
    if mask_mode == MASK_EXPLICIT:
        m1, m2 = (m.to(device=dev, dtype=torch.uint8).contiguous() for m in masks)
        if m1.numel() != b * M * dims.H1 or m2.numel() != b * M * dims.H2:
            raise nv.NativeError("strategic best response: masks must be [b, %d, H1] and [b, %d, H2]" % (M, M))
    need = ctypes.c_size_t(0)
    nv.check(nv.lib().ac_strategic_workspace(ctypes.byref(dims), b, M, ctypes.byref(need)), "ac_strategic_workspace")
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nv.check(nv.lib().ac_strategic_best_response(
            ctypes.byref(dims), nv.ptr(flat), nv.ptr(X), X.stride(0), b, nv.ptr(feat), nv.ptr(delta), M, nv.ptr(coef),
            cost_type, mask_mode, nv.ptr(m1), nv.ptr(m2), float(dropout_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
            nv.ptr(out["choice"]), nv.ptr(out["util"]), nv.ptr(out["util_all"]), nv.ptr(out["Y"]), D, nv.ptr(out["logits"]),
            nv.ptr(ws), ws.numel(), nv.stream_ptr(dev)), "ac_strategic_best_response")
    return out


def _check_coef(coef, D):
    """The reference's torch.dot(c, x) raises unless c is a float32 vector of x's length: the same conditions, the same error
    type (RuntimeError), before anything runs."""
    if coef is None:
        raise RuntimeError("strategic best response: no cost coefficients")
    c = coef if isinstance(coef, torch.Tensor) else torch.tensor(coef)
    if c.dim() != 1 or c.numel() != D:
        raise RuntimeError("inconsistent tensor size: cost coefficients have %d elements, the embedding %d" % (c.numel(), D))
    if c.dtype != torch.float32:
        raise RuntimeError("dot : expected both vectors to have same dtype, but found %s and Float" % (c.dtype,))
    return c.detach().contiguous()


class StrategicCostFunction(ABC):
    """Abstract base class for strategic cost functions."""

    @abstractmethod
    def compute_cost(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Cost of moving from x to y."""

    @abstractmethod
    def compute_best_response(self, x: torch.Tensor, f) -> torch.Tensor:
        """Best response of x against the classifier f."""


class SeparableCostFunction(StrategicCostFunction):
    """c(x, y) = max{0, c2 . y - c1 . x}."""

    cost_type = COST_SEPARABLE

    def __init__(self, c1_coefficients: Union[Dict[str, float], torch.Tensor], c2_coefficients: Union[Dict[str, float], torch.Tensor],
                 feature_names: Optional[List[str]] = None):
        if isinstance(c1_coefficients, dict) and isinstance(c2_coefficients, dict):
            if feature_names is None:
                raise ValueError("feature_names required when using dict coefficients")
            self.c1 = torch.tensor([c1_coefficients.get(name, 0.0) for name in feature_names])
            self.c2 = torch.tensor([c2_coefficients.get(name, 0.0) for name in feature_names])
        else:
            self.c1 = c1_coefficients if isinstance(c1_coefficients, torch.Tensor) else torch.tensor(c1_coefficients)
            self.c2 = c2_coefficients if isinstance(c2_coefficients, torch.Tensor) else torch.tensor(c2_coefficients)
        self.feature_names = feature_names

    def compute_cost(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return torch.relu(torch.dot(self.c2.to(y.device), y) - torch.dot(self.c1.to(x.device), x))

    def search_coefficients(self) -> torch.Tensor:
        """The per-feature coefficient of the native search (single-coordinate moves: cost = relu(c_f dy) needs c1 == c2)."""
        if self.c1 is not self.c2 and not (self.c1.shape == self.c2.shape and torch.equal(self.c1, self.c2)):
            raise nv.NativeError("strategic best response: the native search covers c1 == c2 (the factory's separable form)")
        return self.c2

    def compute_best_response(self, x: torch.Tensor, f=None, num_classes: Optional[int] = None) -> torch.Tensor:
        """Best response of ONE embedding x [D] against f = an AdaptiveHead (eval mode, as predict_strategic runs it) or None
        (uniform f over num_classes): one native search call.  Other callables are not searched natively (NativeError)."""
        from .models import AdaptiveHead
        if f is not None and not isinstance(f, AdaptiveHead):
            raise nv.NativeError("compute_best_response: pass the AdaptiveHead (or None for a uniform classifier); arbitrary "
                                 "callables are not searched natively")
        res = best_response_batch(x.reshape(1, -1), f, num_classes, self.search_coefficients(), self.cost_type)
        return res["Y"][0].to(x.device)

    def _generate_candidates(self, x: torch.Tensor, num_candidates: int = NUM_CANDIDATES) -> List[torch.Tensor]:
        """The candidate rows themselves (host tensors; the native search uses `candidate_table`)."""
        feats, deltas = candidate_table(len(x), num_candidates)
        out = []
        for f, d in zip(feats.tolist(), deltas):
            c = x.clone()
            if f >= 0:
                c[f] += d
            out.append(c)
        return out


class LinearCostFunction(SeparableCostFunction):
    """c(x, y) = <alpha, y - x>_+."""

    cost_type = COST_LINEAR

    def __init__(self, alpha: Union[Dict[str, float], torch.Tensor], feature_names: Optional[List[str]] = None):
        if isinstance(alpha, dict):
            if feature_names is None:
                raise ValueError("feature_names required when using dict coefficients")
            alpha_tensor = torch.tensor([alpha.get(name, 0.0) for name in feature_names])
        else:
            alpha_tensor = alpha if isinstance(alpha, torch.Tensor) else torch.tensor(alpha)
        super().__init__(alpha_tensor, alpha_tensor, feature_names)
        self.alpha = alpha_tensor

    def compute_cost(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return torch.relu(torch.dot(self.alpha.to(x.device), y - x))


class CostFunctionFactory:
    """Cost functions from configuration ("linear" | "separable")."""

    @staticmethod
    def create_cost_function(cost_type: str, cost_coefficients, feature_names: Optional[List[str]] = None,
                             **kwargs) -> StrategicCostFunction:
        if cost_type == "linear":
            return LinearCostFunction(cost_coefficients, feature_names)
        elif cost_type == "separable":
            c2_coefficients = kwargs.get("c2_coefficients", cost_coefficients)
            return SeparableCostFunction(cost_coefficients, c2_coefficients, feature_names)
        raise ValueError(f"Unknown cost function type: {cost_type}")


class StrategicOptimizer:
    """The strategic loss: CE_mean(batch) + lambda * sum over mispredicted best responses of their CE / B, forward and backward
    in one native call over [x; y] (`ac_head_fwd_bwd_strategic`)."""

    def __init__(self, cost_function: StrategicCostFunction):
        self.cost_function = cost_function

    def strategic_loss(self, trainer, embeddings: torch.Tensor, labels: torch.Tensor, strategic_lambda: float = 0.1,
                       masks=None, seed: int = 0, dropout_p: float = 0.1):
        """One batch: best responses (train-mode head: `masks` = ((m1 [B, M, H1], m2 [B, M, H2]) of the candidate forwards,
        (m1 [2B, H1], m2 [2B, H2]) of the [x; y] forward) drawn by the caller, or counter-based masks from `seed`), then the
        loss's forward + backward into trainer.grads.  Returns (loss device scalar, best-response choices int32 [B],
        misprediction flags int32 [B])."""
        X = embeddings.to(device=trainer.device, dtype=torch.float32).contiguous()
        y = labels.to(device=trainer.device, dtype=torch.int64).contiguous()
        B = X.shape[0]
        cf = self.cost_function
        if masks is not None:
            br = best_response_batch(X, trainer.head, coef=cf.search_coefficients(), cost_type=cf.cost_type,
                                     mask_mode=MASK_EXPLICIT, masks=masks[0], dropout_p=dropout_p)
        else:
            br = best_response_batch(X, trainer.head, coef=cf.search_coefficients(), cost_type=cf.cost_type,
                                     mask_mode=MASK_SEED, seed=seed, dropout_p=dropout_p)
        X2 = torch.cat([X, br["Y"]])
        m1 = m2 = None
        if masks is not None:
            m1, m2 = (m.to(device=trainer.device, dtype=torch.uint8).contiguous() for m in masks[1])
        mis = torch.empty(B, dtype=torch.int32, device=trainer.device)
        ws = trainer._workspace(2 * B)
        with torch.cuda.device(trainer.device):
            nv.check(nv.lib().ac_head_fwd_bwd_strategic(
                ctypes.byref(trainer.dims), nv.ptr(trainer.flat), nv.ptr(X2), X2.stride(0), nv.ptr(y), nv.ptr(m1), nv.ptr(m2),
                float(dropout_p), 0 if masks is not None else 1, (int(seed) ^ 0x5DEECE66D) & 0xFFFFFFFFFFFFFFFF, B,
                float(strategic_lambda), nv.ptr(trainer.loss), nv.ptr(trainer.grads), nv.ptr(mis), nv.ptr(ws), ws.numel(),
                nv.stream_ptr(trainer.device)), "ac_head_fwd_bwd_strategic")
        return trainer.loss, br["choice"], mis


class StrategicEvaluator:
    """Robustness under strategic behaviour (the reference's evaluate_robustness): per gaming level, each embedding draws ONE
    torch.rand(1) on the global CPU generator and is replaced by its best response when the draw is below the level; the
    accuracy is that of the head's argmax over all rows."""

    def __init__(self, cost_function: StrategicCostFunction):
        self.cost_function = cost_function

    def evaluate_robustness(self, classifier, test_embeddings: torch.Tensor, test_labels: torch.Tensor,
                            gaming_levels: List[float] = [0.0, 0.5, 1.0], replay: bool = False, seed: int = 0) -> Dict[str, float]:
        """classifier: the AdaptiveHead, run in the train / eval state it is in (train: dropout in every forward -- masks drawn
        on the host in the reference's order when `replay`, else counter-based from `seed`)."""
        head = classifier
        if head is None:
            raise TypeError("'NoneType' object is not callable")
        cf = self.cost_function
        coef = cf.search_coefficients()
        dims = head.native_dims()
        train = bool(head.training)
        p = head.DROPOUT_P
        X = test_embeddings.to(torch.float32)
        n = X.shape[0]
        labels = test_labels.to(torch.int64).cpu()
        results = {}
        for li, level in enumerate(gaming_levels):
            chosen, cmasks = [], ([], [])
            for i in range(n):
                if torch.rand(1).item() < level:
                    chosen.append(i)
                    if train and replay:         # the 50 single-row candidate forwards of this embedding, in order
                        M = NUM_CANDIDATES
                        ms = [(torch.empty(1, dims.H1).bernoulli_(1 - p), torch.empty(1, dims.H2).bernoulli_(1 - p)) for _ in range(M)]
                        cmasks[0].append(torch.cat([a for a, _ in ms]))
                        cmasks[1].append(torch.cat([b for _, b in ms]))
            Xs = X.to(head.flat_params().device).contiguous().clone()
            if chosen:
                idx = torch.tensor(chosen, dtype=torch.long, device=Xs.device)
                if not train:
                    br = best_response_batch(Xs.index_select(0, idx), head, coef=coef, cost_type=cf.cost_type)
                elif replay:
                    br = best_response_batch(Xs.index_select(0, idx), head, coef=coef, cost_type=cf.cost_type,
                                             mask_mode=MASK_EXPLICIT, masks=(torch.stack(cmasks[0]), torch.stack(cmasks[1])),
                                             dropout_p=p)
                else:
                    br = best_response_batch(Xs.index_select(0, idx), head, coef=coef, cost_type=cf.cost_type,
                                             mask_mode=MASK_SEED, seed=seed * 1000003 + li, dropout_p=p)
                Xs.index_copy_(0, idx, br["Y"])
            logits = self._head_logits(head, Xs, train, replay, seed * 1000003 + li + 7919, coef, cf.cost_type)
            predictions = torch.argmax(logits.cpu(), dim=-1)
            results[f"accuracy_gaming_{level}"] = (predictions == labels).float().mean().item()
        results["robustness_score"] = results["accuracy_gaming_0.0"] - results["accuracy_gaming_1.0"]
        results["relative_robustness"] = results["accuracy_gaming_1.0"] / results["accuracy_gaming_0.0"]
        return results

    @staticmethod
    def _head_logits(head, X, train, replay, seed, coef, cost_type):
        """head(X) in its state: eval -> forward_native; train -> the one-candidate form of the search kernel (identity move
        only) with the layer masks of that forward."""
        if not train:
            return head.forward_native(X)
        n = X.shape[0]
        dims = head.native_dims()
        p = head.DROPOUT_P
        if replay:
            m1 = torch.empty(n, dims.H1).bernoulli_(1 - p)
            m2 = torch.empty(n, dims.H2).bernoulli_(1 - p)
        out = {"logits": torch.empty(n, dims.C, dtype=torch.float32, device=X.device)}
        feat = torch.tensor([-1], dtype=torch.int32, device=X.device)
        delta = torch.zeros(1, dtype=torch.float32, device=X.device)
        choice = torch.empty(n, dtype=torch.int32, device=X.device)
        util = torch.empty(n, dtype=torch.float32, device=X.device)
        Y = torch.empty_like(X)
        need = ctypes.c_size_t(0)
        nv.check(nv.lib().ac_strategic_workspace(ctypes.byref(dims), n, 1, ctypes.byref(need)), "ac_strategic_workspace")
        ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=X.device)
        c = coef.to(X.device)
        mm = (m1.to(torch.uint8).to(X.device), m2.to(torch.uint8).to(X.device)) if replay else (None, None)
        with torch.cuda.device(X.device):
            nv.check(nv.lib().ac_strategic_best_response(
                ctypes.byref(dims), nv.ptr(head.flat_params()), nv.ptr(X), X.stride(0), n, nv.ptr(feat), nv.ptr(delta), 1,
                nv.ptr(c), cost_type, MASK_EXPLICIT if replay else MASK_SEED, nv.ptr(mm[0]), nv.ptr(mm[1]), float(p),
                int(seed) & 0xFFFFFFFFFFFFFFFF, nv.ptr(choice), nv.ptr(util), None, nv.ptr(Y), X.shape[1], nv.ptr(out["logits"]),
                nv.ptr(ws), ws.numel(), nv.stream_ptr(X.device)), "ac_strategic_best_response")
        return out["logits"]
