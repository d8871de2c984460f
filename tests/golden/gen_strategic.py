"""Generate tests/golden/strategic_bert_mini.json / .npz: the STRATEGIC-MODE differential.

    python tests/golden/gen_strategic.py        # build container only (/root/reference present); CPU

Runs the UNMODIFIED reference on CPU the way gen_e2e_train.py does (oracle.hub_standin, oracle.faiss_shim, the bert-mini
stand-in): `AdaptiveClassifier(name, config={"enable_strategic_mode": True, "cost_coefficients": [D floats],
"strategic_training_frequency": 1})`, one `add_examples` call (regular training, then the strategic training step), then
`predict` (dual), `predict_strategic`, `predict_robust` and `evaluate_strategic_robustness` at levels [0, 0.5, 1].  It records
by observation only (the best-response search's classifier function and the strategic loss are wrapped to log what they
return; nothing the reference computes is changed):
  * every best-response decision: the candidate table as (feature, delta), all 50 utilities and the chosen index;
  * the per-step strategic losses and the final head parameters (.npz);
  * the prediction lists and the robustness metrics.
Every recorded decision has a top-2 utility margin >= 1e-4 (asserted), so the product's fp32 search must choose the same."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import faiss_shim, hub_standin  # noqa: E402

faiss_shim.install()
hub_standin.install()
sys.path.insert(0, "/root/reference/src")
import adaptive_classifier as ref  # noqa: E402
from adaptive_classifier import strategic as ref_strategic  # noqa: E402
import gen_e2e  # noqa: E402

assert ref.__file__.startswith("/root/reference"), ref.__file__

MARGIN = 1e-4
COEF_SEED = 7
COEF_SCALE = 0.05
N_TRAIN = 12          # examples of the add_examples call (every other text of TRAIN_1: one batch of 12 per strategic epoch)
K = 3


def coefficients(D):
    g = np.random.default_rng(COEF_SEED)
    return [float(v) for v in (g.standard_normal(D) * COEF_SCALE).astype(np.float32)]


def main():
    decisions, losses = [], []
    orig_br = ref_strategic.SeparableCostFunction.compute_best_response
    orig_loss = ref_strategic.StrategicOptimizer.strategic_loss

    def logging_br(self, x, f):
        outs = []

        def f_logged(c):
            o = f(c)
            outs.append(o.detach().clone())
            return o
        y = orig_br(self, x, f_logged)
        cands = self._generate_candidates(x)
        util = []
        for c, o in zip(cands, outs):
            fm = torch.max(o.squeeze())
            util.append(float(fm - self.compute_cost(x, c)))
        nominal = [float(v) for v in torch.linspace(-2.0, 2.0, 10) if v != 0]
        table = []
        for i, c in enumerate(cands):                 # (feature moved, nominal delta: the i-th of the linspace loop)
            d = (c - x).nonzero().flatten().tolist()
            table.append([-1, 0.0] if i == 0 else [d[0] if d else -2, nominal[(i - 1) % len(nominal)]])
        choice = next(i for i, c in enumerate(cands) if torch.equal(c, y))
        decisions.append({"util": util, "choice": choice, "table": table})
        return y

    def logging_loss(self, model, embeddings, labels, strategic_lambda=0.1):
        out = orig_loss(self, model, embeddings, labels, strategic_lambda)
        losses.append(float(out.detach()))
        return out

    ref_strategic.SeparableCostFunction.compute_best_response = logging_br
    ref_strategic.StrategicOptimizer.strategic_loss = logging_loss
    try:
        torch.manual_seed(0)
        np.random.seed(0)
        probe = ref.AdaptiveClassifier(gen_e2e.NAME, device="cpu", use_onnx=False)
        D = probe.embedding_dim
        coefs = coefficients(D)
        torch.manual_seed(0)
        np.random.seed(0)
        cfg = {"enable_strategic_mode": True, "cost_coefficients": coefs, "strategic_training_frequency": 1}
        clf = ref.AdaptiveClassifier(gen_e2e.NAME, device="cpu", use_onnx=False, config=cfg)
        assert clf.strategic_mode
        train = gen_e2e.TRAIN_1[::2]
        clf.add_examples([t for t, _ in train], [l for _, l in train])
        train_decisions = list(decisions)
        decisions.clear()
        head = {k: v.detach().numpy().copy() for k, v in clf.adaptive_head.state_dict().items()}
        queries = gen_e2e.QUERIES[:16]
        pred_dual, pred_strat, pred_robust, strat_dec = [], [], [], []
        for q in queries:
            pred_dual.append(clf.predict(q, k=K))
            pred_strat.append(clf.predict_strategic(q, k=K))
            strat_dec.append(decisions[-1])
            pred_robust.append(clf.predict_robust(q, k=K))
        decisions.clear()
        torch.manual_seed(123)
        ev_texts = [t for t, _ in gen_e2e.TRAIN_1]
        ev_labels = [l for _, l in gen_e2e.TRAIN_1]
        assert not clf.adaptive_head.training        # (predict left the head in eval mode)
        robust = clf.evaluate_strategic_robustness(ev_texts, ev_labels, [0.0, 0.5, 1.0])
        eval_decisions = list(decisions)
    finally:
        ref_strategic.SeparableCostFunction.compute_best_response = orig_br
        ref_strategic.StrategicOptimizer.strategic_loss = orig_loss
    for d in train_decisions + strat_dec + eval_decisions:
        u = sorted(d["util"], reverse=True)
        assert u[0] - u[1] >= MARGIN, ("near tie", u[:2])
        assert d["table"] == train_decisions[0]["table"]
    exp = {"model_name": gen_e2e.NAME, "coefficients": coefs, "config": cfg, "train": train, "queries": queries, "k": K,
           "table": train_decisions[0]["table"],
           "train_choices": [d["choice"] for d in train_decisions], "train_util": [d["util"] for d in train_decisions],
           "step_losses": losses, "predict": pred_dual, "predict_strategic": pred_strat, "predict_robust": pred_robust,
           "strategic_choices": [d["choice"] for d in strat_dec], "strategic_util": [d["util"] for d in strat_dec],
           "eval_texts": ev_texts, "eval_labels": ev_labels, "eval_seed": 123, "robustness": robust,
           "eval_choices": [d["choice"] for d in eval_decisions]}
    path = os.path.join(HERE, "strategic_bert_mini.json")
    json.dump(exp, open(path, "w"))
    np.savez_compressed(os.path.join(HERE, "strategic_bert_mini_head.npz"), **head)
    print("decisions: train %d, strategic %d, eval %d; steps %d; losses %.6f .. %.6f; robustness %s; %d bytes"
          % (len(train_decisions), len(strat_dec), len(eval_decisions), len(losses), losses[0], losses[-1], robust,
             os.path.getsize(path)))


if __name__ == "__main__":
    main()
