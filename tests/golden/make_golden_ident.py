#!/usr/bin/env python3
"""Generate tests/golden/ident.npz by RUNNING THE REFERENCE's objective_assessment (train/train_utils.py:752-816).

Run in the build container only (needs the reference tree; it never travels):

    python tests/golden/make_golden_ident.py

The "model" is a callable that returns stored outputs (tests/ident_oracle.py synth_batch, seeded), the dataloader a list
of batches: plain target tensors (dataset=None) or {'image', 'fmri'} dicts (dataset='bold').  Per case it stores the
batch seeds, the reference's PearsonCorrelation / StructuralSimilarity of every (output, target) pair of every batch
(the pair list is row-major over all pairs), and for top = 2, 5, 10 the ``random.seed`` used, the score, and the
smallest |gt - distractor| margin over the drawn comparisons (pairs of bitwise-equal targets excluded: those tie
exactly).  Seeds are chosen so that the margin is > 1e-4 and both scores lie strictly between 0 and 1.
Fixtures are data only (numbers); no reference source is stored.
"""
import importlib
import os
import random
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

import ident_oracle as IO  # noqa: E402  (seeded batches and the stored-output model only)

REF = "/root/reference"
MIN_MARGIN = 1e-4

# name, dataset, [(n, c, h, w, seed, dup)]: a duplicated target in the first batch, a second batch of another size
CASES = [
    ("px64", None, [(16, 3, 64, 64, 31, (2, 5)), (10, 3, 64, 64, 32, None)]),
    ("px100", "bold", [(12, 3, 100, 100, 41, (0, 7)), (7, 3, 100, 100, 42, None)]),
]
TOPS = (2, 5, 10)


def reference_train_utils():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvu = types.ModuleType("torchvision.utils")
    tvu.make_grid = tvu.save_image = lambda *a, **k: None
    tv.models, tv.utils = tvm, tvu
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.utils": tvu})
    for m in ("train.train_utils", "train"):
        sys.modules.pop(m, None)
    return importlib.import_module("train.train_utils")


def batches_of(dataset, spec):
    outs, tgts, loader = [], [], []
    for n, c, h, w, seed, dup in spec:
        pred, truth = IO.synth_batch(n, c, h, w, seed, dup)
        outs.append(pred)
        tgts.append(truth)
        loader.append({"image": truth, "fmri": torch.zeros(n, 8)} if dataset == "bold" else truth)
    return outs, tgts, loader


def main():
    tu = reference_train_utils()
    pcc, ssim = tu.PearsonCorrelation(), tu.StructuralSimilarity()
    out = {"meta/case": np.array("ident"), "meta/cases": np.array([c[0] for c in CASES]),
           "meta/tops": np.array(TOPS)}
    for name, dataset, spec in CASES:
        outs, tgts, loader = batches_of(dataset, spec)
        out[f"{name}/dataset"] = np.array(dataset or "none")
        out[f"{name}/batches"] = np.array([[n, c, h, w, s, *(dup if dup else (-1, -1))]
                                           for n, c, h, w, s, dup in spec])
        mats = []
        for b, (o, t) in enumerate(zip(outs, tgts)):
            n = len(t)
            P = np.zeros((n, n))
            S = np.zeros((n, n))
            for i in range(n):
                for j in range(n):
                    P[i, j] = pcc(o[i], t[j]).item()
                    S[i, j] = ssim(o[i].unsqueeze(0), t[j].unsqueeze(0)).item()
            out[f"{name}/b{b}/pcc"], out[f"{name}/b{b}/ssim"] = P, S
            same = np.array([[torch.equal(t[i], t[j]) for j in range(n)] for i in range(n)])
            mats.append((P, S, same))
        model = IO.StoredModel(loader, outs)
        for top in TOPS:
            for seed in range(1000 * top, 1000 * top + 500):
                random.seed(seed)
                margin = [np.inf, np.inf]
                for (P, S, same), t in zip(mats, tgts):
                    d = IO.draw_distractors(len(t), top).numpy()
                    for i in range(len(t)):
                        for j in d[i]:
                            if not same[i, j]:
                                margin[0] = min(margin[0], abs(P[i, i] - P[i, j]))
                                margin[1] = min(margin[1], abs(S[i, i] - S[i, j]))
                random.seed(seed)
                score = tu.objective_assessment(model, loader, dataset=dataset, top=top)
                if min(margin) > MIN_MARGIN and all(0.0 < float(v) < 1.0 for v in score):
                    break
            else:
                raise SystemExit(f"{name} top {top}: no seed with margin > {MIN_MARGIN} and a score in (0, 1)")
            out[f"{name}/top{top}/seed"] = np.int64(seed)
            out[f"{name}/top{top}/score"] = score.numpy().astype(np.float32)
            out[f"{name}/top{top}/margin"] = np.array(margin)
            print(name, "top", top, "seed", seed, "score", score.tolist(), "margin", margin)
    np.savez_compressed(os.path.join(HERE, "ident.npz"), **out)


if __name__ == "__main__":
    main()
