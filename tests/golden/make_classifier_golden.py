"""Writes tests/golden/classifier_train_p0.npz: inputs and expected results of the reference's FusionClassifier for the ragged
front door (FusionClassifier.forward_packed).  Run once on a CPU with the reference checkout's root on PYTHONPATH:

    PYTHONPATH=<reference root> python tests/golden/make_classifier_golden.py

The reference's models.fusion_classifier.FusionClassifier is imported at run time and produces every recorded result in fp32; only
inputs and expected outputs are written.  Weights are never stored: both sides fill the parameters with the closed-form initialiser
oracle.hri_emo_oracle.closed_form_init_.  The model is FusionClassifier(128, 4, 8, 2, 32, dropout=0.0) in train mode (dropout 0:
the same function as eval), B = 4, the loss is the trainer's nn.CrossEntropyLoss (train_fusion_seq_level.py:394).

  seq   (L_a, L_t) = (40, 35), audio lengths [40, 5, 1, 33], text lengths [35, 20, 1, 32]: sample 1 has audio shorter than text, so
        audio PAD rows enter the pooled mean (fusion_classifier.py:145 pools all L_t positions); 1, 32, 33 sit on the 32-row chunk
        edge.  PAD input rows are zeros, as the reference's collate_seq_batch makes them.
  eq    (33, 33), every sample full length, no masks
  utt   eval, utterance-level [B, d] inputs, B = 5 (train_fusion_utter_level.py)
Per case: inputs, labels, logits, beta, pooled, loss; for seq and eq the norm and a 64-element strided sample of every parameter's
gradient (g.norm.<name>, g.samp.<name>)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.hri_emo_oracle import closed_form_init_  # noqa: E402

CFG = (128, 4, 8, 2, 32)
SEQ = {"pad": (40, 35), "la": [40, 5, 1, 33], "lt": [35, 20, 1, 32]}
EQ = {"pad": (33, 33), "la": [33] * 4, "lt": [33] * 4}


def padded(g, lens, L, d):
    x = torch.randn(len(lens), L, d, generator=g)
    m = torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]
    x[m] = 0.0
    return x, m


def strided(flat):
    return flat[torch.linspace(0, flat.numel() - 1, 64).long()].clone()


def main():
    from models.fusion_classifier import FusionClassifier          # the reference (PYTHONPATH)
    torch.set_num_threads(4)
    d = CFG[0]
    g = torch.Generator().manual_seed(20261020)
    out = {}
    for name, c in (("seq", SEQ), ("eq", EQ)):
        m = closed_form_init_(FusionClassifier(*CFG, dropout=0.0)).train()
        h_a, m_a = padded(g, c["la"], c["pad"][0], d)
        h_t, m_t = padded(g, c["lt"], c["pad"][1], d)
        y = torch.randint(0, CFG[1], (len(c["la"]),), generator=g)
        masked = bool(m_a.any() or m_t.any())
        logits, beta, pooled = m(h_a, h_t, m_a if masked else None, m_t if masked else None)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        out.update({f"{name}.h_a": h_a, f"{name}.h_t": h_t, f"{name}.len_a": torch.tensor(c["la"]), f"{name}.len_t": torch.tensor(c["lt"]),
                    f"{name}.pad": torch.tensor(c["pad"]), f"{name}.y": y, f"{name}.logits": logits, f"{name}.beta": beta,
                    f"{name}.pooled": pooled, f"{name}.loss": loss.reshape(1)})
        for n, p in m.named_parameters():
            out[f"{name}.g.norm.{n}"] = p.grad.norm().reshape(1)
            out[f"{name}.g.samp.{n}"] = strided(p.grad.reshape(-1))
    m = closed_form_init_(FusionClassifier(*CFG, dropout=0.0)).eval()
    u_a, u_t = torch.randn(5, d, generator=g), torch.randn(5, d, generator=g)
    with torch.no_grad():
        logits, beta, pooled = m(u_a, u_t)
    out.update({"utt.h_a": u_a, "utt.h_t": u_t, "utt.logits": logits, "utt.beta": beta, "utt.pooled": pooled})
    path = os.path.join(HERE, "classifier_train_p0.npz")
    np.savez_compressed(path, **{k: v.detach().numpy() for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes,", len(out), "keys")


if __name__ == "__main__":
    main()
