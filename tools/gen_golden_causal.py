"""Golden vectors of the reference's AUTOREGRESSIVE mode.  TEST INFRASTRUCTURE ONLY — needs the reference checkout that
oracle/gen_golden.py imports, never runs on the GPU box.

Builds the reference's own ``OmniBioTA`` (imported through the helpers of oracle/gen_golden.py: the mup stand-in, the hash
weights; nothing of the reference is copied) with ``autoregressive=True`` and no attention mask — its causal path,
model.py:115-130 — on the tiny config of the existing fixtures, fp32, B = 2, T = 64, once through SDPA (``flash=True``) and once
through its manual tril path (``flash=False``), and records

    tokens, emb, logits, loss, grad_sample/<parameter> (every 5th element, the layout of oracle/gen_golden.py), grad_sum/, grad_abs/

into tests/golden/tiny_fp32_causal.npz and tests/golden/tiny_fp32_causal_manual.npz.

THE LOSS IS THIS GENERATOR'S DEFINITION, not the reference's (which has no causal trainer): the mean cross entropy of position
t's logits against token t + 1 over the first T - 1 positions of every row — what omnibiote_amd.model.next_token_loss computes.
Everything up to ``emb`` is genuine reference code; ``logits`` onward depends on the restated readout (oracle/gen_golden.py).

Usage:  python tools/gen_golden_causal.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402
import omnibiote_ref as R  # noqa: E402


def next_token_loss(logits: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    V = logits.shape[-1]
    return F.cross_entropy(logits[:, :-1].reshape(-1, V), tokens[:, 1:].reshape(-1))


def build_causal_ref(ref_model, cfg: R.RefConfig):
    c = ref_model.OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd = cfg.block_size, cfg.vocab_size, cfg.n_layer, cfg.n_head, cfg.n_embd
    c.dropout = 0.0
    c.autoregressive = True
    c.flash = cfg.flash
    m = ref_model.OmniBioTA(c)
    sd = m.state_dict()
    for k, v in R.hash_weights(cfg).items():
        assert sd[k].shape == v.shape, k
        sd[k].copy_(v)
    m.train()
    return m


def run_case(ref_model, name: str, cfg: R.RefConfig, B: int, T: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    tokens = G.synth_tokens(rng, B, T, cfg.vocab_size, [[20, 41], [9, 30, 50]])   # EOS tokens are ordinary tokens here: no mask
    tok = torch.from_numpy(tokens)
    m = build_causal_ref(ref_model, cfg)
    out = {"tokens": tokens, "grad_stride": np.int64(5),
           "cfg": np.array([cfg.block_size, cfg.vocab_size, cfg.n_layer, cfg.n_head, cfg.n_embd, int(cfg.flash)], dtype=np.int64)}
    out["emb"] = m(tok, return_embeddings=True).detach().float().numpy()
    m.zero_grad(set_to_none=True)
    logits = m(tok)
    out["logits"] = logits.detach().float().numpy()
    loss = next_token_loss(logits, tok)
    out["loss"] = np.float32(loss.item())
    loss.backward()
    for k, p in m.named_parameters():
        out["grad_sample/" + k] = G.sample(p.grad)
        out["grad_sum/" + k] = np.float64(p.grad.double().sum().item())
        out["grad_abs/" + k] = np.float64(p.grad.double().abs().sum().item())
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), **out)
    print(f"{name}: loss {out['loss']:.6f} emb|max| {np.abs(out['emb']).max():.4f}")


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(4)
    ref_model, _ = G._import_reference()
    tiny = dict(block_size=64, vocab_size=512, n_layer=2, n_head=2, n_embd=128)
    run_case(ref_model, "tiny_fp32_causal", R.RefConfig(**tiny, autoregressive=True), 2, 64, 5)
    run_case(ref_model, "tiny_fp32_causal_manual", R.RefConfig(**tiny, autoregressive=True, flash=False), 2, 64, 5)


if __name__ == "__main__":
    main()
