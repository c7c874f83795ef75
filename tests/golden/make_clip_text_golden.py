"""Writes tests/golden/clip_text.npz: a tiny seeded `transformers.CLIPTextModelWithProjection` (built offline from a config,
no download), run on the CPU in float64 - the independent oracle of tests/text_ref.py and, through it, of gad/text.py.

  config   vocab 48 (bos 46, eos 47), 20 positions, hidden 32, 2 heads (head dim 16), 2 layers, intermediate 64, projection 24,
           quick_gelu, layer_norm_eps 1e-5
  stored   the state dict under HF's own names (`sd/<key>`; `position_ids` left out), three id rows - a short prompt padded
           with the end token, a full-length one, start + end only - `last_hidden_state` [3, 20, 32] and `text_embeds` [3, 24]
The parameters are re-drawn (seeded, LayerNorm gains around 1, biases not zero) so that no term of the network is trivially
absent; they are rounded to float32 values, the arithmetic is float64.  `attn_implementation="sdpa"`: transformers' "eager"
attention takes its softmax in float32 whatever the model's dtype (2e-7 off), the sdpa path stays in float64.  transformers'
tokenizer is NOT used anywhere: only the model.

    python tests/golden/make_clip_text_golden.py"""
import os

import numpy as np
import torch
from transformers import CLIPTextConfig, CLIPTextModelWithProjection

V, T, W, HEADS, LAYERS, MLP, E = 48, 20, 32, 2, 2, 64, 24
BOS, EOS = 46, 47


def main():
    torch.manual_seed(20)
    cfg = CLIPTextConfig(vocab_size=V, hidden_size=W, intermediate_size=MLP, projection_dim=E, num_hidden_layers=LAYERS,
                         num_attention_heads=HEADS, max_position_embeddings=T, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                         bos_token_id=BOS, eos_token_id=EOS, pad_token_id=EOS, attn_implementation="sdpa")
    model = CLIPTextModelWithProjection(cfg).double().eval()
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g, dtype=torch.float64)
            if "layer_norm" in name:
                r = 1 + 0.1 * r if name.endswith("weight") else 0.1 * r
            elif "position_embedding" in name:
                r = 0.02 * r
            elif "token_embedding" in name or name.endswith("bias"):
                r = 0.1 * r
            else:
                r = r / p.shape[1] ** 0.5
            p.copy_(r.float().double())                                  # the weights are float32 values, the arithmetic float64
    gi = torch.Generator().manual_seed(22)
    ids = torch.full((3, T), EOS, dtype=torch.long)
    ids[:, 0] = BOS
    ids[0, 1:6] = torch.randint(0, BOS, (5,), generator=gi)              # short prompt: bos, 5 pieces, eos, eos padding
    ids[1, 1:T - 1] = torch.randint(0, BOS, (T - 2,), generator=gi)      # full length: eos is the last position
    # row 2: bos, eos, eos padding
    with torch.no_grad():
        out = model(input_ids=ids)
        # causality, checked here once: changing token 3 leaves rows 0-2 as they were
        ids2 = ids.clone()
        ids2[1, 3] = (ids2[1, 3] + 1) % BOS
        assert torch.equal(model(input_ids=ids2).last_hidden_state[1, :3], out.last_hidden_state[1, :3])
    arrays = {"ids": ids.numpy().astype(np.int32), "last_hidden_state": out.last_hidden_state.numpy(),
              "text_embeds": out.text_embeds.numpy(), "config": np.array([V, T, W, LAYERS, HEADS, MLP, E], dtype=np.int64)}
    for k, v in model.state_dict().items():
        if not k.endswith("position_ids"):
            arrays["sd/" + k] = v.numpy().astype(np.float32)             # exact: they are float32 values
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_text.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
