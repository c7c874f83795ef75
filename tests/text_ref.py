"""Plain-torch restatement of the text towers of gad/text.py, written from the architecture (a pre-LN transformer under a causal
mask, CLIP's text encoder), not from its code: embedding lookup, explicit masked softmax attention, QuickGELU, final LayerNorm,
end-of-text pooling by argmax, projection.  Takes both key layouts (OpenAI's names; HF's, with or without `text_model.`) and runs
in whatever dtype it is asked to: float64 on the CPU is the reference, float32 on the CPU the yardstick for what float32
arithmetic costs.  `to_openai` renames an HF state dict into OpenAI's layout."""
import torch
import torch.nn.functional as F


def _names(sd):
    if "token_embedding.weight" in sd:
        return sd, "openai"
    if "embeddings.token_embedding.weight" in sd:
        return sd, "hf"
    out = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}
    assert "embeddings.token_embedding.weight" in out, "neither layout's token embedding"
    return out, "hf"


def _act(h, kind):
    if kind == "gelu":
        return 0.5 * h * (1 + torch.erf(h / 2 ** 0.5))
    return h * torch.sigmoid(1.702 * h)


def _attention(q, k, v, heads):
    B, T, W = q.shape
    d = W // heads
    q, k, v = (t.view(B, T, heads, d).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / d ** 0.5
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, W)


def hidden_and_embed(sd, cfg, ids, dtype=torch.float64):
    """(last_hidden_state [B, T, W], text embedding [B, E] or None)"""
    sd, layout = _names(sd)
    p = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    W, ids = cfg.width, torch.as_tensor(ids).long()

    def ln(x, name):
        return F.layer_norm(x, (W,), p[name + ".weight"], p[name + ".bias"], cfg.eps)

    def lin(x, name):
        return x @ p[name + ".weight"].t() + p[name + ".bias"]

    if layout == "openai":
        x = p["token_embedding.weight"][ids] + p["positional_embedding"]
        for i in range(cfg.layers):
            b = f"transformer.resblocks.{i}."
            q, k, v = (ln(x, b + "ln_1") @ p[b + "attn.in_proj_weight"].t() + p[b + "attn.in_proj_bias"]).chunk(3, dim=-1)
            x = x + lin(_attention(q, k, v, cfg.heads), b + "attn.out_proj")
            x = x + lin(_act(lin(ln(x, b + "ln_2"), b + "mlp.c_fc"), cfg.act), b + "mlp.c_proj")
        h = ln(x, "ln_final")
        proj = p["text_projection"]
    else:
        x = p["embeddings.token_embedding.weight"][ids] + p["embeddings.position_embedding.weight"]
        for i in range(cfg.layers):
            b = f"encoder.layers.{i}."
            y = ln(x, b + "layer_norm1")
            a = _attention(lin(y, b + "self_attn.q_proj"), lin(y, b + "self_attn.k_proj"), lin(y, b + "self_attn.v_proj"), cfg.heads)
            x = x + lin(a, b + "self_attn.out_proj")
            x = x + lin(_act(lin(ln(x, b + "layer_norm2"), b + "mlp.fc1"), cfg.act), b + "mlp.fc2")
        h = ln(x, "final_layer_norm")
        proj = p["text_projection.weight"].t() if "text_projection.weight" in p else None
    if proj is None:
        return h, None
    return h, h[torch.arange(h.shape[0]), ids.argmax(dim=-1)] @ proj


def hidden(sd, cfg, ids, dtype=torch.float64):
    return hidden_and_embed(sd, cfg, ids, dtype)[0]


def embed(sd, cfg, ids, dtype=torch.float64):
    return hidden_and_embed(sd, cfg, ids, dtype)[1]


def embed_unit(sd, cfg, ids, dtype=torch.float64):
    e = embed(sd, cfg, ids, dtype)
    return e / e.norm(dim=-1, keepdim=True)


def to_openai(sd, layers):
    """an HF state dict (with or without `text_model.`) under OpenAI's names: q / k / v fused into in_proj, text_projection
    transposed, final_layer_norm -> ln_final"""
    sd, layout = _names(sd)
    assert layout == "hf"
    out = {"token_embedding.weight": sd["embeddings.token_embedding.weight"], "positional_embedding": sd["embeddings.position_embedding.weight"],
           "ln_final.weight": sd["final_layer_norm.weight"], "ln_final.bias": sd["final_layer_norm.bias"],
           "text_projection": sd["text_projection.weight"].t().contiguous()}
    for i in range(layers):
        a, b = f"encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for wb in ("weight", "bias"):
            out[b + "attn.in_proj_" + wb] = torch.cat([sd[a + f"self_attn.{n}_proj." + wb] for n in "qkv"], 0)
            for src, dst in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                             ("mlp.fc2", "mlp.c_proj")):
                out[b + dst + "." + wb] = sd[a + src + "." + wb]
    return out
