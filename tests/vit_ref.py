"""Plain-torch restatement of the image towers of gad/vit.py, written from the architecture (a pre-LN Vision Transformer), not
from its code: nn.Conv2d-style patch embedding on the normalised image, explicit softmax attention, both GELUs, both output
conventions.  Takes the same state dicts (OpenAI / open-CLIP names for a configuration with an `embed_dim`, HF BLIP names for
one without, prefix optional) and runs in whatever dtype and on whatever device it is asked to: float64 on the CPU is the
reference, float32 on the CPU the yardstick for what float32 arithmetic costs."""
import torch
import torch.nn.functional as F


def geometry(H, W, R, clip):
    """torchvision Resize(R) (shorter side to R, the longer one int(R * long / short)) + CenterCrop(R), or BLIP's Resize((R, R))
    -> (rh, rw, top, left)"""
    if not clip:
        return R, R, 0, 0
    rh, rw = (R, int(R * W / H)) if H <= W else (int(R * H / W), R)
    return rh, rw, int(round((rh - R) / 2.0)), int(round((rw - R) / 2.0))


def preprocess(images01, cfg, dtype=torch.float64):
    """[B,3,H,W] in [0,1] -> normalised [B,3,R,R]: antialiased bicubic resize, centre crop, (x - mean) / std"""
    x = images01.to(dtype)
    R = cfg.image_size
    rh, rw, top, left = geometry(x.shape[2], x.shape[3], R, cfg.embed_dim is not None)
    x = F.interpolate(x, size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)[:, :, top:top + R, left:left + R]
    mean = torch.tensor(cfg.mean, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(cfg.std, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def _strip(sd, prefix, probe):
    if probe in sd:
        return sd
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _act(h, kind):
    if kind == "gelu":
        return 0.5 * h * (1 + torch.erf(h / 2 ** 0.5))
    return h * torch.sigmoid(1.702 * h)


def _attention(x, w_qkv, b_qkv, heads):
    B, T, W = x.shape
    d = W // heads
    q, k, v = (x @ w_qkv.t() + b_qkv).view(B, T, 3, heads, d).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, T, W)


def forward(sd, cfg, images01, dtype=torch.float64, device="cpu"):
    """raw embedding [B, embed_dim or width]"""
    clip = cfg.embed_dim is not None
    if clip:
        sd = _strip(sd, "visual.", "conv1.weight")
        n = dict(patch="conv1", cls="class_embedding", pos="positional_embedding", pre="ln_pre", blk="transformer.resblocks.{}.",
                 ln1="ln_1", ln2="ln_2", qw="attn.in_proj_weight", qb="attn.in_proj_bias", out="attn.out_proj", fc="mlp.c_fc",
                 pj="mlp.c_proj", post="ln_post")
    else:
        sd = _strip(sd, "vision_model.", "embeddings.patch_embedding.weight")
        n = dict(patch="embeddings.patch_embedding", cls="embeddings.class_embedding", pos="embeddings.position_embedding",
                 pre="pre_layernorm", blk="encoder.layers.{}.", ln1="layer_norm1", ln2="layer_norm2", qw="self_attn.qkv.weight",
                 qb="self_attn.qkv.bias", out="self_attn.projection", fc="mlp.fc1", pj="mlp.fc2", post="post_layernorm")
    p = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    W = cfg.width

    def ln(x, name):
        return F.layer_norm(x, (W,), p[name + ".weight"], p[name + ".bias"], cfg.eps)

    x = preprocess(images01.to(device), cfg, dtype)
    x = F.conv2d(x, p[n["patch"] + ".weight"], p.get(n["patch"] + ".bias") if cfg.patch_bias else None, stride=cfg.patch)
    B = x.shape[0]
    x = x.flatten(2).transpose(1, 2)                                       # [B, g g, W], row-major patches
    x = torch.cat([p[n["cls"]].reshape(1, 1, W).expand(B, 1, W), x], 1) + p[n["pos"]].reshape(1, -1, W)
    if cfg.ln_pre:
        x = ln(x, n["pre"])
    for i in range(cfg.layers):
        b = n["blk"].format(i)
        a = _attention(ln(x, b + n["ln1"]), p[b + n["qw"]], p[b + n["qb"]], cfg.heads)
        x = x + a @ p[b + n["out"] + ".weight"].t() + p[b + n["out"] + ".bias"]
        h = _act(ln(x, b + n["ln2"]) @ p[b + n["fc"] + ".weight"].t() + p[b + n["fc"] + ".bias"], cfg.act)
        x = x + h @ p[b + n["pj"] + ".weight"].t() + p[b + n["pj"] + ".bias"]
    if clip:
        return ln(x[:, 0], n["post"]) @ p["proj"]
    return ln(x, n["post"])[:, 0]


def embed_unit(sd, cfg, images01, dtype=torch.float64, device="cpu"):
    e = forward(sd, cfg, images01, dtype, device)
    return e / e.norm(dim=-1, keepdim=True)
