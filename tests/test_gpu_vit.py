"""The Vision Transformer image towers on the GPU: the four kernels of csrc/vit.hip through the C ABI against float64, gad/vit.py
against the plain-torch restatement of tests/vit_ref.py in float64, the two scores built on it, and the two entry points that
switch to it.

Every bound is a multiple of what float32 arithmetic costs on the SAME inputs, measured on the CPU (numpy / torch in float32
against float64) and written next to the constant; the inputs are seeded, so the yardsticks are fixed numbers."""
import functools
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_ref as R
from gad import _capi, ops, scoring, vit

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TAIL = 5                       # rows allocated past the end of every output
SENTINEL = -123.5
WS_TAIL, WS_FILL = 256, 0xA5


def _lib():
    return _capi.load()


# ---------------------------------------------------------------------------------------------------------------
# gad_resize_bicubic_patches
# ---------------------------------------------------------------------------------------------------------------
# (H, W, rh, rw, oy, ox, R, P): 32 -> 24; 40 x 56 with the shorter side to 30, then the centre 24 (crop origin on both axes);
# the same image with the shorter side to 24 (crop origin on one axis only); 16 -> 56, upscaling; 37 x 53 -> 64 with P = 4,
# odd sizes and ragged tap counts at both borders
RESIZE_GEOMETRIES = [(32, 32, 24, 24, 0, 0, 24, 8), (40, 56, 30, 42, 3, 9, 24, 8), (40, 56, 24, 33, 0, 4, 24, 8),
                     (16, 16, 56, 56, 0, 0, 56, 8), (37, 53, 64, 64, 0, 0, 64, 4)]
# the same table (vit.resize_matrix, rounded to float32) applied in float32 numpy, columns first, against float64, max abs
# over the five geometries at B = 3: 2.06e-07 (per geometry 1.76e-07, 1.68e-07, 1.50e-07, 2.06e-07, 1.91e-07)
RESIZE_F32_ERR = 2.06e-07


def _resize_inputs(H, W, B):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W))


def _patchify(img, P):
    """[B,3,R,R] -> [B g g, P P 3] with (ph, pw, c) fastest"""
    B, _, Rr, _ = img.shape
    g = Rr // P
    return img.reshape(B, 3, g, P, g, P).transpose(0, 2, 4, 3, 5, 1).reshape(B * g * g, P * P * 3)


def _resize_ref(x, geom, dtype):
    H, W, rh, rw, oy, ox, Rr, P = geom
    My, Mx = vit.resize_matrix(H, rh, oy, Rr, dtype), vit.resize_matrix(W, rw, ox, Rr, dtype)
    return _patchify(My @ (x.numpy().astype(dtype) @ Mx.T), P)


def resize_f32_error(geom, B=3):
    x = _resize_inputs(geom[0], geom[1], B)
    return float(np.abs(_resize_ref(x, geom, np.float32).astype(np.float64) - _resize_ref(x, geom, np.float64)).max())


def _run_resize(x, geom, a=1.0, b=0.0):
    H, W, rh, rw, oy, ox, Rr, P = geom
    B, rows, cols = x.shape[0], x.shape[0] * (Rr // P) ** 2, P * P * 3
    lib = _lib()
    need = lib.gad_resize_bicubic_patches_workspace_bytes(H, W, rh, rw, oy, ox, Rr, P)
    assert need > 0, lib.gad_last_error()
    ws = torch.full((need + WS_TAIL,), WS_FILL, device=dev, dtype=torch.uint8)
    y = torch.full((rows + TAIL, cols), SENTINEL, device=dev)
    xd = x.to(dev).contiguous()
    rc = lib.gad_resize_bicubic_patches(xd.data_ptr(), y.data_ptr(), B, H, W, rh, rw, oy, ox, Rr, P, a, b, ws.data_ptr(), need,
                                        ops._stream())
    assert rc == 0, lib.gad_last_error()
    assert bool((y[rows:] == SENTINEL).all()) and bool((ws[need:] == WS_FILL).all())
    return y[:rows].cpu().double().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("geom", RESIZE_GEOMETRIES)
def test_resize_bicubic_patches_against_the_float64_table(geom, B):
    x = _resize_inputs(geom[0], geom[1], 3)[:B]
    want = _resize_ref(x, geom, np.float64)
    got = _run_resize(x, geom)
    err = np.abs(got - want).max()
    print(f"resize {geom} B={B}: max abs err {err:.3e} (bound {4 * RESIZE_F32_ERR:.3e})")
    assert err <= 4 * RESIZE_F32_ERR
    if B == 3:      # y = a v + b: a times the error of v, one rounding of the product and one of the sum, each of a value below 4
        got = _run_resize(x, geom, a=2.0, b=-1.0)
        assert np.abs(got - (2 * want - 1)).max() <= 2 * 4 * RESIZE_F32_ERR + 2 * 2.0 ** -22


def test_resize_refusals_launch_nothing():
    lib = _lib()
    x, y, ws = torch.zeros(1, 3, 32, 32, device=dev), torch.zeros(9, 192, device=dev), torch.zeros(4096, device=dev)
    bad = [((32, 32, 24, 24, 0, 0, 24, 7), "multiple of the patch"), ((32, 32, 24, 24, 1, 0, 24, 8), "crop"),
           ((32, 32, 24, 24, 0, -1, 24, 8), "crop"), ((1024, 32, 24, 24, 0, 0, 24, 8), "64 taps"), ((32, 32, 0, 24, 0, 0, 24, 8), ">= 1"),
           ((32, 32, 128, 128, 0, 0, 128, 128), "LDS")]
    for geom, why in bad:
        assert lib.gad_resize_bicubic_patches_workspace_bytes(*geom) == -1 and why in lib.gad_last_error().decode(), geom
        H, W, rh, rw, oy, ox, Rr, P = geom
        assert lib.gad_resize_bicubic_patches(x.data_ptr(), y.data_ptr(), 1, H, W, rh, rw, oy, ox, Rr, P, 1.0, 0.0, ws.data_ptr(),
                                              ws.numel() * 4, ops._stream()) == 1
        assert why in lib.gad_last_error().decode()
    assert lib.gad_resize_bicubic_patches(x.data_ptr(), y.data_ptr(), 1, 32, 32, 24, 24, 0, 0, 24, 8, 1.0, 0.0, ws.data_ptr(), 16,
                                          ops._stream()) == 1 and "workspace" in lib.gad_last_error().decode()
    assert lib.gad_resize_bicubic_patches(None, y.data_ptr(), 1, 32, 32, 24, 24, 0, 0, 24, 8, 1.0, 0.0, ws.data_ptr(), 16384,
                                          ops._stream()) == 1 and "null" in lib.gad_last_error().decode()
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# gad_vit_tokens
# ---------------------------------------------------------------------------------------------------------------
# torch's float32 F.layer_norm of the float32 sum (CPU) against float64 on these inputs (B = 3, T = 10; rows near 100 with a
# spread of 0.1, where E[x^2] - E[x]^2 has lost every digit): C = 64: 1.42e-04, C = 96: 8.43e-05.  The error is the sum's own
# rounding at 100 (ulp 7.6e-6) seen against the spread.
TOKENS_F32_ERR = {64: 1.42e-04, 96: 8.43e-05}


def _token_inputs(C, B=3, T=10):
    g = torch.Generator().manual_seed(C)
    patches = 100 + 0.1 * torch.randn(B, T - 1, C, generator=g)
    cls = 100 + 0.1 * torch.randn(C, generator=g)
    pos = 0.1 * torch.randn(T, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return patches, cls, pos, gamma, beta


def _tokens_ref(patches, cls, pos, gamma, beta, dtype, eps=1e-5):
    B, _, C = patches.shape
    x = torch.cat([cls.to(dtype).view(1, 1, C).expand(B, 1, C), patches.to(dtype)], 1) + pos.to(dtype)
    return x if gamma is None else F.layer_norm(x, (C,), gamma.to(dtype), beta.to(dtype), eps)


def tokens_f32_error(C):
    t = _token_inputs(C)
    return float((_tokens_ref(*t, torch.float32).double() - _tokens_ref(*t, torch.float64)).abs().max())


def _run_tokens(patches, cls, pos, gamma, beta, offset=0):
    """`offset`: floats by which every buffer is shifted off its 16-byte alignment (the scalar path)"""
    B, Tm1, C = patches.shape
    T = Tm1 + 1

    def put(t):
        if t is None:
            return None
        buf = torch.zeros(t.numel() + offset, device=dev)
        buf[offset:] = t.reshape(-1).to(dev)
        return buf[offset:]
    p, c, po, g, b = put(patches), put(cls), put(pos), put(gamma), put(beta)
    out = torch.full(((B * T + TAIL) * C + offset,), SENTINEL, device=dev)[offset:]
    rc = _lib().gad_vit_tokens(p.data_ptr(), c.data_ptr(), po.data_ptr(), ops._ptr(g), ops._ptr(b), out.data_ptr(), B, T, C, 1e-5,
                               ops._stream())
    assert rc == 0, _lib().gad_last_error()
    assert bool((out[B * T * C:] == SENTINEL).all())
    return out[:B * T * C].view(B, T, C).cpu()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C", [64, 96])
def test_vit_tokens_with_and_without_ln(C, offset):
    patches, cls, pos, gamma, beta = _token_inputs(C)
    got = _run_tokens(patches, cls, pos, gamma, beta, offset)
    err = float((got.double() - _tokens_ref(patches, cls, pos, gamma, beta, torch.float64)).abs().max())
    print(f"tokens C={C} offset={offset}: LN max abs err {err:.3e} (bound {4 * TOKENS_F32_ERR[C]:.3e})")
    assert err <= 4 * TOKENS_F32_ERR[C]
    plain = _run_tokens(patches, cls, pos, None, None, offset)            # no norm: one float32 add, bit for bit
    assert torch.equal(plain, _tokens_ref(patches, cls, pos, None, None, torch.float32))
    assert torch.equal(plain[:, 0], (cls + pos[0]).expand(3, C))
    for B in (1, 2):                                                      # rows depend on their own image alone
        assert torch.equal(_run_tokens(patches[:B], cls, pos, gamma, beta, offset), got[:B])


def test_vit_tokens_refusals():
    lib, z = _lib(), torch.zeros(4096, device=dev)
    p = z.data_ptr()
    assert lib.gad_vit_tokens(p, p, p, p, None, p, 1, 10, 64, 1e-5, ops._stream()) == 1 and "together" in lib.gad_last_error().decode()
    assert lib.gad_vit_tokens(p, p, p, None, None, p, 1, 1, 64, 1e-5, ops._stream()) == 1 and "T=1" in lib.gad_last_error().decode()
    assert lib.gad_vit_tokens(p, None, p, None, None, p, 1, 10, 64, 1e-5, ops._stream()) == 1 and "null" in lib.gad_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------
# gad_gelu
# ---------------------------------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, 20.0, -20.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 6.0, -6.0, 1.0, -1.0]


def _gelu_inputs(rows, C):
    x = 3 * torch.randn(rows, C, generator=torch.Generator().manual_seed(C))
    x[0, :len(SPECIALS)] = torch.tensor(SPECIALS)
    return x


def _gelu_ref(x, kind):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5)) if kind == 0 else x * torch.sigmoid(1.702 * x)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("C,ld", [(64, 80), (70, 77)])
def test_gelu_on_a_slice(C, ld, kind):
    """Both kinds on a [rows][C] slice of a [rows][ld] buffer (float4 path: C = 64, ld = 80; scalar path: C = 70, ld = 77) with
    +-0, +-20, denormals and +-6 (where 1 + erf cancels) in the first row.  Bound: 4 x the error of torch's float32 evaluation
    of the same formula on the same inputs against float64, taken in the test itself: 2.8e-07 / 4.2e-07 (erf, C = 64 / 70) and
    4.9e-07 / 4.8e-07 (QuickGELU), all at |x| of 7 to 10, where half an ulp of the result is 4.8e-07.  The columns past C keep their bits."""
    rows = 7
    x = _gelu_inputs(rows, C)
    want = _gelu_ref(x.double(), kind)
    yard = float((_gelu_ref(x, kind).double() - want).abs().max())
    buf = torch.full((rows, ld), float("nan"))
    buf[:, C:] = torch.arange(rows * (ld - C)).view(rows, -1).float() - 3.25
    buf[:, :C] = x
    d = buf.to(dev)
    rc = _lib().gad_gelu(d.data_ptr(), rows, C, ld, kind, ops._stream())
    assert rc == 0, _lib().gad_last_error()
    got = d.cpu()
    assert torch.equal(got[:, C:].view(torch.int32), buf[:, C:].view(torch.int32))
    err = float((got[:, :C].double() - want).abs().max())
    print(f"gelu kind={kind} C={C}: max abs err {err:.3e}, float32 torch {yard:.3e}")
    assert yard > 1e-8 and err <= 4 * yard
    s = got[0, :len(SPECIALS)]
    assert torch.isfinite(s).all()
    assert float(s[0]) == 0.0 and float(s[1]) == 0.0 and float(s[2]) == 20.0 and abs(float(s[3])) < 1e-6
    assert (s[4:8].abs() <= 1e-40).all()                                   # a denormal stays one (or flushes to zero)


def test_gelu_refusals():
    lib, z = _lib(), torch.zeros(64, device=dev)
    assert lib.gad_gelu(z.data_ptr(), 1, 64, 64, 2, ops._stream()) == 1 and "kind=2" in lib.gad_last_error().decode()
    assert lib.gad_gelu(z.data_ptr(), 1, 64, 32, 0, ops._stream()) == 1 and "ld=32" in lib.gad_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------
# gad_l2_normalize_rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", [(96, 96), (96, 104), (70, 77), (512, 512)])
def test_l2_normalize_rows(C, ld):
    """Rows of norm about 1, 1e-20 (its squares are below the smallest float32) and 1e+20 (their sum is above the largest), against
    float64.  Bound 16 x 2^-24 on entries of magnitude <= 1: the scaling is by powers of two and exact; the sum of squares is a
    tree of at most 2 (float4) + 6 (wave) levels behind at most 2 serial adds per lane, each rounding once, the square, the
    square root and the division once more - under 16 half-ulps of relative error on the norm and the quotient together."""
    rows = 6
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(C + ld))
    x[1] *= 1e-20 / C ** 0.5
    x[2] *= 1e+20 / C ** 0.5
    x[3, 1:] = 0                                                           # a single non-zero entry: exactly +-1
    buf = torch.full((rows, ld), SENTINEL)
    buf[:, :C] = x
    d = buf.to(dev)
    rc = _lib().gad_l2_normalize_rows(d.data_ptr(), rows, C, ld, ops._stream())
    assert rc == 0, _lib().gad_last_error()
    got = d.cpu()
    assert bool((got[:, C:] == SENTINEL).all())
    want = x.double() / x.double().norm(dim=1, keepdim=True)
    assert torch.isfinite(got[:, :C]).all()
    err = float((got[:, :C].double() - want).abs().max())
    print(f"l2 C={C} ld={ld}: max abs err {err:.3e}")
    assert err <= 16 * 2.0 ** -24
    assert abs(float(got[3, 0])) == 1.0 and float(got[3, 1:C].abs().max()) == 0.0
    assert float((got[1, :C].double().norm() - 1).abs()) < 1e-6


def test_l2_normalize_zero_row_has_no_eps():
    d = torch.zeros(2, 64, device=dev)
    d[1] = 1.0
    assert _lib().gad_l2_normalize_rows(d.data_ptr(), 2, 64, 64, ops._stream()) == 0
    got = d.cpu()
    assert torch.isnan(got[0]).all() and torch.equal(got[1], torch.full((64,), 0.125))


# ---------------------------------------------------------------------------------------------------------------
# the whole tower
# ---------------------------------------------------------------------------------------------------------------
# name -> (config, input H x W).  T = 10: the M = B T rows are ragged; T = 50: ViT-B/32's token count, one head of 64;
# T = 257: ViT-L/14's token count, two heads of 64, BLIP's conventions (erf GELU, no ln_pre, patch bias, unprojected output)
TOWERS = {
    "t10": (vit.Config(24, 8, 64, 2, 2, 256, 32), (40, 56)),
    "t50": (vit.Config(56, 8, 64, 2, 1, 256, 32), (70, 60)),
    "t257": (vit.Config(64, 4, 128, 2, 2, 512, None, act="gelu", ln_pre=False, patch_bias=True), (37, 53)),
}
# vit_ref in float32 on the CPU against float64 on the same three images, max abs over the unit embedding (t10, t50) or the raw
# one (t257, entries of magnitude up to 3): the yardstick; the GPU may take 8 x it (two blocks of MFMA summation orders).
#                 yardstick
#   t10           4.36e-07
#   t50           1.06e-06
#   t257          2.10e-06
# The GPU's own error is printed by the test (`pytest -s`); it has not been recorded here yet.
TOWER_F32_ERR = {"t10": 4.36e-07, "t50": 1.06e-06, "t257": 2.10e-06}
SEED = 7


def _tower_images(name):
    H, W = TOWERS[name][1]
    return torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(H + W))


@functools.lru_cache(maxsize=None)
def _tower_ref(name, dtype=torch.float64):
    cfg = TOWERS[name][0]
    sd = vit.seeded_state_dict(cfg, SEED)
    fn = R.embed_unit if cfg.embed_dim is not None else R.forward
    with torch.no_grad():
        return fn(sd, cfg, _tower_images(name), dtype)


def tower_f32_error(name):
    return float((_tower_ref(name, torch.float32).double() - _tower_ref(name)).abs().max())


@functools.lru_cache(maxsize=None)
def _tower(name):
    return vit.VisionTower.seeded(TOWERS[name][0], SEED).to(dev)


def _tower_out(name, images):
    t = _tower(name)
    return (t.embed_unit(images) if t.cfg.embed_dim is not None else t(images)).cpu().double()


@pytest.mark.parametrize("B,max_batch", [(1, None), (3, None), (3, 2)])
@pytest.mark.parametrize("name", list(TOWERS))
def test_whole_tower_against_the_float64_reference(name, B, max_batch):
    t = _tower(name)
    assert t.tag == f"vit-seeded{SEED}" and t.cfg.tokens == {"t10": 10, "t50": 50, "t257": 257}[name]
    keep = t.max_batch
    try:
        if max_batch:
            t.max_batch = max_batch                     # two chunks, the second of one image
        got = _tower_out(name, _tower_images(name)[:B].to(dev))
    finally:
        t.max_batch = keep
    want = _tower_ref(name)[:B]
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"tower {name} B={B} max_batch={max_batch}: max abs err {err:.3e} (yardstick {TOWER_F32_ERR[name]:.3e})")
    assert err <= 8 * TOWER_F32_ERR[name]


def test_cosine_and_aesthetic_scores():
    """cosine of an image with itself; the aesthetic head on the tower against float64 within the tower's bound times |w|_1"""
    name = "t10"
    t, images = _tower(name), _tower_images(name).to(dev)
    e = t.embed_unit(images)
    assert float(((e * e).sum(1) - 1).abs().max()) <= 1e-6
    head = vit.AestheticHead.seeded(t, 11).to(dev)
    assert head.tag == "aesthetic-seeded11"
    w, b = head.weight.cpu().double(), head.bias.cpu().double()
    want = _tower_ref(name) @ w.t() + b
    got = head(images).cpu().double()
    assert got.shape == (3,)
    err = float((got - want.view(-1)).abs().max())
    print(f"aesthetic: max abs err {err:.3e} (bound {8 * TOWER_F32_ERR[name] * float(w.abs().sum()):.3e})")
    assert err <= 8 * TOWER_F32_ERR[name] * float(w.abs().sum())


def test_tower_refuses_without_weights_and_off_device():
    with pytest.raises(_capi.GadError, match="no weights"):
        vit.VisionTower(TOWERS["t10"][0])(torch.zeros(1, 3, 24, 24, device=dev))
    with pytest.raises(_capi.GadError, match="device tensor"):
        _tower("t10")(torch.zeros(1, 3, 24, 24))


# ---------------------------------------------------------------------------------------------------------------
# diversity_against_dataset on the BLIP tower
# ---------------------------------------------------------------------------------------------------------------
DIV_CFG = TOWERS["t257"][0]
GROUPS, PER_GROUP, GEN_COUNTS = 4, 10, (6, 3, 2, 1)


class _ToyDataset:
    """40 images in [-1, 1]: four seeded prototypes, ten noisy copies of each, interleaved"""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.protos = torch.rand(GROUPS, 3, 37, 53, generator=g)
        self.group = torch.arange(GROUPS * PER_GROUP) % GROUPS
        self.images01 = (self.protos[self.group] + 0.02 * torch.randn(GROUPS * PER_GROUP, 3, 37, 53, generator=g)).clamp(0, 1)
        self.gen_group = torch.tensor([k for k, n in enumerate(GEN_COUNTS) for _ in range(n)])
        self.gen01 = (self.protos[self.gen_group] + 0.02 * torch.randn(len(self.gen_group), 3, 37, 53, generator=g)).clamp(0, 1)

    def __len__(self):
        return len(self.images01)

    def device_tensor(self, device, idx=None):
        x = self.images01 if idx is None else self.images01[idx]
        return (x * 2 - 1).to(device)


def test_diversity_on_the_blip_tower(monkeypatch):
    """the three keys and the tower's tag; entropy and counts equal `diversity_from_embeddings` on the float64 reference's
    embeddings.  No assignment can flip: a dot product of two embeddings moves by at most 2 d max|e|_1 when every entry moves
    by d = 8 x the yardstick (the tower test's bound, with the yardstick taken on these images), and both the gap between the clusters of the reference set and the
    margin of every generated image's nearest cluster are asserted to exceed 10 x that."""
    from src.attributions.global_scores.diversity_score import diversity_from_embeddings
    monkeypatch.setitem(vit.PRESETS, "blip_vqa_base", DIV_CFG)
    monkeypatch.setenv("GAD_DIVERSITY_NET", "blip-seeded")
    monkeypatch.delenv("GAD_BLIP_VISION_WEIGHTS", raising=False)
    scoring._REF_STATS.clear()
    ds = _ToyDataset()
    sd = vit.seeded_state_dict(DIV_CFG, 1234)
    ref01 = ds.device_tensor("cpu").add(1).div(2).clamp(0, 1)      # the images as the product sees them: through [-1, 1] and back
    with torch.no_grad():
        e_ref, e_gen = R.forward(sd, DIV_CFG, ref01).numpy(), R.forward(sd, DIV_CFG, ds.gen01).numpy()
        yard = max(np.abs(R.forward(sd, DIV_CFG, x, torch.float32).double().numpy() - e).max() for x, e in ((ref01, e_ref), (ds.gen01, e_gen)))
    entropy, counts, props, labels, assigned = diversity_from_embeddings(e_ref, e_gen, GROUPS)
    # stability of the reference's own answer
    move = 2 * 8 * yard * max(np.abs(e_ref).sum(1).max(), np.abs(e_gen).sum(1).max())
    sim = e_ref @ e_ref.T
    same = ds.group.numpy()[:, None] == ds.group.numpy()[None, :]
    assert len({(int(a), int(b)) for a, b in zip(ds.group, labels)}) == GROUPS           # Ward recovers the four prototypes
    assert sim[same].min() - sim[~same].max() > 10 * move
    d_gen = sim.max() - e_gen @ e_ref.T
    mean_d = np.stack([d_gen[:, labels == c].mean(1) for c in range(1, GROUPS + 1)], 1)
    two = np.sort(mean_d, 1)[:, :2]
    assert (two[:, 1] - two[:, 0]).min() > 10 * move
    assert sorted(counts) == sorted(float(n) for n in GEN_COUNTS) and 1.0 < entropy < 2.0

    got = scoring.diversity_against_dataset(ds.gen01.to(dev), ds, dev, num_cluster=GROUPS)
    assert sorted(got) == ["cluster_count", "cluster_proportions", "entropy", "feature_extractor"]
    assert got["feature_extractor"] == "blip_vqa_base-seeded1234"
    assert got["cluster_count"] == counts and got["cluster_proportions"] == props
    assert got["entropy"] == pytest.approx(entropy, abs=1e-12)
    # raw pooler_output, not normalised: the cached reference embeddings are the tower's own, within the tower's bound
    (rkey,) = [k for k in scoring._REF_STATS if k[0] == "div_ref"]
    assert np.abs(scoring._REF_STATS[rkey] - e_ref).max() <= 8 * yard
    scoring._REF_STATS.clear()


# ---------------------------------------------------------------------------------------------------------------
# compute_model_behaviors end to end
# ---------------------------------------------------------------------------------------------------------------
class _ToyDecoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 3, 1)

    def forward(self, x):
        return torch.tanh(F.interpolate(self.conv(x), scale_factor=8.0, mode="nearest"))


def test_sd_behaviours_with_clip_towers_end_to_end(tmp_path, monkeypatch):
    import gad
    from test_gpu_sd import SMALL, rnd
    from text_to_image import compute_model_behaviors as M
    monkeypatch.setitem(vit.PRESETS, "clip_vit_b32", TOWERS["t10"][0])
    monkeypatch.setitem(vit.PRESETS, "clip_vit_l14", TOWERS["t50"][0])
    torch.manual_seed(0)
    dec = tmp_path / "decoder.pt"
    torch.jit.script(_ToyDecoder().eval()).save(str(dec))
    monkeypatch.setenv("GAD_VAE_DECODER_TS", str(dec))
    monkeypatch.setenv("GAD_SD_SCORER", "clip-seeded")
    for v in M.WEIGHT_VARS:
        monkeypatch.delenv(v, raising=False)
    dirs = []
    for j in range(2):                                                       # two LoRAs on one seeded base: reference, coalition
        torch.manual_seed(0)
        net = gad.UNet2DConditionModel(**SMALL).to(dev)
        for i, p in enumerate(net.inject_lora(rank=4)):
            with torch.no_grad():
                p.copy_(rnd(*p.shape, seed=50 + 100 * j + i, scale=0.05))
        dirs.append(tmp_path / f"lora{j}")
        net.save_attn_procs(str(dirs[-1]))
    weights = tmp_path / "unet.pt"
    torch.save({k: v for k, v in net.state_dict().items() if "lora_layer" not in k}, weights)
    pe = tmp_path / "pe.pt"
    torch.save({"cond": rnd(77, 96, seed=1, scale=0.5), "uncond": rnd(77, 96, seed=2, scale=0.5), "clip_prompt": 3 * rnd(32, seed=3)}, pe)
    db, img_dir = str(tmp_path / "db.jsonl"), tmp_path / "img"
    base = ["--reference_lora_dir", str(dirs[0]), "--db", db, "--num_images", "2", "--resolution", "128", "--seed", "42",
            "--unet_overrides", json.dumps(SMALL), "--unet_weights", str(weights), "--num_inference_steps", "2", "--n_noises", "1",
            "--prompt_embeds", str(pe)]
    assert M.main(M.parse_args(base + ["--lora_dir", str(dirs[1]), "--exp_name", "coalition", "--img_dir", str(img_dir)]))
    assert M.main(M.parse_args(base + ["--lora_dir", str(dirs[0]), "--exp_name", "reference"]))
    rows = [json.loads(line) for line in open(db)]
    assert len(rows) == 2
    tag = "clip_vit_b32-seeded1234;clip_vit_l14-seeded1234;aesthetic-seeded1234"
    # the row an unconfigured run writes has exactly these keys (assemble_row is the one writer)
    lists = {b: [0.0, 0.0] for b in M.BEHAVIOURS}
    keys = set(M.assemble_row(types.SimpleNamespace(**{k: None for k in M.REFERENCE_KEYS}), lists, lists, None, None))
    for r in rows:
        assert set(r) == keys and r["feature_extractor"] == tag
        for i in range(2):
            for b in M.BEHAVIOURS:
                assert np.isfinite(r[f"generated_image_{i}_{b}"]) and r[f"generated_image_{i}_{b}_time"] > 0
            assert -1.0 <= r[f"generated_image_{i}_clip_similarity"] <= 1.0 + 1e-6
            assert -1.0 <= r[f"generated_image_{i}_clip_prompt_score"] <= 1.0
    coal, ref = rows
    for i in range(2):
        assert abs(ref[f"generated_image_{i}_clip_similarity"] - 1) <= 1e-5
        assert ref[f"generated_image_{i}_ssim"] == 1.0 and ref[f"generated_image_{i}_nrmse"] == 0.0
        assert coal[f"generated_image_{i}_ssim"] < 1.0
        assert ref[f"generated_image_{i}_aesthetic_score"] != coal[f"generated_image_{i}_aesthetic_score"]
    stored = torch.load(img_dir / "latents_seed=42_sample_0.pt", weights_only=False)
    assert stored["sample_image"].shape == (128, 128, 3) and stored["sample_image"].dtype == torch.uint8
    assert stored["reference"].shape == (1, 4, 16, 16) and set(stored) == {"reference", "sample", "reference_image", "sample_image"}
