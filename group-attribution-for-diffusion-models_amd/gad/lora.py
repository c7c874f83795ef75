"""LoRA unlearning of the unconditional U-Nets (reference unconditional_generation/unlearn.py:404-424, 629-634, 748-749 through
peft): `LoraConfig`, `get_peft_model`, `merge_and_unload` and the LoRA+ parameter groups of `FusedTrainer`.

peft is not a dependency and could not be consulted when this was written; the semantics restated here are from memory of
peft's LoRA layer: y = base(x) + B(A(dropout(x))) * lora_alpha / r, A ~ kaiming_uniform(a = sqrt(5)),
B = 0, every base parameter frozen, dropout active in training mode only.  The three projections of an attention block run
as one autograd node (`ops.LoraDropoutQKVFn`) over csrc/lora.hip: the dropout masks are regenerated in the kernels - the same
Bernoulli(1 - p) distribution as torch's dropout, different draws."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _capi, ops
from .nn import Attention
from .training import _slot

QKV = ("to_q", "to_k", "to_v")


@dataclass
class LoraConfig:
    """The four peft.LoraConfig fields the reference sets (unlearn.py:410-415)"""
    r: int = 8
    lora_alpha: float = 8
    lora_dropout: float = 0.0
    target_modules: tuple = QKV


class LoraQKV(nn.Module):
    """LoRA matrices of one attention block's to_q / to_k / to_v (module order) and the forward through them"""

    def __init__(self, attn: Attention, config: LoraConfig, layer: int, seed: int):
        super().__init__()
        self.r, self.scale, self.p = int(config.r), float(config.lora_alpha) / int(config.r), float(config.lora_dropout)
        self.layer, self.seed, self.calls = layer, seed, 0
        dev = attn.to_q.weight.device
        for name in QKV:
            lin = getattr(attn, name)
            out_f, in_f = lin.weight.shape
            # peft's order of draws from the CPU generator: both nn.Linear constructors initialise themselves, then reset_lora_parameters
            a, b = nn.Linear(in_f, self.r, bias=False), nn.Linear(self.r, out_f, bias=False)
            nn.init.kaiming_uniform_(a.weight, a=math.sqrt(5))
            nn.init.zeros_(b.weight)
            self.register_parameter(f"{name}_A", nn.Parameter(a.weight.detach().to(dev)))
            self.register_parameter(f"{name}_B", nn.Parameter(b.weight.detach().to(dev)))

    def matrices(self):
        """[(projection name, A [r, in], B [out, r])] in module order"""
        return [(n, getattr(self, f"{n}_A"), getattr(self, f"{n}_B")) for n in QKV]

    def forward(self, attn: Attention, h):
        lins = [getattr(attn, n) for n in QKV]
        p = self.p if self.training else 0.0             # nn.Dropout: the identity in eval mode
        if self.training:
            if p > 0 and torch.cuda.is_current_stream_capturing():
                raise _capi.GadError("LoRA dropout inside a hipGraph capture: the mask offset is a host scalar, a replay would repeat one "
                                     "step's masks (train this model with FusedTrainer(use_graph=False))")
            self.calls += 1                              # the mask stream's offset: one per training forward of this block
        mats = self.matrices()
        return ops.lora_dropout_qkv(h, [l.weight for l in lins], [l.bias for l in lins], [a for _, a, _ in mats],
                                    [b for _, _, b in mats], p, self.scale, self.seed, self.calls, self.layer)


def lora_layers(model):
    return [m for m in model.modules() if isinstance(m, Attention) and getattr(m, "lora_qkv", None) is not None]


def get_peft_model(model, config: LoraConfig):
    """Freeze every parameter of `model` and attach LoRA matrices to each attention block's to_q / to_k / to_v, in place.
    -> `model`"""
    targets = set(config.target_modules)
    if targets != set(QKV):
        raise NotImplementedError(f"get_peft_model: target_modules={sorted(targets)}; the fused LoRA attention node covers exactly "
                                  f"{list(QKV)} (the reference's targets, unlearn.py:412)")
    if not (config.r % 4 == 0 and 4 <= config.r <= 64):
        raise _capi.GadError(f"get_peft_model: r={config.r} must be a multiple of 4 in 4..64 (csrc/lora.hip)")
    if not 0.0 <= config.lora_dropout < 1.0:
        raise _capi.GadError(f"get_peft_model: lora_dropout={config.lora_dropout} outside [0, 1)")
    attns = [m for m in model.modules() if isinstance(m, Attention)]
    if not attns:
        raise ValueError("get_peft_model: the model has no attention block, so none of the target modules exists")
    for m in attns:
        if m.dpad != m.dim_head:
            raise NotImplementedError(f"get_peft_model: head-grouped-pruned attention (head dim {m.dim_head}, run with zero-padded heads) is "
                                      "not supported under LoRA: the padded-heads route has no LoRA form (DESIGN.md section 8)")
    for p in model.parameters():
        p.requires_grad_(False)
    seed = torch.initial_seed() & 0xFFFFFFFF             # read, not drawn: the generator is consumed by the matrices alone
    for layer, m in enumerate(attns):
        m.lora_qkv = LoraQKV(m, config, layer, seed)
    model.peft_config = config
    return model


def lora_parameters(model, loraplus_lr_ratio=16.0):
    """(parameters laid out [all A | all B], [(slice of the flat buffer, lr multiplier)]) for `FusedTrainer(params=, groups=)`:
    create_loraplus_optimizer's two groups - the B matrices train at `loraplus_lr_ratio` times the A matrices' rate."""
    mats = [t for m in lora_layers(model) for t in m.lora_qkv.matrices()]
    a, b = [t[1] for t in mats], [t[2] for t in mats]
    na, nb = sum(_slot(p.numel()) for p in a), sum(_slot(p.numel()) for p in b)
    return a + b, [(slice(0, na), 1.0), (slice(na, na + nb), float(loraplus_lr_ratio))]


@torch.no_grad()
def merge_and_unload(model):
    """W += (lora_alpha / r) B A for every adapted projection (gad_lora_merge), then the LoRA layers are removed: sampling
    takes the fused no-LoRA route on plain weights.  The base parameters stay frozen, as peft leaves them.  -> `model`"""
    for m in lora_layers(model):
        lq = m.lora_qkv
        for name, a, b in lq.matrices():
            ops.lora_merge_raw(getattr(m, name).weight.detach(), b.detach().contiguous(), a.detach().contiguous(), lq.scale)
        del m.lora_qkv
    if hasattr(model, "peft_config"):
        del model.peft_config
    ops.written_everywhere()          # the projections were rewritten through device pointers: every derived copy refreshes
    return model
