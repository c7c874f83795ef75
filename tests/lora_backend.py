"""Test-only backend namespace for `unlearn.py --method lora` without a GPU: tests/oracle_backend.py plus the LoRA names the
entry point takes from `gad`, served by tests/lora_ref.py on the CPU oracle model and torch.optim.  Never imported by the product."""
import types

import torch

import lora_ref as LR
import oracle_backend as OB
from gad.lora import LoraConfig  # noqa: F401  (a plain dataclass)


def make():
    """a fresh namespace; `ns.log` records what the entry point asked for"""
    ns = types.SimpleNamespace(**{k: getattr(OB, k) for k in dir(OB) if not k.startswith("_")})
    ns.LoraConfig = LoraConfig
    ns.log = []

    def get_peft_model(model, config):
        ns.log.append(("get_peft_model", config.r, config.lora_alpha, config.lora_dropout, tuple(config.target_modules)))
        return LR.get_peft_model(model, config.r, config.lora_alpha, config.lora_dropout, torch.initial_seed() & 0xFFFFFFFF)

    def lora_parameters(model, ratio=16.0):
        layers = [l for ls in LR.lora_layers(model) for l in ls]
        ns.log.append(("lora_parameters", len(layers), ratio))
        return [l.A for l in layers] + [l.B for l in layers], [(len(layers), 1.0), (len(layers), float(ratio))]

    def merge_and_unload(model):
        ns.log.append(("merge_and_unload", sum(float(l.B.detach().abs().sum()) for ls in LR.lora_layers(model) for l in ls)))
        return LR.merge_and_unload(model)

    class FusedTrainer:
        """gad.FusedTrainer's LoRA surface on torch.optim.Adam: `groups` here are (parameter count, lr multiplier) runs of `params`"""

        def __init__(self, model, scheduler, ema, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adamw=False,
                     max_grad_norm=1.0, loss_sign=1.0, params=None, groups=None):
            assert ema is None and params is not None and groups is not None and weight_decay == 0.0 and loss_sign == 1.0
            runs, i = [], 0
            for n, mult in groups:
                runs.append({"params": params[i:i + n], "lr": lr * mult})
                i += n
            assert i == len(params)
            self.opt = torch.optim.Adam(runs, lr=lr, betas=betas, eps=eps)
            self.model, self.scheduler, self.params, self.max_norm, self.steps = model, scheduler, params, max_grad_norm, 0
            ns.log.append(("FusedTrainer", lr, [g["lr"] for g in runs]))

        def step(self, image, noise, timesteps):
            self.steps += 1
            LR.set_offset(self.model, self.steps)
            self.model.train()
            self.opt.zero_grad()
            eps = self.model(self.scheduler.add_noise(image, noise, timesteps), timesteps).sample
            loss = torch.nn.functional.mse_loss(eps, noise)
            loss.backward()
            assert all(p.grad is None for p in self.model.parameters() if not p.requires_grad)
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
            self.opt.step()
            return loss.detach()

    ns.get_peft_model, ns.lora_parameters, ns.merge_and_unload, ns.FusedTrainer = get_peft_model, lora_parameters, merge_and_unload, FusedTrainer
    return ns
