"""Test-side restatement of influence unlearning (reference unconditional_generation/unlearn.py:509-546 and
src/unlearn/Wfisher.py), written from the formulas, in fp64, over explicit (image, noise, timesteps) batches:

    get_grad          G(batches) = sum_b len(b) * grad_theta mean-MSE(eps_theta(add_noise(x_b, e_b, t_b), t_b), e_b)   (eval mode)
    weighting         R = G(remaining) * f / ((f + r) r),   F = G(removed) / (f + r)       f, r: the two counts
    woodfisher_diff   k = F - R;  first batch: o = g;  later: tmp = o.g, k -= (k.g) / (N + tmp) o, o -= tmp / (N + tmp) o   (N = r)
    apply_perturb     theta += ratio * k

Vectors are in `torch.cat([p.view(-1) for p in model.parameters()])` order.  Never imported by the product."""
import copy
import types

import torch


class ToyEps(torch.nn.Module):
    """Two small convolutions and a timestep embedding; `model(x, t).sample` like a diffusers U-Net."""

    def __init__(self, channels=24, num_train_timesteps=50):
        super().__init__()
        self.conv_in = torch.nn.Conv2d(3, channels, 3, padding=1)
        self.time = torch.nn.Embedding(num_train_timesteps, channels)
        self.conv_out = torch.nn.Conv2d(channels, 3, 3, padding=1)

    def forward(self, x, t):
        h = torch.tanh(self.conv_in(x) + self.time(t)[:, :, None, None])
        return types.SimpleNamespace(sample=self.conv_out(h))


class ToyScheduler:
    """Stand-in with what get_grad / woodfisher_diff read of a scheduler: add_noise and config.num_train_timesteps"""

    def __init__(self, num_train_timesteps=50):
        self.config = types.SimpleNamespace(num_train_timesteps=num_train_timesteps)
        betas = torch.linspace(1e-3, 0.2, num_train_timesteps, dtype=torch.float64)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0)

    def add_noise(self, x, noise, t):
        ac = self.alphas_cumprod.to(x.dtype)[t].view(-1, 1, 1, 1)
        return ac.sqrt() * x + (1 - ac).sqrt() * noise


def as_double(model):
    m = copy.deepcopy(model).double()
    m.eval()
    return m


def batch_gradient(model64, scheduler, image, noise, t):
    """fp64 gradient of the batch-mean MSE in torch.cat order; `model64` is a double model in eval mode"""
    image, noise = image.double(), noise.double()
    pred = model64(scheduler.add_noise(image, noise, t), t).sample
    loss = torch.nn.functional.mse_loss(pred, noise)
    grads = torch.autograd.grad(loss, list(model64.parameters()))
    return torch.cat([g.reshape(-1) for g in grads])


def gradient_sum(model64, scheduler, batches):
    total = torch.zeros(sum(p.numel() for p in model64.parameters()), dtype=torch.float64)
    for image, noise, t in batches:
        total += image.shape[0] * batch_gradient(model64, scheduler, image, noise, t)
    return total


def woodfisher(model64, scheduler, batches, N, v):
    k, o = v.double().clone(), None
    for image, noise, t in batches:
        g = batch_gradient(model64, scheduler, image, noise, t)
        if o is None:
            o = g.clone()
            continue
        tmp, kg = torch.dot(o, g), torch.dot(k, g)
        k = k - kg / (N + tmp) * o
        o = o - tmp / (N + tmp) * o
    return k


def distinct_labels(label_batches):
    seen = set()
    for labels in label_batches:
        seen.update(int(l) for l in labels)
    return len(seen)


def weighted(forget_sum, retain_sum, forget_count, retain_count):
    """(F, R) of unlearn.py:528-531"""
    R = retain_sum * (forget_count / ((forget_count + retain_count) * retain_count))
    F = forget_sum / (forget_count + retain_count)
    return F, R


def delta_w(model, scheduler, removed, remaining, remaining_again, forget_count, retain_count):
    """The whole IU vector and its two weighted gradient sums (F, R)"""
    m = as_double(model)
    F, R = weighted(gradient_sum(m, scheduler, removed), gradient_sum(m, scheduler, remaining), forget_count, retain_count)
    return woodfisher(m, scheduler, remaining_again, retain_count, F - R), F, R


class InfluenceUnlearner:
    """The surface of gad.InfluenceUnlearner on the functions above, over any torch model (the CPU oracle's U-Net)"""

    def __init__(self, model, scheduler):
        self.model, self.scheduler = model, scheduler
        self.calls = []                                   # (method, what the entry point passed): read by the tests

    def gradient_sum(self, batches):
        batches = list(batches)
        self.calls.append(("gradient_sum", len(batches)))
        return gradient_sum(as_double(self.model), self.scheduler, batches)

    def woodfisher(self, batches, N, v):
        batches = list(batches)
        self.calls.append(("woodfisher", len(batches), N))
        return woodfisher(as_double(self.model), self.scheduler, batches, N, v)

    @torch.no_grad()
    def apply(self, delta, ratio):
        self.calls.append(("apply", float(ratio), float(delta.abs().max())))
        off = 0
        for p in self.model.parameters():
            n = p.numel()
            p.add_((ratio * delta[off:off + n]).view(p.shape).to(p.dtype))
            off += n
