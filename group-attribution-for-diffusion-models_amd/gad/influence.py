"""Influence unlearning (IU): the WoodFisher perturbation of the reference's `--method iu`
(unconditional_generation/unlearn.py:509-546, src/unlearn/Wfisher.py) on the flat parameter buffers.

`InfluenceUnlearner` computes the three pieces the entry point combines: the size-weighted gradient sum of a loader
(`get_grad`), the WoodFisher inverse-Hessian-vector product over a loader (`woodfisher_diff`) and the parameter update
(`apply_perturb`).  Every gradient is `trak._GradStep(model, scheduler, "loss")`: the eval-mode gradient of the batch-mean MSE,
left in the model's flat gradient buffer with no host sync.  The recursion itself is two launches per batch, gad_wf_dots and
gad_wf_update (csrc/influence.hip); its coefficients stay on the device.

All vectors are in flat-buffer order (training.flatten_params): conv weights [Cout][KH][KW][Cin], every slot padded to 8
floats with zeros - a fixed permutation of the reference's torch.cat order, and every quantity here is a dot product or an
elementwise update, so the result is the same vector under that permutation.  A gradient's padding is zero and stays zero
in every vector derived from it.  At P = 35.75 M the entry point holds about four P-vectors beside the model (0.6 GB): the
two gradient sums (their difference is formed in place) and the recursion's k and o."""
from __future__ import annotations

import torch

from . import ops
from .trak import _GradStep


class InfluenceUnlearner:
    """`batches` is always an iterable of (image, noise, timesteps) on the model's device: the RNG policy stays with the caller,
    as with FusedTrainer.step.  The model runs in eval mode inside each method and gets its mode back afterwards."""

    def __init__(self, model, scheduler):
        self.model = model
        self.step = _GradStep(model, scheduler, "loss")
        self.flat, self.gflat = self.step.flat, self.step.gflat
        self._o = None                                                    # allocated by the first woodfisher()
        self._dots = torch.zeros(2, dtype=torch.float64, device=self.gflat.device)

    def _gradients(self, batches):
        was_training = self.model.training
        self.model.eval()
        try:
            for image, noise, timesteps in batches:
                yield image.shape[0], self.step(image, noise, timesteps)
        finally:
            self.model.train(was_training)

    def gradient_sum(self, batches) -> torch.Tensor:
        """sum over batches b of len(b) * grad mean-MSE(b) (Wfisher.py:108-111), in a buffer of its own"""
        total = torch.zeros_like(self.gflat)
        for n, g in self._gradients(batches):
            total.add_(g, alpha=float(n))
        return total

    def woodfisher(self, batches, N, v) -> torch.Tensor:
        """k after the recursion over `batches` (Wfisher.py:136-207): k = v; the first batch sets o = g; every later batch
        runs  k -= (k.g) / (N + o.g) * o,  o -= (o.g) / (N + o.g) * o  with the old o."""
        if v.shape != self.gflat.shape:
            raise ValueError(f"woodfisher: v has {tuple(v.shape)} entries, the flat gradient {tuple(self.gflat.shape)}")
        k = v.to(self.gflat.device, torch.float32).clone()
        if self._o is None:
            self._o = torch.empty_like(self.gflat)
        o, first = self._o, True
        for _, g in self._gradients(batches):
            if first:
                o.copy_(g)
                first = False
            else:
                ops.wf_dots_raw(o, k, g, self._dots)
                ops.wf_update_raw(o, k, self._dots, float(N))
        return k

    @torch.no_grad()
    def apply(self, delta, ratio):
        """flat += ratio * delta on the model's flat parameter buffer (apply_perturb, Wfisher.py:12-21)"""
        flat = self.flat
        if delta.shape != flat.shape:
            raise ValueError(f"apply: delta has {tuple(delta.shape)} entries, the flat parameter buffer {tuple(flat.shape)}")
        flat.add_(delta.to(flat.device, torch.float32), alpha=float(ratio))
        # the parameters are views with version counters of their own: what is derived from them (rotated 3x3 weights, Winograd
        # panels, bf16 casts, fused projections) keys on the buffer's epoch, as after the raw optimizer kernel
        ops.written(flat)
