"""TRAK / D-TRAK gradient features (reference src/attributions/methods/d_trak_grad.py) on the MI355X engine.

`Projector` takes the constructor keys of trak.projectors.CudaProjector (fast_jl, CUDA only) and projects with
gad_jl_project (csrc/projector.hip), which generates the random matrix on the fly.  `gradient_features` computes the
per-sample feature of one image, emb = (1/k) sum_t grad_theta f(x, t), as ONE forward / backward of the fused engine
over the batch of that image's k (noisy, t) rows: the gradient of the batch-mean loss is exactly that average, and it
lands in the model's flat gradient buffer (training.flatten_params), which is staged row by row and projected.

The row index of R is the offset in the flat buffer: conv weights sit in their [Cout][KH][KW][Cin] storage order and
every parameter slot is padded to 8 floats with zeros, so R differs from the reference's vectorisation by a fixed
permutation of rows (and the zero padding contributes nothing).

`lora_gradient_features` is the Stable-Diffusion + LoRA form (reference text_to_image/grad_text_to_image_lora.py, where
vmap(grad(f)) yields the per-sample gradients of a batch): with bf16 activations every LoRA gradient is a contraction over
the token axis, so ONE ordinary forward / backward over S samples x j timesteps writes all S per-sample gradients into S
staging rows (half.per_sample_gradients -> gad_hgemm_tn_seg); with fp32 activations it runs one sample per backward
through the flat buffer, as `gradient_features` does.

`journey_latents` / `journey_gradient_features` are Journey-TRAK's validation side (d_trak_grad.py --calculate_gen_grad, reference
:450-494, :729-731): batched ancestral DDPM trajectories stepped by gad_ddpm_step (csrc/sampler.hip: one launch per step, variance
noise from in-kernel Philox keyed per sample), and the features of their latents taken as they are through the same _GradStep."""
from __future__ import annotations

import ctypes as C
from enum import Enum

import torch

from . import _capi, ops
from ._capi import check


class ProjectionType(str, Enum):
    normal = "normal"
    rademacher = "rademacher"


_TYPES = {ProjectionType.normal: _capi.JL_NORMAL, ProjectionType.rademacher: _capi.JL_RADEMACHER}


def jl_args(a, lda, G, P, d, seed, model_id=0, proj_type=ProjectionType.normal, p0=0, accumulate=False, out=None,
            workspace=None, workspace_bytes=0) -> _capi.JLArgs:
    """gad_jl_args from plain values / tensors (data pointers are read from tensors; ints are taken as addresses)"""
    def ptr(x):
        return None if x is None else (x.data_ptr() if torch.is_tensor(x) else int(x))
    args = _capi.JLArgs()
    args.A, args.lda, args.G, args.P, args.p0, args.d = ptr(a), lda, G, P, p0, d
    args.seed, args.model_id = seed & 0xFFFFFFFF, model_id & 0xFFFFFFFF
    args.type, args.accumulate = _TYPES[ProjectionType(proj_type)], int(bool(accumulate))
    args.out, args.workspace, args.workspace_bytes = ptr(out), ptr(workspace), workspace_bytes
    return args


def workspace_bytes(G, P, d, proj_type=ProjectionType.normal) -> int:
    n = _capi.load().gad_jl_project_workspace_bytes(C.byref(jl_args(None, (P + 3) // 4 * 4, G, P, d, 0, proj_type=proj_type)))
    if n < 0:
        raise _capi.GadError(f"gad_jl_project_workspace_bytes: {_capi.load().gad_last_error().decode()}")
    return n


def project_raw(a, out, P, seed, model_id=0, proj_type=ProjectionType.normal, p0=0, accumulate=False, workspace=None):
    """out[G][d] (+)= a[G][:P] @ R[p0 : p0 + P] in one launch on the current stream.  `a`: fp32 device rows with a row
    stride that is a multiple of 4; `out`: contiguous fp32 [G][d]; `workspace`: a uint8 device tensor (allocated here
    if None)."""
    ops._req(out, "jl out")
    if not (a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1):
        raise _capi.GadError(f"jl A: expected fp32 device rows with unit column stride, got {a.dtype} {a.device} {a.stride()}")
    G, d = out.shape
    if a.shape[0] != G or not 0 < P <= a.shape[1]:
        raise _capi.GadError(f"jl: A {tuple(a.shape)} does not hold {G} rows of P={P} entries")
    need = workspace_bytes(G, P, d, proj_type)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=out.device)
    args = jl_args(a, a.stride(0), G, P, d, seed, model_id, proj_type, p0, accumulate, out, workspace, workspace.numel())
    check(_capi.load().gad_jl_project(C.byref(args), ops._stream()), "gad_jl_project")
    return out


class Projector:
    """Drop-in for trak.projectors.CudaProjector(grad_dim, proj_dim, seed, proj_type, device, max_batch_size).

    R has unit-variance entries and no 1/sqrt(proj_dim) scale (TRAK's scores and the cosine of vanilla_gradient do not
    change under a global scale of the features).  proj_dim must be a multiple of 64."""

    def __init__(self, grad_dim, proj_dim, seed, proj_type=ProjectionType.normal, device="cuda", max_batch_size=32,
                 *args, **kwargs):
        self.grad_dim, self.proj_dim, self.seed = int(grad_dim), int(proj_dim), int(seed)
        self.proj_type = ProjectionType(proj_type)
        self.device = torch.device(device)
        self.max_batch_size = int(max_batch_size)
        self.workspace = torch.empty(workspace_bytes(self.max_batch_size, self.grad_dim, self.proj_dim, self.proj_type),
                                     dtype=torch.uint8, device=self.device)

    def project(self, grads, model_id, out=None, p0=0, accumulate=False):
        """[G][grad_dim] fp32 gradient rows -> [G][proj_dim] features (rows in chunks of max_batch_size; a row's result does
        not depend on the chunking).  `p0` / `accumulate` project a column chunk of longer rows into `out`."""
        if grads.dim() != 2 or grads.shape[1] > self.grad_dim - p0:
            raise ValueError(f"grads {tuple(grads.shape)}: expected [G][<= {self.grad_dim - p0}] rows")
        if grads.dtype != torch.float32 or grads.device != self.device:
            grads = grads.to(self.device, torch.float32)
        P = grads.shape[1]
        if grads.stride(1) != 1 or grads.stride(0) % 4 or grads.data_ptr() % 16:
            padded = torch.zeros(grads.shape[0], (P + 3) // 4 * 4, device=self.device)
            padded[:, :P] = grads
            grads = padded
        if out is None:
            out = torch.empty(grads.shape[0], self.proj_dim, device=self.device)
        for r in range(0, grads.shape[0], self.max_batch_size):
            project_raw(grads[r:r + self.max_batch_size], out[r:r + self.max_batch_size], P, self.seed, model_id,
                        self.proj_type, p0, accumulate, self.workspace)
        return out


BEHAVIOURS = ("loss", "mean-squared-l2-norm", "mean", "l1-norm", "l2-norm", "linf-norm")


def _seed_gradient(pred, behaviour):
    """d(mean over the k rows of f(row)) / d pred for the behaviours that are not an MSE (tiny torch ops on pred)."""
    p = pred.detach().reshape(pred.shape[0], -1).requires_grad_(True)
    if behaviour == "mean":
        f = p.mean(dim=1)
    else:
        f = torch.linalg.vector_norm(p, ord={"l1-norm": 1, "l2-norm": 2, "linf-norm": float("inf")}[behaviour], dim=1)
    (g,) = torch.autograd.grad(f.mean(), p)
    return g.reshape(pred.shape).contiguous()


class _GradStep:
    """(add_noise ->) U-Net -> behaviour (+ its gradient) -> backward into the flat gradient buffer of `model`.
    `add_noise=False` feeds x to the U-Net as it is (Journey-TRAK: x is a latent of the generation trajectory)."""

    def __init__(self, model, scheduler, behaviour):
        if behaviour not in BEHAVIOURS:
            raise NotImplementedError(f"--model_behavior {behaviour}: not ported (the engine computes {', '.join(BEHAVIOURS)})")
        self.model, self.scheduler, self.behaviour = model, scheduler, behaviour
        self.flat, self.gflat = model.flatten_parameters() if model._flat is None else model.flat
        self.params = list(model.parameters())
        self._unwritten = None

    def __call__(self, x, noise, t, add_noise=True):
        noisy = self.scheduler.add_noise(x, noise, t) if add_noise else x
        pred = self.model(noisy, t).sample.contiguous()
        if self.behaviour == "loss":                              # TRAK: MSE(pred, eps)
            _, d = ops.mse_fwd_bwd_raw(pred, noise.contiguous())
        elif self.behaviour == "mean-squared-l2-norm":            # D-TRAK: MSE(pred, 0)
            _, d = ops.mse_fwd_bwd_raw(pred, torch.zeros_like(pred))
        else:
            d = _seed_gradient(pred, self.behaviour)
        ops.begin_backward_step()
        try:
            pred.backward(d)
        finally:
            ops.end_backward_step()
        if self._unwritten is None:                               # a parameter with no gradient keeps a stale slot
            ep = ops._SINK_EPOCH[0]
            self._unwritten = [p._gad_sink for p in self.params if getattr(p, "_gad_sink_epoch", -1) != ep]
        for v in self._unwritten:
            v.zero_()
        return self.gflat


def selected_timesteps(t_strategy, k_partition, num_train_timesteps=1000):
    """d_trak_grad.py:625-628"""
    if t_strategy == "uniform":
        return list(range(0, num_train_timesteps, num_train_timesteps // k_partition))
    if t_strategy == "cumulative":
        return list(range(0, k_partition))
    raise ValueError(f"t_strategy={t_strategy}")


def gradient_features(model, scheduler, images, behaviour, timesteps, projector: Projector, opt_seed=42, batch_size=8,
                      model_id=0, out=None):
    """[N][proj_dim] TRAK (`loss`) / D-TRAK (`mean-squared-l2-norm`) features of `images` [N][C][H][W] (dataset order).

    Noise follows the reference (d_trak_grad.py:630-638): per data batch of `batch_size` images and per t,
    seed_everything(opt_seed * 1000 + t) and one standard-normal draw of the batch's shape on the device.  The model runs in
    eval mode (vmap's default randomness='error' forces the same in the reference).  Rows are staged in a
    [projector.max_batch_size][P] buffer and every full buffer is projected with one launch.  `out`: an optional host
    array (e.g. np.memmap) that receives each projected block as it is done; the features are returned as a CPU tensor."""
    return _feature_rows(model, scheduler, images, behaviour, timesteps, projector, opt_seed, batch_size, model_id, out,
                         as_is=False, scale=1.0)


def _feature_rows(model, scheduler, images, behaviour, timesteps, projector, opt_seed, batch_size, model_id, out, as_is, scale):
    """The body of gradient_features and journey_gradient_features.  as_is=False: images [N][C][H][W], a sample's k rows are its
    image noised at the k timesteps.  as_is=True: images [N][>= k][C][H][W], its k rows are images[i][:k], fed to the U-Net as
    they are.  Either way the noise draw (the `loss` target) follows the reference's rule, and the staged row is `scale` x the
    mean over the k rows of grad f."""
    from .coalition import seed_everything
    dev = projector.device
    step = _GradStep(model, scheduler, behaviour)
    P = step.gflat.numel()
    if P != projector.grad_dim:
        raise ValueError(f"projector.grad_dim={projector.grad_dim} but the model's flat gradient has {P} entries")
    was_training = model.training
    model.eval()
    k = len(timesteps)
    ts = torch.tensor(list(timesteps), device=dev, dtype=torch.long)
    N = images.shape[0]
    feats = torch.empty(N, projector.proj_dim)
    G = projector.max_batch_size
    staging = torch.empty(G, P, device=dev)
    block = torch.empty(G, projector.proj_dim, device=dev)
    filled, row0 = 0, 0

    def flush():
        nonlocal filled, row0
        projector.project(staging[:filled], model_id, out=block[:filled])
        feats[row0:row0 + filled] = block[:filled].cpu()
        if out is not None:
            out[row0:row0 + filled] = feats[row0:row0 + filled].numpy()
        row0 += filled
        filled = 0

    try:
        for b0 in range(0, N, batch_size):
            image = images[b0:b0 + batch_size].to(dev, torch.float32)
            like = torch.empty((image.shape[0],) + tuple(image.shape[-3:]), device=dev)   # the reference's batch: [bsz][C][H][W]
            noises = []
            for t in timesteps:
                seed_everything(opt_seed * 1000 + t)
                noises.append(torch.randn_like(like))
            noise = torch.stack(noises, dim=1)                   # [bsz][k][C][H][W]
            for i in range(image.shape[0]):
                x = image[i, :k].contiguous() if as_is else image[i:i + 1].expand(k, *image.shape[1:]).contiguous()
                gflat = step(x, noise[i].contiguous(), ts, add_noise=not as_is)
                if scale == 1.0:
                    staging[filled].copy_(gflat)
                else:
                    torch.mul(gflat, scale, out=staging[filled])
                filled += 1
                if filled == G:
                    flush()
        if filled:
            flush()
    finally:
        model.train(was_training)
    return feats


def journey_timesteps(k_partition, num_train_timesteps=1000):
    """The timesteps a Journey-TRAK trajectory visits (d_trak_grad.py:472): T - 1 downwards in strides of T // k.  Their
    count is ceil(T / (T // k)), which is k only when k divides T (k = 3: [999, 666, 333, 0])."""
    T = int(num_train_timesteps)
    return list(range(T - 1, -1, -(T // int(k_partition))))


def journey_seeds(opt_seed, samples):
    """The 64-bit noise key of every sample, (opt_seed << 32) | sample, as int64 values (two's complement)"""
    keys = [((int(opt_seed) & 0xFFFFFFFF) << 32) | (int(s) & 0xFFFFFFFF) for s in samples]
    return [v - (1 << 64) if v >= 1 << 63 else v for v in keys]


@torch.no_grad()
def journey_latents(model, scheduler, n_samples, k_partition, opt_seed=42, batch_size=64, posterior_steps=100, device=None):
    """[n_samples][K][C][H][W] (CPU): the latents of n_samples ancestral DDPM trajectories (d_trak_grad.py:450-483), K =
    len(journey_timesteps(k_partition)).

    As in the reference (:481), index j of a row is the latent that ENTERED the U-Net at journey_timesteps[K - 1 - j]: index
    K - 1 is the initial noise, and index 0 is the input of the last visited timestep - not a finished image (the reference's
    last forward and step produce a tensor it never stores, so only K - 1 forwards and steps are run here).  Row s starts from
    torch.randn((1, C, H, W), generator=torch.Generator(device).manual_seed(s), device=device), the reference's per-sample
    seeded draw.  The posterior of a step at t is taken towards prev_t = t - T // posterior_steps (abar_prev = 1 when
    prev_t < 0): the reference sets num_inference_steps = 100 whatever k_partition is (:455-456), and the default keeps that.

    Deliberate deviation: the variance noise of row s is keyed by (opt_seed << 32) | s and generated inside gad_ddpm_step
    (Philox, counter (element >> 2, t, 0, 2)), so a trajectory is reproducible and does not depend on batch_size or on the
    rows it shares a launch with; the reference draws it from the unseeded global generator.  Rows run in batches of
    `batch_size` through a device slab [K][rows][C][H][W]: the U-Net reads slice i and the step writes slice i + 1."""
    c = scheduler.config
    if c.prediction_type != "epsilon" or c.thresholding or c.variance_type not in ops._DDPM_VARIANCE:
        raise NotImplementedError("journey_latents: epsilon prediction with fixed_small / fixed_large variance only")
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    T = int(c.num_train_timesteps)
    ts = journey_timesteps(k_partition, T)
    K = len(ts)
    stride = T // int(posterior_steps)
    ss = model.config.sample_size
    H, W = ss if isinstance(ss, (tuple, list)) else (ss, ss)
    C_in = model.config.in_channels
    rows = max(1, min(int(batch_size), int(n_samples)))
    slab = torch.empty(K, rows, C_in, H, W, device=dev)
    tdev = torch.empty(rows, device=dev, dtype=torch.int64)
    out = torch.empty(n_samples, K, C_in, H, W)
    was_training = model.training
    model.eval()
    try:
        for s0 in range(0, n_samples, rows):
            n = min(rows, n_samples - s0)
            for r in range(n):
                slab[0, r] = torch.randn((1, C_in, H, W), generator=torch.Generator(dev).manual_seed(s0 + r), device=dev)[0]
            seeds = torch.tensor(journey_seeds(opt_seed, range(s0, s0 + n)), dtype=torch.int64, device=dev)
            for i, t in enumerate(ts[:-1]):
                tdev.fill_(t)
                eps = model(slab[i, :n], tdev[:n]).sample.contiguous()
                ops.ddpm_step_raw(slab[i, :n], eps, seeds, t, *scheduler.alpha_pair(t, t - stride), scheduler.clip, c.variance_type,
                                  out=slab[i + 1, :n])
            out[s0:s0 + n] = slab[:, :n].flip(0).transpose(0, 1).cpu()
    finally:
        model.train(was_training)
    return out


def journey_gradient_features(model, scheduler, latents, behaviour, timesteps, projector: Projector, opt_seed=42, batch_size=8,
                              model_id=0, out=None, k_partition=None):
    """[N][proj_dim] Journey-TRAK features of the trajectories `latents` [N][K][C][H][W] (journey_latents); gradient_features'
    contract otherwise.  Row i's k = len(timesteps) rows are latents[i][index_t] evaluated at timesteps[index_t] as they are -
    no add_noise (d_trak_grad.py:729-731).  The `loss` target is the noise drawn by gradient_features' rule
    (seed_everything(opt_seed * 1000 + t), one draw of the data batch's [bsz][C][H][W]).  The sum over the rows is divided by
    `k_partition` as the reference does (:770), not by the number of rows (they differ when k does not divide T); None: k.

    Kept from the reference: with --t_strategy uniform the gradient at index j is taken at t = j (T // k), while the latent at
    index j entered the U-Net at journey_timesteps[K - 1 - j] = j (T // k) + (T // k - 1) when k divides T."""
    k = len(timesteps)
    if latents.dim() != 5 or latents.shape[1] < k:
        raise ValueError(f"latents {tuple(latents.shape)}: expected [N][K >= {k}][C][H][W]")
    return _feature_rows(model, scheduler, latents, behaviour, timesteps, projector, opt_seed, batch_size, model_id, out,
                         as_is=True, scale=k / float(k_partition if k_partition is not None else k))


def _per_row_seed(pred, target, behaviour):
    """d f(row) / d pred for every row of the batch (f is a mean over the row's own elements, so rows do not mix)"""
    B = pred.shape[0]
    if behaviour == "loss":                                       # B x the gradient of the batch-mean MSE
        return ops.mse_fwd_bwd_raw(pred, target.contiguous(), float(B))[1]
    if behaviour == "mean-squared-l2-norm":
        return ops.mse_fwd_bwd_raw(pred, torch.zeros_like(pred), float(B))[1]
    return _seed_gradient(pred, behaviour) * B


def lora_flat_gradient(model):
    """(LoRA parameters, their flat gradient buffer): the trainable parameters of a gad.sd.UNet2DConditionModel with injected LoRA,
    re-homed in one flat buffer (training.flatten_params) unless a trainer already did that"""
    from .training import flatten_params
    params = [p for p in model.parameters() if p.requires_grad]
    if not params or any(p.dim() != 2 for p in params):
        raise ValueError("lora_gradient_features: the trainable parameters must be LoRA matrices (model.inject_lora / load_attn_procs)")
    homes = {id(getattr(p, "_gad_flat", (None,))[0]) for p in params}
    if len(homes) != 1 or getattr(params[0], "_gad_flat", None) is None:
        flatten_params(params)
    return params, params[0]._gad_flat[0]._gad_grad


def lora_per_sample_gradients(model, scheduler, latents, contexts, timesteps, behaviour, rows_per_block, noise=None, seed=42,
                              samples_per_backward=None, timesteps_per_backward=None, device=None):
    """Generator of (first row, staging[:n]) per block of `rows_per_block` rows: staging[i] is the flat gradient
    (1/k) sum_c grad_theta f(eps_theta(add_noise(latents[i], noise[i][c], timesteps[i][c]), timesteps[i][c], contexts[i])) over the LoRA
    matrices theta of `model` (gad.sd.UNet2DConditionModel), f as BEHAVIOURS.  The buffer is reused by the next block.

    latents [N][C][H][W], contexts [N][T][D], timesteps [N][k] (or [k]: the same for every row) - `--source train / generated`: k
    selected timesteps of an image; `generated_journey`: k noise draws at the row's own t.  noise: [N][k][C][H][W], or None: drawn
    per block from a device generator seeded with `seed` (so a row's noise does not depend on the route or on the two chunk
    sizes below).

    bf16 activations (ops.half_activations()): each backward carries S = samples_per_backward rows x j = timesteps_per_backward of
    their timesteps; the average over k is accumulated over the ceil(k / j) chunks with alpha = 1 / k (gad_hgemm_tn_seg).  fp32
    activations: one row per backward, its timesteps in chunks of j, through the flat gradient buffer."""
    from . import half
    if behaviour not in BEHAVIOURS:
        raise NotImplementedError(f"--f {behaviour}: not ported (the engine computes {', '.join(BEHAVIOURS)})")
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    params, gflat = lora_flat_gradient(model)
    P = gflat.numel()
    N = latents.shape[0]
    ts_all = torch.as_tensor(timesteps, dtype=torch.long)
    if ts_all.dim() == 1:
        ts_all = ts_all.expand(N, -1)
    k = ts_all.shape[1]
    G = int(rows_per_block)
    segmented = ops.half_activations()
    S_max = min(int(samples_per_backward or G), G) if segmented else 1
    j = min(int(timesteps_per_backward or (1 if segmented else k)), k)
    was_training = model.training
    model.eval()
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    staging = torch.zeros(G, P, device=dev)                       # slot padding and never-written slots stay zero
    try:
        for g0 in range(0, N, G):
            n = min(G, N - g0)
            x_blk = latents[g0:g0 + n].to(dev, torch.float32)
            c_blk = contexts[g0:g0 + n].to(dev, torch.float32)
            t_blk = ts_all[g0:g0 + n].to(dev)
            if noise is None:
                e_blk = torch.randn((n, k) + tuple(x_blk.shape[1:]), device=dev, generator=gen)
            else:
                e_blk = noise[g0:g0 + n].to(dev, torch.float32)
            for s0 in range(0, n, S_max):
                S = min(S_max, n - s0)
                for c0 in range(0, k, j):
                    jj = min(j, k - c0)

                    def rep(v):
                        return v[s0:s0 + S].unsqueeze(1).expand(S, jj, *v.shape[1:]).reshape(S * jj, *v.shape[1:]).contiguous()
                    eps = e_blk[s0:s0 + S, c0:c0 + jj].reshape(S * jj, *x_blk.shape[1:]).contiguous()
                    t = t_blk[s0:s0 + S, c0:c0 + jj].reshape(S * jj).contiguous()
                    pred = model(scheduler.add_noise(rep(x_blk), eps, t), t, rep(c_blk)).sample.contiguous()
                    d = _per_row_seed(pred, eps, behaviour)
                    if segmented:
                        with half.per_sample_gradients(staging, s0, S, alpha=1.0 / k, accumulate=c0 > 0):
                            pred.backward(d)
                        continue
                    ops.begin_backward_step()
                    try:
                        pred.backward(d)                          # the flat buffer: sum over the chunk's jj rows of grad f
                    finally:
                        ops.end_backward_step()
                    ep = ops._SINK_EPOCH[0]
                    for p in params:
                        if getattr(p, "_gad_sink_epoch", -1) != ep:
                            p._gad_sink.zero_()
                    if c0 == 0:
                        torch.mul(gflat, 1.0 / k, out=staging[s0])
                    else:
                        staging[s0].add_(gflat, alpha=1.0 / k)
            yield g0, staging[:n]
    finally:
        model.train(was_training)


def lora_gradient_features(model, scheduler, latents, contexts, timesteps, behaviour, projector: Projector, noise=None,
                           seed=42, samples_per_backward=None, timesteps_per_backward=None, model_id=0, out=None):
    """[N][proj_dim] features: the rows of lora_per_sample_gradients (its arguments), each block of projector.max_batch_size rows
    projected with one gad_jl_project launch (its workspace is 16 MiB at P = 5e7, d = 32768, G = 16: slabs x G x d floats, 8 slabs).
    Row index of R = offset in the flat gradient buffer (module docstring).  `out`: an optional host array that receives each
    projected block as it is done; the features are returned as a CPU tensor."""
    _, gflat = lora_flat_gradient(model)
    if gflat.numel() != projector.grad_dim:
        raise ValueError(f"projector.grad_dim={projector.grad_dim} but the model's flat gradient has {gflat.numel()} entries")
    feats = torch.empty(latents.shape[0], projector.proj_dim)
    block = torch.empty(projector.max_batch_size, projector.proj_dim, device=projector.device)
    for g0, rows in lora_per_sample_gradients(model, scheduler, latents, contexts, timesteps, behaviour, projector.max_batch_size,
                                              noise, seed, samples_per_backward, timesteps_per_backward, projector.device):
        n = rows.shape[0]
        projector.project(rows, model_id, out=block[:n])
        feats[g0:g0 + n] = block[:n].cpu()
        if out is not None:
            out[g0:g0 + n] = feats[g0:g0 + n].numpy()
    return feats
