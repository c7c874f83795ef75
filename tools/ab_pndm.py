"""PNDM (PLMS) sampler: the fused guided step (csrc/sampler.hip) against the same update written in torch ops and against the
guided DDIM step it stands beside.  One process, per shape ([16][4][64][64] and [64][4][32][32] latents, guidance 7.5):

  plms      PNDMScheduler's launch in its costliest mode - a guided four-term step that pushes into the ring, in place:
            x, eps_u, eps_c and three stored predictions read, x_prev and the pushed prediction written, 32 B per element
  torch     the same update in torch elementwise ops on the same buffers (guidance, the four-term combination, the transfer,
            a copy into the ring): what a port of diffusers' step_plms costs
  ddim      gad_cfg_ddim_step, in place: x and the doubled eps read, x_prev written, 16 B per element

Bytes are the algorithm's; GB/s = those bytes over the measured time, next to the fraction of the 6.3 TB/s a float4 copy reaches.
At these sizes (1 MB tensors) every version is expected to be bound by how fast the host enqueues launches, as
profiles/journey_ab.txt found for the DDPM step: the figure is then a launch count, not a bandwidth.

Method: device events around `ITERS` back-to-back calls after a warm-up of the same shape; `ROUNDS` rounds with the versions
alternating inside each round; median and min .. max over the rounds.  tests/test_gpu_pndm.py holds the kernel to fp64.

Run by hand on the GPU under a time limit:
    timeout -k 10 300 python tools/ab_pndm.py --out profiles/pndm_ab.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

dev = torch.device("cuda:0")
ITERS, ROUNDS, WARM = 500, 5, 20
HBM = 6.3e12                                                     # what a float4 copy reaches on the MI355X
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def alternate(fns, iters=ITERS, warm=WARM):
    for fn in fns.values():
        window(fn, warm)
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def report(name, ts, nbytes):
    med = statistics.median(ts)
    say(f"  {name:48s} {med * 1e6:8.1f} us  ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})   {nbytes / med / 1e9:8.1f} GB/s of "
        f"{nbytes / 1e6:.1f} MB = {nbytes / med / HBM * 100:.1f} % of the HBM roof")
    return med


def versions(shape, g=7.5):
    import gad
    from gad import ops
    from gad.schedulers import PLMS_WEIGHTS, plms_coefficients
    sch = gad.sd_scheduler("pndm")
    gen = torch.Generator(device=dev).manual_seed(0)
    # x is overwritten with a contraction of itself every call (cs x with |cm m| small), so keep it bounded: cs = 1 here
    x = torch.randn(shape, device=dev, generator=gen)
    eps = torch.randn((2 * shape[0],) + tuple(shape[1:]), device=dev, generator=gen) * 1e-3
    n = x.numel()
    ring = torch.randn(3, n, device=dev, generator=gen) * 1e-3
    w = PLMS_WEIGHTS[4]
    _, cm = plms_coefficients(sch.alphas_cumprod[501].item(), sch.alphas_cumprod[491].item())
    cs = 1.0
    a_t = a_p = sch.alphas_cumprod[501].item()                    # DDIM with a_prev = a_t: x_prev = x, bounded as well

    def plms():
        ops.plms_step_raw(x, eps, cs, cm, w, history=[ring[0], ring[1], ring[2]], push=ring[2], guidance=g, out=x)

    xf = x.view(-1)

    def torch_path():
        eu, ec = eps.view(2, -1)
        e = eu + g * (ec - eu)
        m = w[0] * e + w[1] * ring[0] + w[2] * ring[1] + w[3] * ring[2]
        ring[2].copy_(e)
        xf.copy_(cs * xf - cm * m)

    def ddim():
        ops.cfg_ddim_step_raw(x, eps, g, a_t, a_p, 0.0, out=x)
    return {"plms": plms, "torch": torch_path, "ddim": ddim}, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pndm_ab.txt"))
    a = ap.parse_args()
    say("Guided PLMS step: gad_plms_step (one launch) against the same update in torch ops and against gad_cfg_ddim_step")
    say(f"device: {torch.cuda.get_device_name(0)}; {ITERS} calls per window after {WARM} warm-up, {ROUNDS} alternating rounds; median (min .. max)")
    for shape in ((16, 4, 64, 64), (64, 4, 32, 32)):
        fns, n = versions(shape)
        say(f"\n[{shape[0]}][{shape[1]}][{shape[2]}][{shape[3]}] latents, guidance 7.5, four-term step with push, in place")
        ts = alternate(fns)
        p = report("gad_plms_step (32 B / element)", ts["plms"], 32 * n)
        t = report("torch elementwise ops (same 32 B / element)", ts["torch"], 32 * n)
        d = report("gad_cfg_ddim_step (16 B / element)", ts["ddim"], 16 * n)
        say(f"  torch / plms = {t / p:.2f}x    plms / ddim = {p / d:.2f}x")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
