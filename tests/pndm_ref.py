"""numpy fp64 restatement of diffusers-0.24 PNDMScheduler as Stable Diffusion runs it (skip_prk_steps=True, epsilon prediction,
leading spacing), with its own state: the list `ets` of noise predictions, `counter`, `cur_sample`.  diffusers is not installed, so
this file is the pinned truth for gad.PNDMScheduler and gad_plms_step.  The alphas_cumprod table is handed in (the fp32 table the
scheduler under test built, read as fp64), so that both sides step with the same constants."""
import numpy as np


def sd_alphas_cumprod(n=1000, beta_start=0.00085, beta_end=0.012):
    """the scaled_linear table as diffusers builds it: fp32 linspace of the square roots, squared, fp32 cumprod"""
    import torch
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).double().numpy()


def timesteps(n, num_train_timesteps=1000, steps_offset=1):
    r = num_train_timesteps // n
    ts = np.arange(n) * r + steps_offset
    return np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()


def transfer(a_t, a_p):
    """(cs, cm) of x_prev = cs x - cm m (PNDMScheduler._get_prev_sample, epsilon prediction)"""
    cs = np.sqrt(a_p / a_t)
    cm = (a_p - a_t) / (a_t * np.sqrt(1.0 - a_p) + np.sqrt(a_t * (1.0 - a_t) * a_p))
    return float(cs), float(cm)


class PNDMRef:
    def __init__(self, alphas_cumprod, num_train_timesteps=1000, steps_offset=1, set_alpha_to_one=False):
        self.ac = np.asarray(alphas_cumprod, dtype=np.float64)
        self.T, self.offset = num_train_timesteps, steps_offset
        self.final = 1.0 if set_alpha_to_one else float(self.ac[0])
        self.n = None

    def set_timesteps(self, n):
        self.n = n
        self.timesteps = timesteps(n, self.T, self.offset)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def step(self, e, t, x):
        """-> x_prev (fp64); `self.last` records what the step did: t_from, t_to, the weights on (e, stored predictions newest
        first), whether e was appended, whether the remembered sample was used / written, and (cs, cm)"""
        e, x = np.asarray(e, dtype=np.float64), np.asarray(x, dtype=np.float64)
        r = self.T // self.n
        t, prev = int(t), int(t) - r
        stored = list(self.ets[::-1])                      # before this step, newest first
        push = self.counter != 1
        if push:
            self.ets = self.ets[-3:]
            self.ets.append(e)
        else:
            prev, t = t, t + r
        save = use_saved = False
        if len(self.ets) == 1 and self.counter == 0:
            m, w = e, (1.0,)
            self.cur_sample, save = x, True
        elif len(self.ets) == 1 and self.counter == 1:
            m, w = (e + self.ets[-1]) / 2, (0.5, 0.5)
            x, self.cur_sample, use_saved = self.cur_sample, None, True
        elif len(self.ets) == 2:
            m, w = (3 * self.ets[-1] - self.ets[-2]) / 2, (3 / 2, -1 / 2)
        elif len(self.ets) == 3:
            m, w = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12, (23 / 12, -16 / 12, 5 / 12)
        else:
            m, w = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24, (55 / 24, -59 / 24, 37 / 24, -9 / 24)
        a_t = self.ac[t]
        a_p = self.ac[prev] if prev >= 0 else self.final
        cs, cm = transfer(a_t, a_p)
        self.last = dict(t_from=t, t_to=prev, weights=tuple(w) + (0.0,) * (4 - len(w)), push=push, use_saved=use_saved, save=save,
                         cs=cs, cm=cm, xs=x, m=m, history=stored[:len(w) - 1], final=prev < 0)
        self.counter += 1
        return cs * x - cm * m
