"""Coupling plan x_t = alpha_t x1 + sigma_t x0 (reference: LDMAE/transport/path.py).

Only the linear (rectified-flow) plan of the shipped configuration is implemented (configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml:
path_type Linear, prediction velocity); the reference's VP / GVP plans and the score / noise parametrisations are outside the hot-path scope
 and raise in ``create_transport``.  The SDE sampler's diffusion coefficient and the velocity-to-score conversion of this plan
are host functions of one time (``diffusion``, ``score_from_velocity``): the sampler turns them into the coefficients of its step kernel."""
import torch as th


def expand_t_like_x(t, x):
    """[B] -> [B, 1, 1, ...] (path.py:5-13)."""
    return t.view(t.size(0), *([1] * (x.dim() - 1)))


class ICPlan:
    """Linear path: alpha = t, sigma = 1 - t (path.py:18-136)."""

    def __init__(self, sigma=0.0):
        self.sigma = sigma

    def compute_alpha_t(self, t):
        return t, 1

    def compute_sigma_t(self, t):
        return 1 - t, -1

    def compute_mu_t(self, t, x0, x1):
        t = expand_t_like_x(t, x1)
        return self.compute_alpha_t(t)[0] * x1 + self.compute_sigma_t(t)[0] * x0

    def compute_xt(self, t, x0, x1):
        return self.compute_mu_t(t, x0, x1)

    def compute_ut(self, t, x0, x1, xt):
        t = expand_t_like_x(t, x1)
        return self.compute_alpha_t(t)[1] * x1 + self.compute_sigma_t(t)[1] * x0

    def plan(self, t, x0, x1):
        xt = self.compute_xt(t, x0, x1)
        return t, xt, self.compute_ut(t, x0, x1, xt)


DIFFUSION_FORMS = ("constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")     # the reference's keys (path.py:54-61), its spelling


def diffusion(t, form="constant", norm=1.0):
    """w(t) of ICPlan.compute_diffusion (path.py:45-68) at one time, on the host in f64.  SBDM is (1-t)^2 / t + (1-t): infinite at t = 0."""
    import math
    t, norm = float(t), float(norm)
    if form == "constant":
        return norm
    if form == "SBDM":
        return norm * ((1 - t) ** 2 / t + (1 - t)) if t != 0 else math.inf
    if form in ("sigma", "linear"):
        return norm * (1 - t)
    if form == "decreasing":
        return 0.25 * (norm * math.cos(math.pi * t) + 1) ** 2
    if form == "inccreasing-decreasing":
        return norm * math.sin(math.pi * t) ** 2
    raise NotImplementedError(f"Diffusion form {form} not implemented (one of {', '.join(DIFFUSION_FORMS)})")


def score_from_velocity(t):
    """ICPlan.get_score_from_velocity (path.py:70-84) as the pair (a, b) of score = a v + b x: a = t / var, b = -1 / var with
    var(t) = (1-t)^2 + t (1-t).  Host f64; singular at t = 1."""
    t = float(t)
    var = (1 - t) ** 2 + t * (1 - t)
    if var == 0:
        raise ValueError(f"the score of the linear path is singular at t = {t} (var = 0)")
    return t / var, -1 / var
