"""Host side of DPM-Solver++ for the MI355X build: the VP noise schedule of a discrete-time model and the time grid.

Only what the drop-in sampler's fixed configuration needs (reference ldm/models/diffusion/dpm_solver/dpm_solver.py, Lu et al.
2022): `NoiseScheduleVP('discrete')` -- log(alpha_t) piecewise linear in t between the N discrete steps t_n = (n + 1) / N --
and the 'time_uniform' grid.  Every scalar is a float32 torch op on the CPU in the reference's order, so the times fed to the
model and the per-step coefficients equal the reference's.  The tensor updates themselves are one HIP kernel per step
(lr_dpmpp_cfg_step)."""
import torch


class NoiseScheduleVP:
    def __init__(self, schedule='discrete', betas=None, alphas_cumprod=None, **kwargs):
        if schedule != 'discrete':
            raise NotImplementedError(f"NoiseScheduleVP: schedule {schedule!r} is not supported; only 'discrete' is")
        if betas is not None:
            log_alphas = 0.5 * torch.log(1 - betas.detach().float().cpu()).cumsum(dim=0)
        else:
            assert alphas_cumprod is not None
            log_alphas = 0.5 * torch.log(alphas_cumprod.detach().float().cpu())
        self.schedule = schedule
        self.total_N = len(log_alphas)
        self.T = 1.
        self.t_array = torch.linspace(0., 1., self.total_N + 1)[1:]      # t_n = (n + 1) / N, float32
        self.log_alpha_array = log_alphas

    def marginal_log_mean_coeff(self, t):
        """log(alpha_t): linear between the two keypoints around t (the outer two beyond the ends).  A t equal to a keypoint
        uses the interval that ends there."""
        t = t.reshape(-1)
        xp, yp = self.t_array, self.log_alpha_array
        j = (torch.searchsorted(xp, t, right=False) - 1).clamp(0, xp.shape[0] - 2)
        x0, x1, y0, y1 = xp[j], xp[j + 1], yp[j], yp[j + 1]
        return y0 + (t - x0) * (y1 - y0) / (x1 - x0)

    def marginal_alpha(self, t):
        return torch.exp(self.marginal_log_mean_coeff(t))

    def marginal_std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.marginal_log_mean_coeff(t)))

    def marginal_lambda(self, t):
        """half log-SNR: log(alpha_t) - log(sigma_t)."""
        lm = self.marginal_log_mean_coeff(t)
        return lm - 0.5 * torch.log(1. - torch.exp(2. * lm))

    def model_time(self, t):
        """continuous t in [1/N, 1] -> the discrete model's time label (1000 (t - 1/N))."""
        return (t - 1. / self.total_N) * 1000.


def time_uniform_steps(ns, steps, t_T=None, t_0=None):
    """steps + 1 times from t_T (default T) down to t_0 (default 1/N), uniform in t, float32 (linspace on the CPU)."""
    t_T = ns.T if t_T is None else t_T
    t_0 = 1. / ns.total_N if t_0 is None else t_0
    return torch.linspace(t_T, t_0, steps + 1)


def multistep_plan(ns, steps, order=2, lower_order_final=True):
    """Per-step host scalars of multistep DPM-Solver++ (data prediction, solver_type 'dpm_solver') on the time-uniform grid.

    Step k (1..steps) evaluates the model at t_{k-1} and moves x from t_{k-1} to t_k:
      m_{k-1} = (x - sigma_s e) / alpha_s                                         (s = t_{k-1})
      order 1: x_k = ratio x - c m_{k-1},                    c = alpha_t expm1(-h)
      order 2: x_k = ratio x - c m_{k-1} - (0.5 c) D,        c = alpha_t (exp(-h) - 1), D = (1 / r0) (m_{k-1} - m_{k-2})
    with h = lambda_t - lambda_s, r0 = (lambda_s - lambda_{t_{k-2}}) / h.  The first step is order 1; with lower_order_final the
    order drops to keep k + order <= steps + 1 when steps < 15.  Returns a dict of float32 arrays of length `steps`."""
    if order not in (1, 2):
        raise NotImplementedError(f"DPM-Solver++ order {order} is not supported; orders 1 and 2 are")
    ts = time_uniform_steps(ns, steps)
    keys = ("t", "t_model", "order", "sigma_s", "alpha_s", "ratio", "c", "c_half", "inv_r0")
    plan = {k: [] for k in keys}
    for k in range(1, steps + 1):
        s_, t_ = ts[k - 1:k], ts[k:k + 1]
        if k == 1:
            o = 1
        elif lower_order_final and steps < 15:
            o = min(order, steps + 1 - k)
        else:
            o = order
        sigma_s, alpha_s = ns.marginal_std(s_), ns.marginal_alpha(s_)
        lam_s, lam_t = ns.marginal_lambda(s_), ns.marginal_lambda(t_)
        h = lam_t - lam_s
        sigma_t = ns.marginal_std(t_)
        alpha_t = torch.exp(ns.marginal_log_mean_coeff(t_))
        ratio = sigma_t / sigma_s
        if o == 1:
            c = alpha_t * torch.expm1(-h)
            inv_r0 = torch.zeros(1)
        else:
            h_0 = lam_s - ns.marginal_lambda(ts[k - 2:k - 1])
            r0 = h_0 / h
            inv_r0 = 1. / r0
            c = alpha_t * (torch.exp(-h) - 1.)
        for name, v in (("t", s_), ("t_model", ns.model_time(s_)), ("sigma_s", sigma_s), ("alpha_s", alpha_s),
                        ("ratio", ratio), ("c", c), ("c_half", 0.5 * c), ("inv_r0", inv_r0)):
            plan[name].append(float(v.reshape(-1)[0]))
        plan["order"].append(o)
    out = {k: torch.tensor(v, dtype=torch.float32).numpy() for k, v in plan.items() if k != "order"}
    out["order"] = torch.tensor(plan["order"]).numpy()
    return out
