"""Shared by tests/test_seeded_noise_cpu.py and tests/test_gpu_seeded_noise.py: the five keys of the moment checks, the standardised
statistics, the two-rank sharding worker and the element-wise stub model of the sampler checks.  No tests here."""
import os

import numpy as np

from leftrefill_amd import noise as N

# (seed, sub, stream, step): (0, 0), (1, 0), (0, 1), another step, and a seed whose high word is set with a late step
KEYS = [(0, 0, N.STEP, 0), (1, 0, N.STEP, 0), (0, 1, N.STEP, 0), (0, 0, N.STEP, 7), (2 ** 40 + 7, 3, N.STEP, 49)]
N_MOMENTS = 2 ** 20
BAND = 4.0


def standardised(zs):
    """{name: statistic} for draws zs (a list of equally long float arrays, one per key): per key the mean, variance, skewness and
    kurtosis, each divided by its Gaussian standard error (sqrt(n) mean, sqrt(n / 2) (var - 1), sqrt(n / 6) skew, sqrt(n / 24) (kurt - 3))
    and sqrt(n) times the correlation at lags 1, 2 and 4; per pair of keys sqrt(n) times their correlation.  All ~ N(0, 1) under the
    hypothesis of independent standard normals."""
    zs = [np.asarray(z, dtype=np.float64) for z in zs]
    n = zs[0].size
    out = {}
    for k, z in enumerate(zs):
        m, v = z.mean(), z.var()
        d = z - m
        out[f"key{k}.mean"] = np.sqrt(n) * m
        out[f"key{k}.var"] = np.sqrt(n / 2) * (v - 1)
        out[f"key{k}.skew"] = np.sqrt(n / 6) * (d ** 3).mean() / v ** 1.5
        out[f"key{k}.kurt"] = np.sqrt(n / 24) * ((d ** 4).mean() / v ** 2 - 3)
        for lag in (1, 2, 4):
            out[f"key{k}.lag{lag}"] = np.sqrt(n) * np.corrcoef(z[:-lag], z[lag:])[0, 1]
    for i in range(len(zs)):
        for j in range(i + 1, len(zs)):
            out[f"key{i}.key{j}.corr"] = np.sqrt(n) * np.corrcoef(zs[i], zs[j])[0, 1]
    return out


def check_moments(zs, who):
    st = standardised(zs)
    worst = max(st, key=lambda k: abs(st[k]))
    print(f"[{who}] {len(st)} standardised statistics at n = {zs[0].size}: max |.| = {abs(st[worst]):.2f} ({worst}); "
          f"max |z| = {max(float(np.abs(z).max()) for z in zs):.2f}")
    bad = {k: round(float(v), 2) for k, v in st.items() if not abs(v) <= BAND}
    assert not bad, bad


# ---- sharding over a world-2 gloo group -----------------------------------------------------------------------------------------------
SHARD_B, SHARD_SHAPE = 5, (3, 7)      # ragged: 3 + 2 samples; 21 elements per sample (a tail of one)
SHARD_SEEDS = [11, 2 ** 40 + 7, 5, 11, 0]
SHARD_SUBS = [0, 3, 1, 1, 0]


def shard_sample_fn(cond, uncond, x_T, b, seeds):
    """A toy sampler: x_T plus two seeded draws of every sample's own key."""
    import torch
    sn = seeds if isinstance(seeds, N.SeededNoise) else N.SeededNoise(seeds)
    assert len(sn) == b == x_T.shape[0]
    return x_T + sn.normal(N.STEP, 3, x_T.shape[1:]) + 0.5 * sn.normal(N.START, 0, x_T.shape[1:]) + torch.zeros(())


def shard_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from leftrefill_amd import dist as lrd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x_T = torch.arange(SHARD_B * 21.).reshape((SHARD_B,) + SHARD_SHAPE)
    state = torch.get_rng_state()
    sn = N.SeededNoise(SHARD_SEEDS, SHARD_SUBS)
    outs = [lrd.sample_sharded(shard_sample_fn, None, None, x_T, SHARD_B, seeds=s)
            for s in (sn, sn.keys, [(SHARD_SEEDS[0])] * SHARD_B)]
    q.put((rank, [o.numpy().tobytes() for o in outs], bool(torch.equal(state, torch.get_rng_state()))))
    dist.destroy_process_group()


# ---- the stub model of the sampler checks ----------------------------------------------------------------------------------------------
LATENT = (4, 8, 16)


def keyed(seed, stream):
    """A per-sample tensor [4, 8, 16] that is a function of the sample's seed alone (conditioning, x0): the statement's own draw."""
    import torch
    return torch.from_numpy(N.normal_numpy(seed, 0, stream, 0, int(np.prod(LATENT)))).reshape(LATENT)


def stub_model(device):
    """A LatentDiffusion with the schedule buffers of the real linear schedule (betas, alphas_cumprod, the posterior tables,
    num_timesteps = 1000, parameterization 'eps', q_sample) and apply_model(x, t, c) = 0.5 x + c: purely element-wise, so no
    batch-dependent kernel plan can enter."""
    import torch

    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.models.diffusion.ddpm import LatentDiffusion

    class Stub(LatentDiffusion):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.v_posterior, self.clip_denoised, self.log_every_t = "eps", 0., False, 100
            self.channels, self.image_size = 4, 8
            self.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120)

        def apply_model(self, x, t, c, **kw):
            assert x.shape[0] == t.shape[0] == c.shape[0]
            return 0.5 * x + c

    return Stub().to(device).eval()
