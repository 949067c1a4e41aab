"""CPU: seeded sampling noise -- the host statement (leftrefill_amd/noise.py: the pinned vector, the explicit formula, structure,
moments), the CPU route of SeededNoise, the new C-ABI symbol, the samplers' `seeds=` keyword where it needs no device, and
dist.sample_sharded over a world-2 gloo group."""
import math
import os
import socket

import numpy as np
import pytest
import torch

import seeded_noise_helpers as H
from leftrefill_amd import noise as N
from leftrefill_amd.lora_dropout import philox4x32_10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- pin ---------------------------------------------------------------------------------------------------------------------------------
def test_pinned_vector(golden):
    g = golden("seeded_noise")
    n = int(g["n"])
    assert len(g["keys"]) == 2 and n % 4 != 0
    for k, (seed, sub, stream, step) in enumerate([int(v) for v in row] for row in g["keys"]):
        z = N.normal_numpy(seed, sub, stream, step, n)
        assert z.dtype == np.float32 and np.array_equal(_bits(z), _bits(g[f"key{k}.z32"])), k
        z64, r64 = N.normal_parts(seed, sub, stream, step, n)
        assert np.array_equal(z64, g[f"key{k}.z64"]) and np.array_equal(r64, g[f"key{k}.r64"])
        assert [int(w) for w in philox4x32_10((0, sub, step, stream), (seed & 0xFFFFFFFF, seed >> 32))] == [int(w) for w in g[f"key{k}.words0"]]


def test_the_statement_element_by_element():
    """Every element from scalar arithmetic: the counter (g, sub, step, stream), the key (seed lo, seed hi), the 23-bit uniforms, the pairing."""
    seed, sub, stream, step = 2 ** 40 + 7, 3, N.KNOWN, 49
    z = N.normal_numpy(seed, sub, stream, step, 11)
    for i in range(11):
        w = [int(v) for v in philox4x32_10((i >> 2, sub, step, stream), (seed & 0xFFFFFFFF, seed >> 32))]
        p = (i & 3) >> 1
        u1, u2 = ((w[2 * p] >> 9) + 0.5) * 2.0 ** -23, ((w[2 * p + 1] >> 9) + 0.5) * 2.0 ** -23
        assert 0.0 < u1 < 1.0 and np.float32(u1) == u1 and np.float32(2 * u2) == 2 * u2      # exact in fp32
        r = math.sqrt(-2.0 * math.log(u1))
        want = r * (math.sin(2 * math.pi * u2) if i & 1 else math.cos(2 * math.pi * u2))
        assert abs(float(z[i]) - want) <= 2.0 ** -24 * max(r, 1.0), i      # one rounding to fp32
    assert (N.START, N.STEP, N.KNOWN, N.ENCODE, N.POSTERIOR) == (0, 1, 2, 3, 4) and len(set(N.STREAMS.values())) == 5


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
def test_element_i_does_not_depend_on_n():
    full = N.normal_numpy(5, 1, N.STEP, 2, 1023)
    for n in (1, 3, 4, 5, 512, 1022):
        assert np.array_equal(_bits(N.normal_numpy(5, 1, N.STEP, 2, n)), _bits(full[:n])), n
    for first, n in ((1, 9), (5, 4), (1019, 4), (6, 1)):      # a window of the sample: the same elements
        assert np.array_equal(_bits(N.normal_numpy(5, 1, N.STEP, 2, n, first=first)), _bits(full[first:first + n])), (first, n)
    assert N.normal_numpy(5, 1, N.STEP, 2, 3, first=2 ** 34 - 3).shape == (3,)      # the last elements a sample can have
    with pytest.raises(ValueError, match="elements per sample"):
        N.normal_numpy(5, 1, N.STEP, 2, 4, first=2 ** 34 - 3)


def test_every_part_of_the_name_matters():
    base = dict(seed=7, sub=0, stream=N.STEP, step=0)
    z0 = N.normal_numpy(n=256, **base)
    others = [dict(base, seed=8), dict(base, sub=1), dict(base, stream=N.KNOWN), dict(base, step=1), dict(base, seed=2 ** 40 + 7),
              dict(base, seed=7 + 2 ** 32)]
    for o in others:
        z = N.normal_numpy(n=256, **o)
        assert not (z.reshape(-1, 4) == z0.reshape(-1, 4)).all(axis=1).any(), o      # every group of four differs
    assert np.array_equal(N.normal_numpy(7 - 2 ** 64, 0, N.STEP, 0, 256), z0)      # a seed is its low 64 bits
    for bad in (dict(base, sub=2 ** 32), dict(base, step=-1), dict(base, stream=2 ** 32)):
        with pytest.raises(ValueError, match="uint32"):
            N.normal_numpy(n=4, **bad)
    with pytest.raises(ValueError, match="elements per sample"):
        N.normal_numpy(n=0, **base)


# ---- moments -----------------------------------------------------------------------------------------------------------------------------
def test_moments_of_the_statement():
    """Mean, variance, skewness, kurtosis, the lag-1/2/4 and the cross-key correlations of 2^20 values of the five keys, each standardised
    by its Gaussian standard error, lie within +-4.  (At n = 2^20 this would miss a bias below about 4e-3.)"""
    H.check_moments([N.normal_numpy(s, u, st, k, H.N_MOMENTS) for s, u, st, k in H.KEYS], "statement")


# ---- CPU route of SeededNoise -----------------------------------------------------------------------------------------------------------
def test_cpu_route_rows_are_their_own_keys():
    state, np_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    sn = N.SeededNoise([3, 2 ** 40 + 7, 9], subs=[0, 3, 1])
    assert len(sn) == 3 and sn.device.type == "cpu" and sn.keys.dtype == torch.int64 and tuple(sn.keys.shape) == (3, 2)
    z = sn.normal(N.STEP, 5, (3, 7))
    assert z.shape == (3, 3, 7) and z.dtype == torch.float32
    for b, (seed, sub) in enumerate([(3, 0), (2 ** 40 + 7, 3), (9, 1)]):
        one = N.SeededNoise([seed], subs=[sub]).normal(N.STEP, 5, (3, 7))
        assert torch.equal(one[0], z[b])
        assert np.array_equal(_bits(z[b].numpy().reshape(-1)), _bits(N.normal_numpy(seed, sub, N.STEP, 5, 21)))
    assert torch.equal(sn.shard(1, 3).normal(N.STEP, 5, (3, 7)), z[1:]) and len(sn.shard(1, 3)) == 2
    assert torch.equal(sn.row0().normal(N.STEP, 5, (3, 7)), z[:1].expand(3, 3, 7))
    out = torch.full((3, 21), 7.0)
    assert sn.normal(N.STEP, 5, (21,), out=out) is out and torch.equal(out, z.reshape(3, 21))
    # the table as tensors: [B] with subs, [B, 2]; a seed above 2^63 travels as its int64 bits
    big = 2 ** 64 - 5
    t = N.SeededNoise(torch.tensor([3, 2 ** 40 + 7, 9]), subs=[0, 3, 1])
    assert torch.equal(t.keys, sn.keys) and torch.equal(N.SeededNoise(sn.keys).normal(N.STEP, 5, (3, 7)), z)
    assert N.SeededNoise([big]).keys.tolist() == [[-5, 0]] and N.SeededNoise(torch.tensor([[-5, 0]])).host_keys() == [(big, 0)]
    assert np.array_equal(_bits(N.SeededNoise([big]).normal(N.START, 0, (8,)).numpy()[0]), _bits(N.normal_numpy(big, 0, N.START, 0, 8)))
    assert torch.equal(state, torch.get_rng_state()) and np.array_equal(np_state, np.random.get_state()[1])
    with pytest.raises(ValueError, match="2 keys for a batch of 3"):
        N.as_seeded([1, 2], 3, "cpu")
    assert N.as_seeded(None, 3, "cpu") is None and N.as_seeded(sn, 3, "cpu") is sn


# ---- binding -----------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_bound_without_a_twin():
    import abi_helpers as abi
    from leftrefill_amd import _lib
    assert "lr_seeded_normal" in _lib.SIGNATURES and "lr_seeded_normal" not in _lib.BF16_TWINS and "lr_seeded_normal_bf16" not in _lib.SIGNATURES
    assert abi.c_params("lr_seeded_normal") == ["const int64_t* keys", "int B", "int64_t per_sample", "int32_t stream", "int32_t step",
                                                "float* out", "lr_stream_t s"]
    assert _lib.ABI_VERSION == 30      # additive: the version does not move


# ---- the drop-in surface that needs no device ------------------------------------------------------------------------------------------
def test_posterior_sample_takes_a_ready_noise():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    params = torch.arange(2 * 8 * 2 * 3, dtype=torch.float32).reshape(2, 8, 2, 3) / 50 - 1
    post = DiagonalGaussianDistribution(params)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    noise = N.SeededNoise([3, 5]).normal(N.POSTERIOR, 0, (4, 2, 3))
    z = post.sample(noise=noise)
    assert torch.equal(z, post.mean + post.std * noise) and torch.equal(state, torch.get_rng_state())
    # the default draw is the reference's: generators re-seeded to 42, host randn
    torch.manual_seed(42)
    ref = post.mean + post.std * torch.randn(post.mean.shape)
    torch.manual_seed(5)
    assert torch.equal(post.sample(), ref)


def test_multi_sampling_refuses_seeds():
    stub = H.stub_model("cpu")
    from ldm.models.diffusion.ddim import DDIMSampler
    with pytest.raises(NotImplementedError, match="seeds with list conditioning"):
        DDIMSampler(stub).sample(4, 1, H.LATENT, conditioning=[H.keyed(1, 100)[None]], verbose=False, seeds=[1])


# ---- sharding over gloo world-2 ----------------------------------------------------------------------------------------------------------
def test_sample_sharded_with_seeds_gloo_world2():
    """dist.sample_sharded hands every rank the keys of its own rows: the gathered result of a toy sampler that adds seeded draws equals
    the single-process result bit for bit, for a SeededNoise, a [B, 2] tensor and a list of ints; no generator moves."""
    import torch.multiprocessing as mp
    from leftrefill_amd import dist as lrd
    x_T = torch.arange(H.SHARD_B * 21.).reshape((H.SHARD_B,) + H.SHARD_SHAPE)
    sn = N.SeededNoise(H.SHARD_SEEDS, H.SHARD_SUBS)
    forms = (sn, sn.keys, [H.SHARD_SEEDS[0]] * H.SHARD_B)
    full = [H.shard_sample_fn(None, None, x_T, H.SHARD_B, s).numpy().tobytes() for s in forms]
    assert full[0] == full[1] != full[2]
    # no process group: the fifth argument is passed through; four-argument callers are called with four
    assert lrd.sample_sharded(H.shard_sample_fn, None, None, x_T, H.SHARD_B, seeds=sn).numpy().tobytes() == full[0]
    assert lrd.sample_sharded(lambda c, uc, xt, b: xt * 2, None, None, x_T, H.SHARD_B).equal(x_T * 2)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=H.shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
    for rank, outs, rng_untouched in res:
        assert outs == full and rng_untouched, rank
