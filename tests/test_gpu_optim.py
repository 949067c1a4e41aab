"""lr_amp_adamw_step on the GPU against tests/golden/optim.npz: torch's AdamW + GradScaler("cpu") + CosineAnnealingLR on recorded
gradients, with an overflow at step 2 and growth interval 3 (tools/make_golden_optim.py).

Bound on parameters and moments (per tensor, per step): the yardstick is the max-abs distance of torch's own fp32 CPU trajectory from
the float64 one; the kernel may be at most 2 x that plus one fp32 ulp of max|value|.  The factor 2 covers a different but equally long
chain of fp32 roundings.  With LEFTREFILL_PROFILE_DIR set, the measured distances and yardsticks are written to optim_parity.json there
(the committed record is profiles/optim_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("param", "exp_avg", "exp_avg_sq")


def _gold():
    g = np.load(os.path.join(GOLDEN, "optim.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def _optimizer(gold, meta, grad_dtype=torch.float32, shapes=None):
    from leftrefill_amd.optim import AmpAdamW, cosine_schedule
    n = len(meta["shapes"])
    ps = [torch.nn.Parameter(torch.from_numpy(gold["p0.%d" % i]).clone().to(DEV)) for i in range(n)]
    groups = [dict(params=[p for p, gi in zip(ps, meta["group_of"]) if gi == k], **meta["groups"][k]) for k in range(len(meta["groups"]))]
    opt = AmpAdamW(groups, lr=meta["groups"][0]["lr"], growth_interval=meta["growth_interval"])
    opt.set_schedule(cosine_schedule(opt, meta["max_steps"], meta["eta_min"] * meta["groups"][0]["lr"]))
    bufs = [torch.zeros(p.shape, dtype=grad_dtype, device=DEV) for p in ps]
    opt.bind_grads(dict(zip(ps, bufs)))
    return opt, ps, bufs


def _feed(gold, k, bufs, cast=None):
    for i, b in enumerate(bufs):
        g = torch.from_numpy(gold["grad.%d.%d" % (k, i)])
        if cast is not None:
            g = g.to(cast)
        b.copy_(g.to(b.dtype))


def _snapshot(opt, ps):
    return [[p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()] if "exp_avg" in opt.state[p]
            else [p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)] for p in ps]


def _run(gold, meta, grad_dtype=torch.float32, cast=None):
    opt, ps, bufs = _optimizer(gold, meta, grad_dtype)
    states, snaps = [], []
    for k in range(meta["steps"]):
        _feed(gold, k, bufs, cast)
        opt.step()
        states.append(opt.amp_state())
        snaps.append(_snapshot(opt, ps))
    return opt, states, snaps


def test_kernel_follows_torch_step_by_step():
    gold, meta = _gold()
    opt, ps, bufs = _optimizer(gold, meta)
    report = {"bound": "2 * max|torch fp32 - float64| + ulp32(max|float64|), per tensor and step", "steps": []}
    worst = 0.0
    for k in range(meta["steps"]):
        before = _snapshot(opt, ps) if k else None
        _feed(gold, k, bufs)
        opt.step()
        s = opt.amp_state()
        # integers and powers of two: exactly equal
        assert s["scale"] == float(gold["scale"][k]), (k, s)
        for name in ("growth_tracker", "found_inf", "applied_steps", "sched_steps", "skipped", "lr_index"):
            assert s[name] == int(gold[name][k]), (k, name, s)
        assert s["lr"] == [float(np.float32(v)) for v in gold["lr"][k]], (k, s["lr"])
        assert [g["lr"] for g in opt.param_groups] == list(gold["schedule"][k + 1])      # host mirror: the next step's rate
        after = _snapshot(opt, ps)
        if s["found_inf"]:
            assert k == meta["overflow_at"]
            for a, b in zip(before, after):
                for x, y in zip(a, b):
                    assert torch.equal(x, y), "a skipped step must leave parameters and moments bit-unchanged"
        row = {"step": k, "found_inf": s["found_inf"], "scale": s["scale"], "grad_norm": s["grad_norm"], "tensors": []}
        for i in range(len(ps)):
            for j, kind in enumerate(KINDS):
                f64 = gold["f64.%s.%d.%d" % (kind, k, i)]
                f32 = gold["f32.%s.%d.%d" % (kind, k, i)].astype(np.float64)
                got = after[i][j].cpu().numpy().astype(np.float64)
                yard = float(np.abs(f32 - f64).max())
                dist = float(np.abs(got - f64).max())
                bound = 2.0 * yard + float(np.spacing(np.float32(np.abs(f64).max())))
                row["tensors"].append({"tensor": i, "kind": kind, "kernel_vs_f64": dist, "torch_fp32_vs_f64": yard, "bound": bound,
                                       "bit_equal_to_torch_fp32": bool(np.array_equal(got, f32))})
                print(f"step {k} tensor {i} {kind}: kernel {dist:.3e} torch-fp32 {yard:.3e} bound {bound:.3e}")
                worst = max(worst, dist / bound)
        report["steps"].append(row)
        if not s["found_inf"]:      # the norm of the unscaled gradients, against float64 of the recorded ones
            scale_used = 65536.0 if k == 0 else float(gold["scale"][k - 1])
            ref = np.sqrt(sum(float((gold["grad.%d.%d" % (k, i)].astype(np.float64) ** 2).sum()) for i in range(len(ps)))) / scale_used
            assert abs(s["grad_norm"] - ref) <= 1e-6 * ref, (k, s["grad_norm"], ref)
    report["worst_fraction_of_bound"] = worst
    out = os.environ.get("LEFTREFILL_PROFILE_DIR")      # set it to (re)write the committed record profiles/optim_parity.json
    if out:
        with open(os.path.join(out, "optim_parity.json"), "w") as f:
            json.dump(report, f, indent=1)
    for row in report["steps"]:
        for t in row["tensors"]:
            assert t["kernel_vs_f64"] <= t["bound"], (row["step"], t)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_16_bit_gradient_kinds_equal_the_run_on_upcast_gradients(dtype):
    """The kernel up-casts a 16-bit gradient itself: the same bits as feeding the up-cast values as fp32 (the overflow survives the cast)."""
    gold, meta = _gold()
    _, s16, p16 = _run(gold, meta, dtype)
    _, s32, p32 = _run(gold, meta, torch.float32, cast=dtype)
    assert s16 == s32
    assert [s["found_inf"] for s in s16] == [int(v) for v in gold["found_inf"]]
    for a, b in zip(p16, p32):
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                assert torch.equal(u, v)


@pytest.mark.parametrize("n_tensors", [1, 35])
def test_three_launches_whatever_the_tensor_count(n_tensors):
    from leftrefill_amd import ops
    from leftrefill_amd.optim import AmpAdamW
    g = torch.Generator(device=DEV).manual_seed(n_tensors)
    ps = [torch.nn.Parameter(torch.randn(73 * 1024 if i == 0 else 1000 + 37 * i, device=DEV, generator=g)) for i in range(n_tensors)]
    opt = AmpAdamW(ps, lr=1e-4)
    for p in ps:
        p.grad = torch.randn_like(p) * 65536.0
    before = [p.detach().clone() for p in ps]
    n0 = ops.OPT_LAUNCHES.value
    opt.step()
    assert 0 < ops.OPT_LAUNCHES.value - n0 <= 3
    n0 = ops.OPT_LAUNCHES.value
    opt.step()
    opt.step()
    assert ops.OPT_LAUNCHES.value - n0 <= 6
    assert opt.amp_state()["applied_steps"] == 3 and all(not torch.equal(a, p) for a, p in zip(before, ps))
    # against torch on the device: same gradients, three steps
    ref = [torch.nn.Parameter(b.clone()) for b in before]
    topt = torch.optim.AdamW(ref, lr=1e-4)
    for _ in range(3):
        for r, p in zip(ref, ps):
            r.grad = p.grad / 65536.0
        topt.step()
    for r, p in zip(ref, ps):      # each trajectory rounds the parameter once per step (half an ulp); the update terms agree far below that
        assert (r - p).abs().max().item() <= 3 * 2.0 ** -23 * max(1.0, p.abs().max().item())


def test_two_runs_are_bit_identical():
    gold, meta = _gold()
    _, s1, p1 = _run(gold, meta)
    _, s2, p2 = _run(gold, meta)
    assert s1 == s2
    for a, b in zip(p1, p2):
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                assert torch.equal(u, v)


def test_captured_replay_is_bit_identical_to_eager():
    gold, meta = _gold()
    _, s_eager, p_eager = _run(gold, meta)
    opt, ps, bufs = _optimizer(gold, meta)
    _feed(gold, 0, bufs)
    p_init, snap = [p.detach().clone() for p in ps], None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                      # builds the descriptor table and the moments outside of the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fresh, _, _ = _optimizer(gold, meta)
    snap = (fresh._state.clone(), 0, {})
    with torch.no_grad():
        for p, q in zip(ps, p_init):
            p.copy_(q)
    opt.restore(snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    with torch.no_grad():               # capture does not execute, but start from a known state all the same
        for p, q in zip(ps, p_init):
            p.copy_(q)
    opt.restore(snap)
    for k in range(meta["steps"]):
        _feed(gold, k, bufs)
        graph.replay()
        opt.advance_host()
        torch.cuda.synchronize()
        assert opt.amp_state() == s_eager[k], k
        for a, b in zip(_snapshot(opt, ps), p_eager[k]):
            for u, v in zip(a, b):
                assert torch.equal(u, v), k
    assert [s["found_inf"] for s in s_eager] == [int(v) for v in gold["found_inf"]]


def test_scale_one_mode_has_no_scaler_dynamics():
    from leftrefill_amd.optim import AmpAdamW
    p = torch.nn.Parameter(torch.ones(1000, device=DEV))
    opt = AmpAdamW([p], lr=1e-3, init_scale=1.0, growth_interval=0)
    for k in range(4):
        p.grad = torch.full_like(p, float("nan") if k == 1 else 0.5)
        opt.step()
    s = opt.amp_state()
    assert (s["scale"], s["growth_tracker"], s["applied_steps"], s["sched_steps"], s["skipped"]) == (1.0, 0, 3, 4, 1)
    assert torch.isfinite(p).all() and (p < 1).all()
