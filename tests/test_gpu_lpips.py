"""lr_lpips_alex (csrc/lpips.hip) on the MI355X against `evalglue.LPIPSAlex` in float64 on the CPU, on the same stored inputs and the
seeded weights of tests/test_lpips_cpu.py (which also holds the families, the yardstick and the fp16-storage emulation); its exact
cases, determinism, batch independence, graph capture, argument errors, and the glue: `DeviceLPIPS.forward`, `validation_result`,
`tools/run_inpainting.py --device_lpips`.

Tolerance of the parity cases: the FLOOR of an image family is the largest |fp16-storage emulation - float64| over the family's six
cases; the kernel gets 4 x that floor (its fp32 summation order differs from the emulation's), capped at 5e-5 absolute -- half a unit
of the four decimals the harness prints.  Floors measured on the CPU (tests/test_lpips_cpu.py prints them; the harness case adds
none larger on the shapes tried):
    family   LPIPS      floor     tolerance
    far      ~0.03      1.5e-6    6.0e-6
    near     ~1.4e-3    1.5e-7    5.8e-7
    vnear    ~1.5e-5    5.0e-8    2.0e-7
The kernel's own maxima are written to profiles/lpips_parity.json by a run with LEFTREFILL_WRITE_PROFILES set; that file is not in
the tree yet: no MI355X run of this module has been recorded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_lpips_cpu as L  # noqa: E402
from test_gpu_eval_metrics import _write_config  # noqa: E402  (the tiny model of tests/test_gpu_harness.py)
from oracle import golden_spec as G, weights  # noqa: E402

ROOT = L.ROOT
DEV = "cuda"
_SEEN = {}      # family -> rows of the parity cases that have run, for the summary / profile


@pytest.fixture(scope="module")
def device_module():
    from leftrefill_amd.evalglue import DeviceLPIPS
    return DeviceLPIPS().load_weights(L.seeded_state_dict()).to(DEV)


def _d(t):
    return None if t is None else t.to(DEV)


def _kernel(module, pred, origin, mask, x0, Wc, r):
    from leftrefill_amd import ops
    return ops.lpips_alex(_d(pred), _d(origin), _d(mask), x0, Wc, r, module.packed())


@pytest.mark.parametrize("case", range(len(L.CASES)), ids=[c[0] for c in L.CASES])
@pytest.mark.parametrize("fam", list(L.FAMILIES))
def test_kernel_against_float64_lpipsalex(fam, case, device_module):
    """Every case for every family; prints each figure before it asserts and merges the family's floor / maximum into
    profiles/lpips_parity.json when LEFTREFILL_WRITE_PROFILES is set."""
    rows, floor = L.family_references(fam)      # yardstick and emulation of the family's six cases: computed once, shared
    ref = rows[case]
    tol = min(4 * floor, L.CAP)
    got = _kernel(device_module, *ref["inputs"]).cpu().double()
    err = float((got - ref["ref"]).abs().max())
    row = dict(case=ref["case"][0], lpips=float(ref["ref"].mean()), floor=ref["floor"], kernel_err=err,
               kernel_vs_emulation=float((got - ref["emu"]).abs().max()))
    print(fam, json.dumps(row), "family floor", floor, "tolerance", tol)
    _SEEN.setdefault(fam, {})[row["case"]] = row
    if os.environ.get("LEFTREFILL_WRITE_PROFILES"):
        path = os.path.join(os.environ["LEFTREFILL_WRITE_PROFILES"], "lpips_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        seen = list(_SEEN[fam].values())
        doc[fam] = dict(floor=floor, tolerance=tol, kernel_max=max(r_["kernel_err"] for r_ in seen), cases=seen)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
    assert torch.isfinite(got).all()
    assert err <= tol, (err, tol)


def test_exact_zero_cases(device_module):
    """pred == origin with no mask, and a mask of all zeros (the composite equals the origin): exactly 0.0."""
    pred, origin = L.family("far", 2, 67, 95, seed=5)
    out = _kernel(device_module, origin, origin, None, 0, 95, 1)
    assert torch.equal(out.cpu(), torch.zeros(2))
    out = _kernel(device_module, pred, origin, torch.zeros(2, 1, 67, 95), 0, 95, 1)
    assert torch.equal(out.cpu(), torch.zeros(2))
    out = _kernel(device_module, pred[:, :, :66].half(), origin[:, :, :66], torch.zeros(2, 1, 66, 95), 31, 64, 2)
    assert torch.equal(out.cpu(), torch.zeros(2))
    assert (_kernel(device_module, pred, origin, None, 0, 95, 1) > 0).all()


def test_determinism_batch_independence_and_graph_capture(device_module):
    """Two calls give identical bits; sample i alone has the bits it has in a batch of 3; a captured call replayed on new contents of the
    static inputs equals the eager call bit for bit."""
    from leftrefill_amd import ops
    packed = device_module.packed()
    pred, origin = L.family("near", 3, 67, 95, seed=7)
    mask = L.block_mask(3, 67, 95, seed=7)
    p, o, m = _d(pred.half()), _d(origin), _d(mask)
    a = ops.lpips_alex(p, o, m, 0, 95, 1, packed)
    b = ops.lpips_alex(p, o, m, 0, 95, 1, packed)
    assert torch.equal(a, b) and (a > 0).all()
    for i in range(3):
        alone = ops.lpips_alex(p[i:i + 1], o[i:i + 1], m[i:i + 1], 0, 95, 1, packed)
        assert torch.equal(alone, a[i:i + 1]), i
    torch.cuda.synchronize()
    sp, so, sm = p.clone(), o.clone(), m.clone()      # the static inputs of the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.lpips_alex(sp, so, sm, 0, 95, 1, packed)      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.lpips_alex(sp, so, sm, 0, 95, 1, packed)
    pred2, origin2 = L.family("far", 3, 67, 95, seed=8)
    mask2 = L.block_mask(3, 67, 95, seed=8)
    sp.copy_(pred2.half())
    so.copy_(origin2)
    sm.copy_(mask2)
    c.zero_()
    g.replay()
    torch.cuda.synchronize()
    eager = ops.lpips_alex(sp, so, sm, 0, 95, 1, packed)
    assert torch.equal(c, eager) and not torch.equal(c, a)


def test_argument_errors_are_raised_before_any_launch(device_module):
    """LR_E_ARG: r that does not divide a side, a scored side below 31 pixels, a workspace that is too small.  Nothing is launched:
    the output keeps its sentinel."""
    import ctypes
    from leftrefill_amd import _lib, ops
    packed = device_module.packed()
    pred, origin = L.family("far", 1, 64, 64, seed=1)
    p, o = _d(pred), _d(origin)
    sentinel = torch.full((1,), -7.0, device=DEV)
    for args in ((p[:, :, :63], o[:, :, :63], 0, 64, 2), (p, o, 0, 63, 2), (p[:, :, :30], o[:, :, :30], 0, 64, 1), (p, o, 0, 30, 1),
                 (p[:, :, :60], o[:, :, :60], 0, 60, 2)):
        with pytest.raises(RuntimeError, match="bad argument"):
            ops.lpips_alex(args[0], args[1], None, args[2], args[3], args[4], packed, out=sentinel)
    lib = _lib.load()
    need = lib.lr_lpips_workspace_bytes(1, 64, 64, 1)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    a = _lib.LpipsArgs()
    a.pred, a.pred_kind, a.origin, a.mask = p.data_ptr(), 0, o.data_ptr(), 0
    a.N, a.H, a.W, a.x0, a.Wc, a.r = 1, 64, 64, 0, 64, 1
    for k in range(5):
        a.wt[k], a.bias[k], a.lin[k] = packed["wt"][k].data_ptr(), packed["bias"][k].data_ptr(), packed["lin"][k].data_ptr()
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), need - 1, sentinel.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.lr_lpips_alex(ctypes.byref(a), st) == -1      # LR_E_ARG
    a.workspace_bytes, a.x0 = need, 1                        # columns [1, 65) leave the canvas
    assert lib.lr_lpips_alex(ctypes.byref(a), st) == -1
    torch.cuda.synchronize()
    assert float(sentinel) == -7.0
    a.x0 = 0
    assert lib.lr_lpips_alex(ctypes.byref(a), st) == 0       # and the same struct, put right, runs
    torch.cuda.synchronize()
    assert float(sentinel) > 0


def _host_per_sample(sd, pred, origin):
    """The per-sample host route on the same tensors: LPIPSAlex (fp32, on the GPU) one sample at a time."""
    from leftrefill_amd.evalglue import LPIPSAlex
    host = LPIPSAlex().load_weights(sd).to(DEV)
    return torch.tensor([float(host(pred[i:i + 1], origin[i:i + 1])) for i in range(pred.shape[0])], dtype=torch.float64)


def test_forward_is_a_drop_in_loss_fn_alex(device_module):
    """DeviceLPIPS.forward(a, b) on two plain images against LPIPSAlex.forward: [N,1,1,1], within the tolerance of the parity cases."""
    rows, floor = L.family_references("far")
    tol = min(4 * floor, L.CAP)
    a, b = L.family("far", 3, 67, 95, seed=11)
    got = device_module(_d(a), _d(b))
    assert got.shape == (3, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
    want = _host_per_sample(L.seeded_state_dict(), _d(a), _d(b))
    err = float((got.flatten().cpu().double() - want).abs().max())
    print("forward", got.flatten().tolist(), want.tolist(), err, tol)
    assert err <= tol


def test_validation_result_with_device_lpips_uses_one_read_back(device_module, monkeypatch):
    """validation_result with a DeviceLPIPS: returns 'lpips', logs 'val/lpips', and reads the three means back in ONE copy."""
    from leftrefill_amd import evalglue
    rows, floor = L.family_references("far")
    tol = min(4 * floor, L.CAP)
    pred, origin = L.family("far", 2, 64, 128, seed=13)
    mask = L.block_mask(2, 64, 128, seed=13)
    log = {"pred": _d(pred.half()), "origin_image": _d(origin)}
    mask_nhwc = _d(mask.permute(0, 2, 3, 1).contiguous())
    metrics = evalglue.device_metrics(log, mask_nhwc, right_half=True)
    logged = {}

    class M:
        loss_fn_alex = device_module

        def log(self, k, v, sync_dist=False):
            logged[k] = v

    def host_pair():
        raise AssertionError("the host composite must not be built for a DeviceLPIPS")

    torch.cuda.synchronize()
    copies = []
    real_tolist, real_item = torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (copies.append("tolist"), real_tolist(t))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda t: (copies.append("item"), real_item(t))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (_ for _ in ()).throw(AssertionError("a second read-back")))
    res = evalglue.validation_result(M(), metrics, host_pair, lambda fn: fn.score(log, mask_nhwc, right_half=True))
    monkeypatch.undo()
    assert copies == ["tolist"], copies
    assert set(res) == {"psnr", "ssim", "lpips"} and logged == {"val/" + k: v for k, v in res.items()}
    p32 = log["pred"].float() * _d(mask) + log["origin_image"] * (1 - _d(mask))
    want = float(_host_per_sample(L.seeded_state_dict(), p32[:, :, :, 64:], log["origin_image"][:, :, :, 64:]).mean())
    print("validation_result", res, want)
    assert abs(res["lpips"] - want) <= tol


def test_run_inpainting_device_lpips_end_to_end(tmp_path):
    """tools/run_inpainting.py --device_metrics --lpips_weights W with and without --device_lpips, fresh child processes, the synthetic
    set-up of tests/test_gpu_harness.py (the script's default seed 0 for the synthetic batch).  The LPIPS lines agree to the four printed decimals or within
    one unit of the last, which also covers a value that sits at a rounding boundary."""
    size = 64
    mdir = tmp_path / "synthetic_model"
    (mdir / "ckpts").mkdir(parents=True)
    _write_config(str(mdir / "model_config.yaml"), size)
    stub = tmp_path / "stubs"
    stub.mkdir()
    (stub / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    import leftrefill_amd.dropin as dropin
    dropin.install()
    sys.path.insert(0, str(stub))
    try:
        from inpainting_ldm.model import create_model
        model = create_model(str(mdir / "model_config.yaml"))
    finally:
        sys.path.remove(str(stub))
    sd = dict(model.state_dict())
    for k, v in model.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in G.unet_state("MID").items():
        sd["model.diffusion_model." + k] = v
    torch.save({"state_dict": sd}, str(mdir / "ckpts" / "epoch=3.ckpt"))
    wfile = tmp_path / "lpips_seeded.pth"
    torch.save(L.seeded_state_dict(), str(wfile))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))
    runs = {}
    for route in ("eager", "device"):
        out_dir, met_dir = tmp_path / ("out_" + route), tmp_path / ("metrics_" + route)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_inpainting.py"), "--model_path", str(mdir), "--synthetic", "1",
               "--test_size", str(size), "--metric_size", str(size), "--batch_size", "2", "--cfg", "2.5", "--eta", "0.0",
               "--output_path", str(out_dir), "--metric_output", str(met_dir), "--device_metrics", "--lpips_weights", str(wfile)] + \
              (["--device_lpips"] if route == "device" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines = {ln.split(":")[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("PSNR:", "SSIM:", "LPIPS:"))}
        metric = (met_dir / "synthetic_model.txt").read_text()
        runs[route] = dict(lines=lines, lpips=float(lines["LPIPS"].split()[1]), metric=metric)
        print(route, lines["LPIPS"])
        assert len(lines["LPIPS"].split()[1].split(".")[1]) == 4 and metric.split("\n")[2] == lines["LPIPS"]
    assert runs["eager"]["lines"]["PSNR"] == runs["device"]["lines"]["PSNR"] and runs["eager"]["lines"]["SSIM"] == runs["device"]["lines"]["SSIM"]
    assert runs["device"]["lpips"] > 0
    assert abs(runs["eager"]["lpips"] - runs["device"]["lpips"]) <= 1e-4 + 1e-9
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_inpainting.py"), "--model_path", str(mdir), "--device_lpips"],
                       capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert r.returncode != 0 and "--device_lpips requires" in r.stderr
