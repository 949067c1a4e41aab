"""tools/run_inpainting.py --fid_weights W --device_fid on the synthetic set-up of tests/test_gpu_harness.py: a finite `FID:` line in the
printout and the metric file, and every other line and every PNG byte as in a run without the two flags."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_eval_metrics import _write_config  # noqa: E402  (the tiny model of tests/test_gpu_harness.py)
from oracle import golden_spec as G, weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_inpainting_device_fid_end_to_end(tmp_path):
    from leftrefill_amd import fid
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
    wfile = tmp_path / "fid_seeded.pth"
    torch.save(fid.seeded_state_dict(0), str(wfile))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))
    runs = {}
    for route in ("plain", "fid"):
        out_dir, met_dir = tmp_path / ("out_" + route), tmp_path / ("metrics_" + route)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_inpainting.py"), "--model_path", str(mdir), "--synthetic", "2",
               "--test_size", str(size), "--metric_size", str(size), "--batch_size", "2", "--cfg", "2.5", "--eta", "0.0", "--steps", "4",
               "--output_path", str(out_dir), "--metric_output", str(met_dir), "--device_metrics"] + \
              (["--fid_weights", str(wfile), "--device_fid"] if route == "fid" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("PSNR:", "SSIM:", "LPIPS:", "FID:"))]
        pngs = {p.name: p.read_bytes() for p in sorted(out_dir.glob("*.png"))}
        runs[route] = dict(lines=lines, metric=(met_dir / "synthetic_model.txt").read_text(), pngs=pngs)
        print(route, lines)
    plain, with_fid = runs["plain"], runs["fid"]
    assert len(plain["lines"]) == 3 and with_fid["lines"][:3] == plain["lines"] and len(with_fid["lines"]) == 4
    value = float(with_fid["lines"][3].split()[1])
    assert with_fid["lines"][3].startswith("FID: ") and math.isfinite(value) and value > 0
    assert with_fid["metric"] == plain["metric"] + with_fid["lines"][3] + "\n" and "FID" not in plain["metric"]
    assert len(plain["pngs"]) == 4 and with_fid["pngs"] == plain["pngs"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_inpainting.py"), "--model_path", str(mdir), "--device_fid"],
                       capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert r.returncode != 0 and "--device_fid requires" in r.stderr
