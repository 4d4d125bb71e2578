"""The number format's own limit on a stressed UNet (tests/test_musetalk_unet_stress.py), on the host: the float64 oracle against the same oracle with every
conv / linear input, weight, bias and output rounded to the format -- a bf16x3 (hi, lo) pair, or one bf16 -- at the layer boundaries.  A GPU error of the same
size as this one is the format's; a larger one is a kernel's.

  python tools/unet_stress_emulation.py --config small --batch 3 --seed 31 --format bf16x3 none token_offset all
  python tools/unet_stress_emulation.py --config full --batch 2 --seed 41 --format bf16x3 all --tau 24
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_musetalk_unet_stress as S  # noqa: E402
from mere_fusion_amd import weights as W  # noqa: E402
from oracle import musetalk_ref as R  # noqa: E402


def _rounder(fmt):
    def x3(t):
        h = t.bfloat16().double()
        return h + (t - h).bfloat16().double()

    def b16(t):
        return t.bfloat16().double()
    return x3 if fmt == "bf16x3" else b16


class _RoundingF:
    def __init__(self, q):
        self.q = q

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, x, w, b=None, **k):
        q = self.q
        return q(F.conv2d(q(x), q(w), None if b is None else q(b), **k))

    def linear(self, x, w, b=None):
        q = self.q
        return q(F.linear(q(x), q(w), None if b is None else q(b)))


def emulate(sd, cfg, lat, aud, fmt):
    """(L-inf of the rounded run against the exact one, max |latent|)"""
    want = S.unet_fp64(sd, cfg, lat, aud)
    saved = R.F
    R.F = _RoundingF(_rounder(fmt))
    try:
        got = S.unet_fp64(sd, cfg, lat, aud)
    finally:
        R.F = saved
    return float((got - want).abs().max()), float(want.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stressors", nargs="+", help="none, all, or names from STRESSORS")
    ap.add_argument("--config", choices=("small", "full"), default="small")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--format", choices=("bf16x3", "bf16"), default="bf16x3")
    ap.add_argument("--token-r", type=float)
    ap.add_argument("--group-r", type=float)
    ap.add_argument("--tau", type=float)
    ap.add_argument("--ln-gain", type=float)
    a = ap.parse_args()
    if a.ln_gain is not None:
        S.LN_GAIN = a.ln_gain
    cfg = S.SMALL if a.config == "small" else S.MUSETALK_V1
    usd = W.make_musetalk_unet_state_dict(cfg, 0)
    lat, aud = W.make_musetalk_inputs(a.batch, a.seed)
    dt = torch.float64 if a.config == "small" else torch.float32
    rec = S.record(usd, cfg, lat, aud, dtype=dt)
    for name in a.stressors:
        sd, n = (usd, 0) if name == "none" else S.stress(name, usd, rec, lambda s: S.record(s, cfg, lat, aud, dtype=dt), token_r=a.token_r,
                                                         group_r=a.group_r, tau=a.tau)
        err, scale = emulate(sd, cfg, lat, aud, a.format)
        print(f"{name} ({n} layers), {a.format} at the layer boundaries: latents L-inf {err:.3e}, / max|latent| {err / scale:.3e}")


if __name__ == "__main__":
    main()
