"""A transformer block's `ff.net.2` and `proj_out` folded into one layer (Builder::ff_proj_out, mf_musetalk_build.hip).
MF_FF_PROJ_FOLD=0 builds the chain, =1 the fold on every handle; unset, a handle folds where the tuning table holds the fused layer at its capacity, which the
one-block networks below are not -- so both sides of the comparison set the switch.

Between the two layers lies nothing nonlinear, so with gg the GEGLU output, r the residual stream behind the cross-attention and x the block's input

    y = W_po (W_f2 gg + b_f2 + r) + b_po + x = [W_po W_f2 | W_po] [gg ; r] + (W_po b_f2 + b_po) + x

CPU: that identity in float64, with the concat order and the bias the builder uses.  GPU: one-block UNets (the smallest the builder accepts) run once with the
chain and once folded, each in a fresh child process (the switch is latched per process), against each other and against oracle/musetalk_ref.py.

Tolerance.  The fold moves one bf16x3 rounding (the product W_po W_f2 is rounded once, where the chain rounds vB between its two layers); the measure is the
chain's own distance from the fp32 oracle on these configurations, L-inf over the predicted latents, measured on an MI355X:

    configuration                  chain vs oracle   folded vs oracle   folded vs chain
    C 320, 8 x 8, batch 1          1.399e-05         1.375e-05          1.144e-05
    C 320, 8 x 8, batch 3          1.779e-05         1.770e-05          1.526e-05
    C 1280, 4 x 4, batch 1         1.222e-05         7.719e-06          7.629e-06
    C 1280, 4 x 4, batch 3         1.213e-05         1.377e-05          8.106e-06

The folded path must stay within 2 x the chain's figure of the same case (CHAIN_ERR below), and within the latent gate of tests/test_musetalk_full.py (1e-4);
folded and chain may differ by at most the same amount."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mere_fusion_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_LATENT = 1e-4            # tests/test_musetalk_full.py

# the smallest UNets the builder accepts: one block, one layer per block.  C = 1280 on a 4 x 4 map: K = 5C = 6400 is where split-K engages.
CONFIGS = {
    "c320": dict(in_channels=8, out_channels=4, block_out_channels=[320], layers_per_block=1, cross_attention_dim=384, attention_heads=8,
                 norm_num_groups=32, down_attn=[True], up_attn=[True], sample_size=8),
    "c1280": dict(in_channels=8, out_channels=4, block_out_channels=[1280], layers_per_block=1, cross_attention_dim=384, attention_heads=8,
                  norm_num_groups=32, down_attn=[True], up_attn=[False], sample_size=4),
}
BATCHES = (1, 3)
# chain (MF_FF_PROJ_FOLD=0: the schedule of the parent commit) against the oracle, L-inf of the latents, measured on an MI355X
CHAIN_ERR = {("c320", 1): 1.399e-5, ("c320", 3): 1.779e-5, ("c1280", 1): 1.222e-5, ("c1280", 3): 1.213e-5}


# ---- CPU: the algebra ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [320, 640])
def test_fold_algebra_float64(C):
    rng = np.random.default_rng(C)
    T = 5
    w_f2, b_f2 = rng.standard_normal((C, 4 * C)) / np.sqrt(4 * C), rng.standard_normal(C)
    w_po, b_po = rng.standard_normal((C, C)) / np.sqrt(C), rng.standard_normal(C)
    gg, r, x = rng.standard_normal((T, 4 * C)), rng.standard_normal((T, C)), rng.standard_normal((T, C))
    chain = (gg @ w_f2.T + b_f2 + r) @ w_po.T + b_po + x
    w = np.concatenate([w_po @ w_f2, w_po], axis=1)                      # [W_po W_f2 | W_po]: K = 5C
    b = w_po @ b_f2 + b_po
    folded = np.concatenate([gg, r], axis=1) @ w.T + b + x               # over [gg ; r]
    assert w.shape == (C, 5 * C)
    assert np.abs(folded - chain).max() <= 1e-12 * np.abs(chain).max()
    # the order matters: [r ; gg] against the same weights is another function
    swapped = np.concatenate([r, gg[:, :3 * C], gg[:, 3 * C:]], axis=1) @ w.T + b + x
    assert np.abs(swapped - chain).max() > 1e-3 * np.abs(chain).max()


# ---- GPU: chain and fold in child processes ------------------------------------------------------------------------------------------------------------------
def _inputs(tag, batch):
    return W.make_musetalk_inputs(batch, 40 + batch, hw=CONFIGS[tag]["sample_size"])


CHILD = """
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from mere_fusion_amd import weights as W
from mere_fusion_amd.musetalk.models.unet import UNet
configs, batches, out = json.loads(sys.argv[2]), json.loads(sys.argv[3]), {}
for tag, cfg in configs.items():
    unet = UNet(cfg, W.make_musetalk_unet_state_dict(cfg, 0), max_batch=max(batches))
    for b in batches:
        lat, aud = W.make_musetalk_inputs(b, 40 + b, hw=cfg["sample_size"])
        pred = unet.model(lat.cuda(), torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(aud.cuda())).sample
        out[f"{tag}_{b}"] = pred.float().cpu().numpy()
    del unet
np.savez(sys.argv[4], **out)
"""


@pytest.fixture(scope="module")
def runs(lib_built, tmp_path_factory):
    """{fold: {"<config>_<batch>": latents}}: one fresh process per value of the switch runs every configuration and batch."""
    d = tmp_path_factory.mktemp("ff_proj_fold")
    got = {}
    for fold in ("0", "1"):
        path = str(d / f"fold{fold}.npz")
        subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(CONFIGS), json.dumps(BATCHES), path], check=True,
                       env=dict(os.environ, MF_FF_PROJ_FOLD=fold), timeout=600)
        got[fold] = dict(np.load(path))
    return got


@pytest.fixture(scope="module")
def oracle():
    from oracle import musetalk_ref as R
    want = {}
    for tag, cfg in CONFIGS.items():
        sd = W.make_musetalk_unet_state_dict(cfg, 0)
        for b in BATCHES:
            lat, aud = _inputs(tag, b)
            want[f"{tag}_{b}"] = R.unet_forward(sd, cfg, lat, torch.tensor([0]), R.add_positional_encoding(aud)).numpy()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_fold_against_chain_and_oracle(runs, oracle, tag, batch):
    key = f"{tag}_{batch}"
    chain, fold, want = runs["0"][key], runs["1"][key], oracle[key]
    e_chain, e_fold, e_ab = (float(np.abs(a - b).max()) for a, b in ((chain, want), (fold, want), (fold, chain)))
    print(f"ff.net.2 + proj_out fold, {key}: chain vs oracle {e_chain:.3e}, folded vs oracle {e_fold:.3e}, folded vs chain {e_ab:.3e} "
          f"(latents |max| {np.abs(want).max():.2f})")
    bound = min(2.0 * CHAIN_ERR[(tag, batch)], TOL_LATENT)
    assert e_chain <= TOL_LATENT, e_chain
    assert e_fold <= bound, (e_fold, bound)
    assert e_ab <= bound, (e_ab, bound)
