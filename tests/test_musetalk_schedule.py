"""The MuseTalk schedules themselves: (name, kernel, flops per frame) of every op of a handle, read through mf_unet_op_info / mf_vae_op_info right after
create (no forward runs), equal to the lists recorded under tests/golden/musetalk_schedule_*.json.

Parity tests cannot see a lost GroupNorm-statistics hand-off, a moved op or a dropped dual path: the numbers stay within tolerance and only the speed goes.
The fixtures were recorded with the shipped tuning table (MF_TUNE_CACHE, MF_AUTOTUNE and the MF_FORCE_* variables unset).  A later change to a kernel, a
tile choice or the op order re-records the fixture on purpose; a change that is meant to leave the schedules alone must leave this test alone."""
import ctypes as C
import json
import os

import pytest

from mere_fusion_amd import weights as W
from mere_fusion_amd.musetalk.config import MUSETALK_V1, unet_config_json, vae_config_json

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def shipped_launch_configurations(monkeypatch):
    for k in [k for k in os.environ if k in ("MF_TUNE_CACHE", "MF_AUTOTUNE") or k.startswith("MF_FORCE_")]:
        monkeypatch.delenv(k)


def _ops(h, num_ops, op_info):
    out = []
    for i in range(num_ops(h)):
        nm, kn, fl = C.create_string_buffer(256), C.create_string_buffer(256), C.c_double()
        assert op_info(h, i, nm, 256, kn, 256, C.byref(fl)) == 0
        out.append([nm.value.decode(), kn.value.decode(), fl.value])
    return out


def _check(tag, got, must_contain):
    with open(os.path.join(GOLDEN, f"musetalk_schedule_{tag}.json")) as f:
        want = json.load(f)
    kernels = " ; ".join(k for _, k, _ in want) + " ; " + " ; ".join(n for n, _, _ in want)
    for s in must_contain:                       # the fixture exercises the paths it is there to pin
        assert s in kernels, (tag, s)
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (tag, i, g, w)


def _small_unet_cfg(c):
    return dict(in_channels=c["in_channels"], out_channels=c["out_channels"], block_out_channels=list(c["block_out_channels"]),
                layers_per_block=c["layers_per_block"], cross_attention_dim=c["cross_attention_dim"], attention_head_dim=c["attention_heads"],
                norm_num_groups=c["norm_num_groups"], down_attn=c["down_attn"], up_attn=c["up_attn"], sample_size=32)


def test_small_unet_and_vae_schedules(lib_built):
    """MUSETALK_SMALL at max_batch 4, as tests/test_musetalk.py builds them."""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.musetalk.models.unet import UNet
    from mere_fusion_amd.musetalk.models.vae import VAE
    from oracle import musetalk_ref as R
    cfg, l = R.MUSETALK_SMALL, _lib.lib()
    unet = UNet(_small_unet_cfg(cfg["unet"]), W.make_musetalk_unet_state_dict(cfg, 0), max_batch=4)
    _check("small_unet_b4", _ops(unet.model._h, l.mf_unet_num_ops, l.mf_unet_op_info),
           ["statistics from the producer's epilogue", "cross-attention k | v of every block"])
    vc = dict(cfg["vae"]); vc["block_out_channels"] = list(vc["block_out_channels"])
    vae = VAE(config=vc, state_dict=W.make_musetalk_vae_state_dict(cfg, 0), max_batch=4)
    _check("small_vae_b4", _ops(vae._h, l.mf_vae_num_ops, l.mf_vae_op_info), ["statistics from the producer's epilogue", "k_gn_conv3_tail"])


def test_full_vae_schedule_takes_the_f16_fp6_paths(lib_built):
    """MUSETALK_V1 decoder at 8 frames (tests/test_musetalk_stress.py): f16 + FP6 resnet convs and upsamplers, the fused tail."""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.musetalk.models.vae import VAE
    l = _lib.lib()
    vae = VAE(config=vae_config_json(MUSETALK_V1["vae"]), state_dict=W.make_musetalk_vae_state_dict(MUSETALK_V1, 0), max_batch=8)
    _check("v1_vae_b8", _ops(vae._h, l.mf_vae_num_ops, l.mf_vae_op_info),
           ["k_affine_silu_to_q (statistics from the producer's epilogue)", "(input -> f16 + FP6)", "k_gn_conv3_tail"])


def test_full_unet_schedule_takes_the_dual_path(lib_built):
    """MUSETALK_V1 UNet on a 16-frame handle (state dict as tests/test_musetalk_full.py): the dual-path layers are built."""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.musetalk.models.unet import UNet
    l = _lib.lib()
    unet = UNet(unet_config_json(MUSETALK_V1["unet"]), W.make_musetalk_unet_state_dict(MUSETALK_V1, 0), max_batch=16)
    _check("v1_unet_b16", _ops(unet.model._h, l.mf_unet_num_ops, l.mf_unet_op_info),
           ["from q_dual_min frames", "statistics from the producer's epilogue", "cross-attention k | v of every block"])
