"""ER-NeRF avatars trained on HuBERT features (asr_model "hubert": audio_in_dim 1024, ernerf/nerf_triplane/network.py:107-108; nerfasr.py:41-43).

Fixture: tests/golden/ernerf_hubert_golden.npz, recorded from the reference's own NeRFNetwork(asr_model="hubert") by make_ernerf_hubert_golden.py; the
windows, audio nets and field are regenerated here from their seeds.  CPU: the oracle against the fixture, the HuBERT config against transformers.
GPU: the wide audio encoder (k_audio_wide_conv0 + k_audio_encode) against the fixture and the oracle, HubertModel through the wav2vec2 front end against
transformers, a frame through the drop-in, and audio -> enc_a end to end."""
import argparse
import os

import numpy as np
import pytest
import torch

from mere_fusion_amd import weights as W
from oracle import ernerf_net_ref as NR

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


@pytest.fixture(scope="module")
def hubert_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ernerf_hubert_golden.npz"))


def _windows(seed, n=8, in_dim=1024):
    """make_ernerf_hubert_golden.hubert_windows (seed 4100: the fixture's)"""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((n, in_dim, 16)).astype(np.float32)


def _audio_sd(in_dim, seed=0):
    """W.make_ernerf_audio_state_dict over the shapes of the reference's AudioNet(in_dim, 32) + AudioAttNet() (network.py:9-66)"""
    shapes = {"audio_net.encoder_conv.0": (32, in_dim, 3), "audio_net.encoder_conv.2": (32, 32, 3), "audio_net.encoder_conv.4": (64, 32, 3),
              "audio_net.encoder_conv.6": (64, 64, 3), "audio_net.encoder_fc1.0": (64, 64), "audio_net.encoder_fc1.2": (32, 64),
              "audio_att_net.attentionConvNet.0": (16, 32, 3), "audio_att_net.attentionConvNet.2": (8, 16, 3), "audio_att_net.attentionConvNet.4": (4, 8, 3),
              "audio_att_net.attentionConvNet.6": (2, 4, 3), "audio_att_net.attentionConvNet.8": (1, 2, 3), "audio_att_net.attentionNet.0": (8, 8)}
    template = {}
    for k, s in shapes.items():
        template[k + ".weight"], template[k + ".bias"] = torch.empty(s), torch.empty(s[0])
    return W.make_ernerf_audio_state_dict(template, seed)


def _hubert_cfg(cfg):
    from transformers import HubertConfig
    return HubertConfig(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, hidden_dropout=0.0, activation_dropout=0.0,
                        attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0)


def _hubert(cfg, seed=0):
    from transformers import HubertModel
    m = HubertModel(_hubert_cfg(cfg))
    m.load_state_dict(W.make_hubert_state_dict(cfg, seed), strict=True)
    return m.eval()


def _hubert_hidden(model, wav):
    """nerfasr.py:128-136 with the hubert branch: Wav2Vec2Processor (normalising feature extractor) + HubertModel(...).last_hidden_state"""
    from transformers import Wav2Vec2FeatureExtractor
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=False)
    inputs = fe([np.asarray(wav, np.float32)], sampling_rate=16000, return_tensors="pt", padding=True)
    with torch.no_grad():
        return model(inputs.input_values).last_hidden_state.numpy()


HUBERT_4L = dict(W.HUBERT_LARGE, num_hidden_layers=4)          # the large width (audio_dim 1024) at a sixth of the depth: the end-to-end chain


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_encode_audio_matches_hubert_golden(hubert_golden):
    g = hubert_golden
    sd, auds = _audio_sd(1024), torch.from_numpy(_windows(int(g["window_seed"])))
    got = NR.encode_audio(sd, auds)
    np.testing.assert_allclose(got.numpy(), g["enc_audio"], rtol=1e-5, atol=1e-6)                 # reference: model.encode_audio(auds), att 2
    np.testing.assert_allclose(NR.encode_audio(sd, auds[3:4], att=0).numpy(), g["enc_audio_att0"], rtol=1e-5, atol=1e-6)
    assert np.abs(g["enc_audio"]).max() > 0.05 and np.abs(g["enc_audio_att0"]).max() > 0.05


def test_hubert_large_config_builds_transformers_model():
    from transformers import HubertModel
    cfg = _hubert_cfg(W.HUBERT_LARGE)
    assert cfg.hidden_size == 1024 and cfg.feat_proj_layer_norm and cfg.do_stable_layer_norm and cfg.feat_extract_norm == "layer"
    with torch.device("meta"):
        model = HubertModel(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k[len("wav2vec2."):]: s for k, s in W.make_wav2vec2_state_dict(dict(W.HUBERT_LARGE, vocab_size=1), shapes_only=True).items()
            if k.startswith("wav2vec2.")}
    assert shapes == want
    assert sum(int(np.prod(s)) for s in shapes.values()) == 315_438_720        # hubert-large: 315 M parameters (masked_spec_embed included)


def test_hubert_state_dict_carries_the_keys_the_c_loader_reads():
    cfg = dict(W.HUBERT_LARGE, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7,
               num_conv_pos_embedding_groups=2)
    model = _hubert(cfg)                                                                            # strict=True inside
    keys = set(model.state_dict())
    assert "masked_spec_embed" in keys                                                              # the one key the C loader does not read
    need = {"feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias", "feature_projection.projection.weight",
            "feature_projection.projection.bias", "encoder.pos_conv_embed.conv.bias", "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
            "encoder.pos_conv_embed.conv.parametrizations.weight.original1", "encoder.layer_norm.weight", "encoder.layer_norm.bias"}
    for i in range(7):
        need |= {f"feature_extractor.conv_layers.{i}.{n}" for n in ("conv.weight", "conv.bias", "layer_norm.weight", "layer_norm.bias")}
    for l in range(2):
        need |= {f"encoder.layers.{l}.{n}.{p}" for n in ("attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj", "layer_norm",
                                                        "feed_forward.intermediate_dense", "feed_forward.output_dense", "final_layer_norm")
                 for p in ("weight", "bias")}
    assert need <= keys, sorted(need - keys)
    assert not hasattr(model, "lm_head")                                                            # from_hf -> out_hidden (.last_hidden_state)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_encode_audio_hubert_width(lib_built, hubert_golden):
    from mere_fusion_amd.ernerf.audio import HipAudioEncoder
    g = hubert_golden
    sd = _audio_sd(1024)
    a = torch.from_numpy(_windows(int(g["window_seed"]))).cuda()
    enc = HipAudioEncoder(sd, att=2)
    assert enc.in_dim == 1024
    got = enc.encode_audio(a)
    np.testing.assert_allclose(got.cpu().numpy(), g["enc_audio"], rtol=2e-5, atol=2e-6)              # fp32 both sides, different summation order
    assert torch.equal(enc.encode_audio(a), got)                                                    # no atomics: the same bits every call
    one = HipAudioEncoder(sd, att=0)
    np.testing.assert_allclose(one.encode_audio(a[3:4]).cpu().numpy(), g["enc_audio_att0"], rtol=2e-5, atol=2e-6)
    # a window that does not start on 16 bytes (the wide layer reads float4 rows): copied, same result
    flat = torch.empty(a.numel() + 1, device="cuda")
    flat[1:].copy_(a.reshape(-1))
    assert torch.equal(enc.encode_audio(flat[1:].view(8, 1024, 16)), got)
    # the lip-smoothing EMA of renderer.py:190-194 inside the launches: bit-identical to the torch expression it replaces, over a few frames
    prev_t, prev_k = None, None
    for f in range(3):
        af = a * (1.0 + 0.1 * f)
        raw = enc.encode_audio(af)
        prev_t = raw if prev_t is None else 0.35 * prev_t + (1 - 0.35) * raw
        prev_k = enc.encode_audio_smooth(af, prev_k)
        assert torch.equal(prev_k, prev_t), f
    # the window width is checked against the audio net's (a narrower window was read out of bounds)
    with pytest.raises(RuntimeError, match=r"\[n, 1024, 16\]"):
        enc.encode_audio(torch.zeros(8, 44, 16, device="cuda"))
    with pytest.raises(RuntimeError, match=r"\[n, 1024, 16\]"):
        enc.encode_audio_smooth(torch.zeros(8, 1024, 8, device="cuda"), None)
    with pytest.raises(RuntimeError, match="windows"):
        enc.encode_audio(torch.zeros(3, 1024, 16, device="cuda"))
    with pytest.raises(RuntimeError, match="1024"):
        HipAudioEncoder(_audio_sd(1025), att=2)
    # other widths of the wide path, against the oracle
    for w in (65, 128, 512):
        sdw, aw = _audio_sd(w, seed=w), torch.from_numpy(_windows(7000 + w, in_dim=w))
        e2, e0 = HipAudioEncoder(sdw, att=2), HipAudioEncoder(sdw, att=0)
        np.testing.assert_allclose(e2.encode_audio(aw.cuda()).cpu().numpy(), NR.encode_audio(sdw, aw).numpy(), rtol=2e-5, atol=2e-6, err_msg=str(w))
        np.testing.assert_allclose(e0.encode_audio(aw[5:6].cuda()).cpu().numpy(), NR.encode_audio(sdw, aw[5:6], att=0).numpy(), rtol=2e-5, atol=2e-6,
                                   err_msg=str(w))


@pytest.mark.gpu
def test_hip_hubert_front_end_vs_transformers(lib_built):
    """HubertModel(HUBERT_LARGE) as nerfasr.py:42 loads it, through HipWav2Vec2ForCTC.from_hf, then the feature ring"""
    from mere_fusion_amd.ernerf.asr import HipWav2Vec2ForCTC, NerfASRFrontend
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _hubert(W.HUBERT_LARGE, seed=1)
    m = HipWav2Vec2ForCTC.from_hf(model)                                    # masked_spec_embed in the state dict is accepted
    assert m.out_hidden
    fe = NerfASRFrontend(m, m=8, l=10, r=10, att=2, audio_dim=1024)
    wav = W.make_speech_like_wav(18 * 320, 3)
    for i in range(18):
        fe.put_audio_frame(wav[i * 320:(i + 1) * 320])
        fe.run_step()
    full = np.concatenate([np.zeros(10 * 320, np.float32), wav])           # the 10 zero frames nerfasr.py:35-36 pads on the left
    want = _hubert_hidden(model, full)
    got = m(torch.from_numpy(full)[None]).last_hidden_state.cpu().numpy()
    err = np.abs(got - want).max()
    print(f"[hubert large] last_hidden_state L-inf vs transformers {err:.3e} (|h| max {np.abs(want).max():.2f})")
    assert got.shape == want.shape == (1, 27, 1024) and err <= 2e-3
    a = fe.get_next_feat()
    assert tuple(a.shape) == (8, 1024, 16) and (a[:4] == 0).all()
    sl = want[0, 10:18].T                                                   # logits[:, l : T - r + 1] -> ring rows 0..7 (nerfasr.py:138-141)
    np.testing.assert_allclose(a[4, :, 8:].cpu().numpy(), sl, atol=2e-3)
    assert (a[4, :, :8] == 0).all()
    cfg = dict(W.HUBERT_LARGE, feat_proj_layer_norm=False)
    with pytest.raises(ValueError, match="feat_proj_layer_norm"):
        HipWav2Vec2ForCTC(cfg, {}, out_hidden=True)


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_hip_render_hubert_avatar_through_the_mixin(lib_built, hubert_golden, smooth):
    from mere_fusion_amd.ernerf.field import grid_geometry
    from mere_fusion_amd.ernerf.network import HipRenderMixin
    from test_dropin_ernerf import _ReferenceShapedBase
    g = hubert_golden
    offsets, _ = grid_geometry()
    sd = W.make_ernerf_field_state_dict(int(offsets[-1]), 0)
    sd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in sd.items()}
    sd.update(_audio_sd(1024))
    opt = argparse.Namespace(asr_model="hubert", emb=False, att=2, bound=1, min_near=0.05, exp_eye=True, smooth_lips=smooth, ind_num=16, ind_dim=4)

    class Net(HipRenderMixin, _ReferenceShapedBase):
        pass

    m = Net(opt, sd)
    with torch.no_grad():
        m.individual_codes[0].copy_(torch.from_numpy(g["render_ind_code"]))
        m.density_bitfield.copy_(torch.from_numpy(W.make_ernerf_sphere_bitfield()))
    m = m.cuda().eval()
    m.density_scale = 40.0
    Wd = int(g["render_W"])
    ro, rd = W.make_ernerf_camera_rays(Wd)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    bg = torch.tensor([0.1, 0.2, 0.3]).expand(Wd * Wd, 3).contiguous().cuda()
    kw = dict(eye=cu(g["render_e"]), index=[0], staged=True, bg_color=bg, perturb=False, dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4)
    auds = cu(_windows(int(g["window_seed"])))
    res = m.render(cu(ro)[None], cu(rd)[None], auds, torch.zeros(1, Wd * Wd, 2, device="cuda"), torch.eye(4, device="cuda")[None], **kw)
    assert m.mf_frames == 1 and tuple(res["image"].shape) == (1, Wd * Wd, 3)
    err = np.abs(res["image"].reshape(-1, 3).cpu().numpy() - g["render_image"]).max()
    derr = np.abs(res["depth"].reshape(-1).cpu().numpy() - g["render_depth"]).max()
    aerr = np.abs(res["ambient_aud"].reshape(-1).cpu().numpy() - g["render_amb_aud"])
    print(f"hubert avatar through the drop-in (smooth_lips={smooth}) vs the reference's frame: image {err:.3e}, depth {derr:.3e}, ambient_aud {aerr.max():.3e}")
    assert err <= 1e-3 and derr <= 1e-3
    assert (aerr / (1 + np.abs(g["render_amb_aud"]))).max() <= 2e-3
    m.render(cu(ro)[None], cu(rd)[None], auds * 1.1, torch.zeros(1, Wd * Wd, 2, device="cuda"), torch.eye(4, device="cuda")[None], **kw)
    assert m.mf_frames == 2
    if smooth:
        assert m.enc_a is not None and tuple(m.enc_a.shape) == (1, 32)


@pytest.mark.gpu
def test_hip_hubert_audio_to_enc_a_end_to_end(lib_built):
    """speech-like wav -> HuBERT front end -> feature ring -> wide audio encoder, against transformers + the oracle on the same audio"""
    from mere_fusion_amd.ernerf.asr import HipWav2Vec2ForCTC, NerfASRFrontend
    from mere_fusion_amd.ernerf.audio import HipAudioEncoder
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _hubert(HUBERT_4L, seed=2)
    fe = NerfASRFrontend(HipWav2Vec2ForCTC.from_hf(model), m=8, l=10, r=10, att=2, audio_dim=1024)
    sd = _audio_sd(1024, seed=3)
    enc = HipAudioEncoder(sd, att=2)
    n = 18 + 8 + 8                                                          # three network calls: ring rows 0..23
    wav = W.make_speech_like_wav(n * 320, 4)
    frames = [np.zeros(320, np.float32)] * 10 + [wav[i * 320:(i + 1) * 320] for i in range(n)]
    ring = torch.zeros(32, 1024)
    for c, end in enumerate((28, 36, 44)):                                  # the oracle's own ring (nerfasr.py:105-124)
        h = _hubert_hidden(model, np.concatenate(frames[end - 28:end]))
        ring[8 * c:8 * c + 8] = torch.from_numpy(h[0, 10:18])
    for i in range(n):
        fe.put_audio_frame(frames[10 + i])
        fe.run_step()
    np.testing.assert_allclose(fe.feat_queue.cpu().numpy(), ring.numpy(), atol=2e-3)
    front, tail = 24, 8
    att = [torch.zeros(1024, 16)] * 4
    for step in range(6):
        while len(att) < 8:                                                  # nerfasr.py:75-103
            win = torch.cat([ring[front:], ring[:tail]]) if front >= tail else ring[front:tail]
            front, tail = (front + 2) % 32, (tail + 2) % 32
            att.append(win.T.contiguous())
        want_a = torch.stack(att)
        att = att[1:]
        a = fe.get_next_feat()
        got = enc.encode_audio(a)
        want = NR.encode_audio(sd, want_a)
        tight = NR.encode_audio(sd, a.cpu())                                # the encoder alone, on the device's own windows
        np.testing.assert_allclose(got.cpu().numpy(), tight.numpy(), rtol=2e-5, atol=2e-6)
        err = (got.cpu() - want).abs().max().item()
        print(f"[hubert -> enc_a] step {step}: L-inf vs transformers + oracle {err:.3e} (|enc_a| max {want.abs().max().item():.3f})")
        # front-end differences of <= 2e-3 on O(1) features, through conv[0]'s 3072-term sums with He-scaled weights and 12 more layers
        assert err <= 5e-3
