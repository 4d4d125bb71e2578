"""BASELINE.json configs[2] at FULL size under `-m gpu`: the MuseTalk-v1 UNet (850 M weights, 367 ops, fused attention dh 40 / 80 / 160,
split-K, halo_w twins) and the sd-vae-ft-mse decoder at batch 8 against oracle/musetalk_ref.py, through the drop-in objects -> C ABI.

Parity bar (BASELINE.json north_star): fp32 L-inf <= 1e-3 on the predicted latents; uint8 frames within one grey level of the oracle's
(round-half-even ties of `(x * 255).round()`, vae.py:106) with the differing fraction stated and bounded.
PARITY UNPINNED at the diffusers boundary (oracle header); the oracle needs ~1 min of host time for the batch-8 step."""
import numpy as np
import pytest
import torch

from mere_fusion_amd import weights as W
from mere_fusion_amd.musetalk.config import MUSETALK_V1, unet_config_json, vae_config_json
from mere_fusion_amd.tune_grid import batches as grid_batches

pytestmark = pytest.mark.gpu

B = 8
# The parity BOUND is the north star's (fp32 L-inf <= 1e-3; frames within one grey level).  The GATES below sit at about 3 x what the product measures
# on an MI355X (profiles/r02_full_size_parity.txt: latents 2.8e-5, image 1.8e-4, 0.19-0.24 % of uint8 pixels off by one), so that a 10 x regression
# that still meets the bound does not pass unnoticed.
TOL_LATENT = 1e-4          # measured 2.8e-5 (bound 1e-3)
TOL_IMAGE = 6e-4           # decoder output before the clamp, values in about [-4, 4]; measured 1.8e-4 (bound 1e-3 relative = 4e-3)
TOL_U8_FRACTION = 0.007    # fraction of uint8 pixels off by one level (round-half ties); measured 0.0019 - 0.0024
# The single-pass bf16 mode (bench.py's `alt` legs) is not held to the north star's bound; its gates sit at about 3 x what it first measured on an
# MI355X (batch 1 / 8 of the grid, 8-frame handles), and its error must stay at least 10 x the bf16x3 error, or the handle did not switch mode.
TOL_BF16_LATENT = 4.5e-2   # measured 1.40e-2 / 1.49e-2 (bf16x3 on the same handles: 2.3e-5 / 2.8e-5)
TOL_BF16_IMAGE = 2e-1      # measured 5.5e-2 / 6.8e-2 (bf16x3: 1.5e-4 / 1.7e-4)
TOL_BF16_U8 = 24           # uint8 max diff; measured 7 / 8, with 55-56 % of the pixels differing


@pytest.fixture(scope="module")
def full_sd():
    return W.make_musetalk_unet_state_dict(MUSETALK_V1, 0), W.make_musetalk_vae_state_dict(MUSETALK_V1, 0)


@pytest.fixture(scope="module")
def hip_full(lib_built, full_sd):
    """The handles of this module run as a deployment does: launch configurations from the tuning table shipped beside the library."""
    from mere_fusion_amd.musetalk.models.unet import UNet
    from mere_fusion_amd.musetalk.models.vae import VAE
    usd, vsd = full_sd
    unet = UNet(unet_config_json(MUSETALK_V1["unet"]), usd, max_batch=B)
    vae = VAE(config=vae_config_json(MUSETALK_V1["vae"]), state_dict=vsd, max_batch=B)
    return unet, vae


@pytest.fixture(scope="module")
def oracle_full(full_sd):
    """One batch-8 step of the fp32 oracle: predicted latents, pre-clamp decoder image, uint8 frames."""
    import os
    from oracle import musetalk_ref as R
    assert R.MUSETALK_V1 == MUSETALK_V1                      # the product's table and the checker's agree
    usd, vsd = full_sd
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 32)))
    lat, aud = W.make_musetalk_inputs(B, 11)
    pred = R.unet_forward(usd, MUSETALK_V1["unet"], lat, torch.tensor([0]), R.add_positional_encoding(aud))
    img = R.vae_decode(vsd, MUSETALK_V1["vae"], pred / MUSETALK_V1["vae"]["scaling_factor"])
    u8 = R.decode_latents(vsd, MUSETALK_V1["vae"], pred)
    return dict(lat=lat, aud=aud, pred=pred, img=img, u8=u8)


def _step(unet, vae, lat, aud):
    pred = unet.model(lat.cuda(), torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(aud.cuda())).sample
    return pred, vae.decode_latents_device(pred)


def test_full_unet_batch8_vs_oracle(hip_full, oracle_full):
    unet, _ = hip_full
    o = oracle_full
    got = unet.model(o["lat"].cuda(), torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(o["aud"].cuda())).sample.cpu()
    assert got.shape == o["pred"].shape == (B, 4, 32, 32)
    err = (got - o["pred"]).abs().max().item()
    print(f"MUSETALK_V1 UNet, batch {B}: latents L-inf vs oracle {err:.3e} (bound {TOL_LATENT})")
    assert err <= TOL_LATENT, err
    # batch-composition invariance at full size: frames 2 and 5 alone (other tile / split choices) agree with the batch-8 result
    sub = unet.model(o["lat"][[2, 5]].cuda(), torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(o["aud"][[2, 5]].cuda())).sample.cpu()
    sub_err = (sub - got[[2, 5]]).abs().max().item()
    print(f"batch-composition: frames 2, 5 alone vs inside the batch of 8: {sub_err:.3e}")
    assert sub_err <= 1e-4


def test_full_vae_batch8_vs_oracle(hip_full, oracle_full):
    """The decoder alone on the ORACLE's latents (so the comparison isolates the VAE): pre-clamp image and uint8 BGR frames."""
    _, vae = hip_full
    o = oracle_full
    frames, image = vae.decode_latents_device(o["pred"].cuda(), want_image=True)
    ierr = (image.cpu() - o["img"]).abs().max().item()
    got = frames.cpu().numpy()
    assert got.shape == o["u8"].shape == (B, 256, 256, 3) and got.dtype == np.uint8
    d = np.abs(got.astype(int) - o["u8"].astype(int))
    print(f"sd-vae-ft-mse decoder, batch {B}: image L-inf {ierr:.3e} (bound {TOL_IMAGE}); uint8 max diff {d.max()}, "
          f"differing pixels {100 * (d > 0).mean():.3f} %")
    assert ierr <= TOL_IMAGE, ierr
    assert d.max() <= 1 and (d > 0).mean() < TOL_U8_FRACTION, (d.max(), (d > 0).mean())
    assert o["u8"].std() > 10                                 # the frames are not flat


def test_full_step_graph_replay_vs_oracle(hip_full, oracle_full):
    """musereal.py:100-108 end to end at batch 8: call 1 eager, call 2 captures the hipGraphs, calls 3-4 replay them."""
    unet, vae = hip_full
    o = oracle_full
    outs = [_step(unet, vae, o["lat"], o["aud"])[1].cpu().numpy() for _ in range(4)]
    for x in outs[1:]:
        assert np.array_equal(x, outs[0])
    d = np.abs(outs[0].astype(int) - o["u8"].astype(int))
    print(f"full step, batch {B}, graph replay: uint8 max diff vs oracle {d.max()}, differing pixels {100 * (d > 0).mean():.3f} %")
    assert d.max() <= 1 and (d > 0).mean() < TOL_U8_FRACTION, (d.max(), (d > 0).mean())


def test_full_graphs_survive_other_batch_sizes(hip_full, oracle_full):
    """split-K workspaces are sized by a batch-dependent cost model and a captured graph keeps the pointer it was captured
    with.  Replay batch 8, run other batch sizes eagerly (they may outgrow a workspace), replay batch 8 again: identical frames."""
    unet, vae = hip_full
    o = oracle_full
    first = [_step(unet, vae, o["lat"], o["aud"])[1].cpu().numpy() for _ in range(3)][-1]       # eager, capture, replay
    for b in (1, 3, 5, 2):
        for _ in range(2):
            _step(unet, vae, o["lat"][:b], o["aud"][:b])
    again = _step(unet, vae, o["lat"], o["aud"])[1].cpu().numpy()
    assert np.array_equal(first, again)


def test_full_vae_batch8_matches_batch1(hip_full):
    """Batch 8 runs the resnet convs on the LDS-weights halo kernel's fat tiles (channel-slice split on the 32 x 32 levels); batch 1 takes the
    implicit-GEMM twins.  Same latents -> same frames, to the uint8 rounding of the two summation orders."""
    _, vae = hip_full
    g = torch.Generator().manual_seed(5)
    lat = (torch.randn(8, 4, 32, 32, generator=g) * 0.9).cuda()
    f8 = vae.decode_latents_device(lat).clone()
    assert float(f8.float().std()) > 10
    for i in (0, 3, 7):
        f1 = vae.decode_latents_device(lat[i:i + 1])
        d = (f1[0].int() - f8[i].int()).abs()
        print(f"VAE batch 1 vs batch 8, frame {i}: uint8 max diff {int(d.max())}, differing pixels {100 * float((d > 0).float().mean()):.3f} %")
        assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 0.01, (i, int(d.max()), float((d > 0).float().mean()))


def test_full_unet_copies_of_a_frame_are_bit_identical_at_every_batch_position(hip_full):
    """Eight copies of ONE frame in a batch: the eight outputs must be the same bits, call after call.  (The five-copy check of the 40-frame handle below places
    copies 8 frames apart, where every copy meets the same tile and fragment positions.  This one caught a LayerNorm-folding epilogue whose packed FMAs returned a
    wrong channel for a 16-pixel fragment now and then -- 1.6e-5 between copies 0 and 3 in one build of the library, 1e-2 noise in another: DESIGN.md section 4.)"""
    unet, vae = hip_full
    lat, aud = W.make_musetalk_inputs(1, 3)
    lat, aud = lat.repeat(B, 1, 1, 1).cuda(), aud.repeat(B, 1, 1).cuda()
    first = None
    for call in range(3):
        pred = unet.model(lat, torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(aud)).sample
        frames = vae.decode_latents_device(pred)
        for k in range(1, B):
            assert torch.equal(pred[k], pred[0]), (call, k, float((pred[k] - pred[0]).abs().max()))
            assert torch.equal(frames[k], frames[0]), (call, k)
        if first is None:
            first = pred.clone()
        assert torch.equal(pred, first), call


def test_full_unet_large_batch_handle_vs_oracle(full_sd, oracle_full):
    """A UNet handle at 40 frames per step (five sessions in one MuseBatcher step): the 320-channel 3x3 convs of the 32 x 32 level run on the LDS-weights
    halo tile there (the implicit GEMM below 40 frames), the 256 x 256 implicit-GEMM tiles appear -- kernel choices the batch-8 handle never makes.  The
    oracle's 8 inputs, tiled 5 x: same parity bar as batch 8, and the five copies agree."""
    from mere_fusion_amd.musetalk.models.unet import UNet
    usd, _ = full_sd
    o = oracle_full
    unet = UNet(unet_config_json(MUSETALK_V1["unet"]), usd, max_batch=40)
    lat, aud = o["lat"].repeat(5, 1, 1, 1).cuda(), o["aud"].repeat(5, 1, 1).cuda()
    got = unet.model(lat, torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(aud)).sample.cpu()
    err = (got[:B] - o["pred"]).abs().max().item()
    rep = max((got[k * B:(k + 1) * B] - got[:B]).abs().max().item() for k in (1, 2, 3, 4))
    print(f"MUSETALK_V1 UNet, handle for 40 frames: latents L-inf vs oracle {err:.3e} (gate {TOL_LATENT}); copies of a frame differ by {rep:.3e}")
    assert err <= TOL_LATENT, err
    assert rep <= 1e-4, rep
    # The same handle at 8 frames: its 320- / 640-channel 3x3 convs of the 32 x 32 / 16 x 16 levels are built twice (f16 + FP6 halo tile from 40 frames per step,
    # bf16x3 below) and a launch picks by its batch -- both sides of that switch against the oracle, and a 40-frame step again afterwards.
    small = unet.model(lat[:B], torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(aud[:B])).sample.cpu()
    err8 = (small - o["pred"]).abs().max().item()
    again = unet.model(lat, torch.tensor([0]).cuda(), encoder_hidden_states=unet.pe(aud)).sample.cpu()
    print(f"... the same handle at 8 frames: {err8:.3e}; 40 frames again: identical = {bool(torch.equal(again, got))}")
    assert err8 <= TOL_LATENT, err8
    assert torch.equal(again, got)


def test_full_vae_large_batch_handle_vs_oracle(full_sd, oracle_full):
    """A handle built for 24 frames per step (the cross-session batcher's regime): every resnet conv and all three upsamplers fill the chip in the
    f16 + FP6 format there (no channel-slice split, the 32 x 32 upsampler included) -- kernel choices the batch-8 handle never makes.  The oracle's
    8 latents, tiled 3 x: same parity bar as batch 8, and the three copies of a frame agree to the uint8 rounding."""
    from mere_fusion_amd.musetalk.models.vae import VAE
    _, vsd = full_sd
    o = oracle_full
    vae = VAE(config=vae_config_json(MUSETALK_V1["vae"]), state_dict=vsd, max_batch=24)
    lat = o["pred"].repeat(3, 1, 1, 1).cuda()
    frames, image = vae.decode_latents_device(lat, want_image=True)
    ierr = (image.cpu()[:B] - o["img"]).abs().max().item()
    got = frames.cpu().numpy()
    d = np.abs(got[:B].astype(int) - o["u8"].astype(int))
    print(f"sd-vae-ft-mse decoder, handle for 24 frames: image L-inf {ierr:.3e}; uint8 max diff {d.max()}, differing pixels {100 * (d > 0).mean():.3f} %")
    assert ierr <= TOL_IMAGE, ierr
    assert d.max() <= 1 and (d > 0).mean() < TOL_U8_FRACTION, (d.max(), (d > 0).mean())
    for k in (1, 2):
        dk = np.abs(got[k * B:(k + 1) * B].astype(int) - got[:B].astype(int))
        assert dk.max() <= 1 and (dk > 0).mean() < TOL_U8_FRACTION


def test_algorithmic_flops_match_the_oracle_count(hip_full):
    """bench.py's FLOP numerator comes from the handles' own op lists; it must equal the analytic count of SURVEY Appendix C."""
    from mere_fusion_amd.musetalk.config import algorithmic_flops_per_frame
    from oracle import musetalk_ref as R
    fu, fv = algorithmic_flops_per_frame(*hip_full)
    m = R.count_macs(MUSETALK_V1)
    assert abs(fu / (2 * m["unet"]) - 1) < 5e-3 and abs(fv / (2 * m["vae"]) - 1) < 5e-3, (fu, 2 * m["unet"], fv, 2 * m["vae"])


def _grid_order(b):
    """The oracle's frame at each of b positions: frame (3 k + b) % 8 at position k, so a frame lands at other positions from batch size to batch size
    (3 is prime to 8: positions k and k % 8 hold the same frame)."""
    return [(3 * k + b) % B for k in range(b)]


@pytest.fixture(scope="module")
def hip_full_64(lib_built, full_sd):
    """A UNet + VAE pair built for 64 frames per step, as tools/make_tune_cache.py and MuseBatcher build them: one handle serves every step size up to it."""
    from mere_fusion_amd.musetalk.models.unet import UNet
    from mere_fusion_amd.musetalk.models.vae import VAE
    usd, vsd = full_sd
    return (UNet(unet_config_json(MUSETALK_V1["unet"]), usd, max_batch=64),
            VAE(config=vae_config_json(MUSETALK_V1["vae"]), state_dict=vsd, max_batch=64))


def _vae_vs_oracle(vae, o, idx):
    """the decoder alone on the oracle's latents in the order idx: (frames, image L-inf, uint8 max diff, fraction of differing uint8 pixels)"""
    frames, image = vae.decode_latents_device(o["pred"][idx].cuda(), want_image=True)
    ierr = (image.cpu() - o["img"][idx]).abs().max().item()
    d = np.abs(frames.cpu().numpy().astype(int) - o["u8"][idx].astype(int))
    return frames, ierr, int(d.max()), float((d > 0).mean())


def test_full_every_grid_batch_on_a_64_frame_handle_vs_oracle(hip_full_64, oracle_full):
    """Every bf16x3 batch size of the tuning table's grid (tune/gfx950.txt: a launch configuration per layer for each, and the handle's capacity switches
    formats -- q_dual_min() in mf_musetalk.hip) on the 64-frame handles, in ascending order: the oracle's 8 frames in a batch-dependent order, each row held
    to the oracle's latents / image / uint8 frames, copies of a frame bit-identical, and the step bit-identical through eager, capture and replay.  Then 64
    and 8 again, identical to their first results after every other size has run (split-K workspaces, captured graphs)."""
    unet, vae = hip_full_64
    o = oracle_full
    first, failed = {}, []
    for b in grid_batches("musetalk", "bf16x3"):
        idx = _grid_order(b)
        lat, aud = o["lat"][idx].cuda(), o["aud"][idx].cuda()
        calls = [tuple(t.clone() for t in _step(unet, vae, lat, aud)) for _ in range(3)]          # eager, capture, replay
        pred, frames = calls[0]
        first[b] = (pred.cpu(), frames.cpu())
        lerr = (pred.cpu() - o["pred"][idx]).abs().max().item()
        vframes, ierr, u8max, u8frac = _vae_vs_oracle(vae, o, idx)
        print(f"MuseTalk bf16x3, batch {b:2d} (64-frame handles): latents L-inf {lerr:.3e}, image L-inf {ierr:.3e}, "
              f"uint8 max diff {u8max}, differing pixels {100 * u8frac:.3f} %")
        if not (lerr <= TOL_LATENT and ierr <= TOL_IMAGE and u8max <= 1 and u8frac < TOL_U8_FRACTION):
            failed.append((b, "vs oracle", lerr, ierr, u8max, u8frac))
        for c, (p, f) in enumerate(calls[1:], 1):
            if not (torch.equal(p, pred) and torch.equal(f, frames)):
                failed.append((b, f"call {c + 1} differs from call 1", float((p - pred).abs().max())))
        for k in range(B, b):                                  # position k holds the frame of position k % 8
            j = k % B
            if not (torch.equal(pred[k], pred[j]) and torch.equal(frames[k], frames[j]) and torch.equal(vframes[k], vframes[j])):
                failed.append((b, f"copies at positions {j} and {k} differ", float((pred[k] - pred[j]).abs().max())))
                break
    for b in (64, 8):
        idx = _grid_order(b)
        pred, frames = _step(unet, vae, o["lat"][idx].cuda(), o["aud"][idx].cuda())
        if not (torch.equal(pred.cpu(), first[b][0]) and torch.equal(frames.cpu(), first[b][1])):
            failed.append((b, "after the sweep, differs from its first result"))
    assert not failed, failed


@pytest.fixture(scope="module")
def hip_full_bf16(lib_built, full_sd):
    from mere_fusion_amd.musetalk.models.unet import UNet
    from mere_fusion_amd.musetalk.models.vae import VAE
    usd, vsd = full_sd
    return (UNet(unet_config_json(MUSETALK_V1["unet"]), usd, precision="bf16", max_batch=B),
            VAE(config=vae_config_json(MUSETALK_V1["vae"]), precision="bf16", state_dict=vsd, max_batch=B))


@pytest.mark.parametrize("b", grid_batches("musetalk", "bf16"))
def test_full_bf16_at_its_grid_batches_vs_oracle(hip_full, hip_full_bf16, oracle_full, b):
    """The single-pass bf16 mode at the batch sizes of its rows in the tuning table, on handles built for 8 frames: gated against the oracle, at least 10 x the
    bf16x3 handles' error at the same batch (the mode switch is real), and the step bit-identical through eager, capture and replay."""
    o = oracle_full
    idx = _grid_order(b)
    lat, aud = o["lat"][idx].cuda(), o["aud"][idx].cuda()
    errs, same = {}, {}
    for prec, (unet, vae) in (("bf16x3", hip_full), ("bf16", hip_full_bf16)):
        calls = [tuple(t.clone() for t in _step(unet, vae, lat, aud)) for _ in range(3)]          # eager, capture, replay
        same[prec] = all(torch.equal(p, calls[0][0]) and torch.equal(f, calls[0][1]) for p, f in calls[1:])
        lerr = (calls[0][0].cpu() - o["pred"][idx]).abs().max().item()
        _, ierr, u8max, u8frac = _vae_vs_oracle(vae, o, idx)
        errs[prec] = (lerr, ierr, u8max, u8frac)
        print(f"MuseTalk {prec}, batch {b} (8-frame handles): latents L-inf {lerr:.3e}, image L-inf {ierr:.3e}, "
              f"uint8 max diff {u8max}, differing pixels {100 * u8frac:.3f} %")
    assert all(same.values()), same
    lerr, ierr, u8max, _ = errs["bf16"]
    assert lerr <= TOL_BF16_LATENT and ierr <= TOL_BF16_IMAGE and u8max <= TOL_BF16_U8, errs["bf16"]
    assert lerr >= 10 * errs["bf16x3"][0] and ierr >= 10 * errs["bf16x3"][1], errs
