"""float64 references and error bounds of the ER-NeRF networks: the radiance field, the torso branch and the audio encoder (test_ernerf_net_configs.py).

- field64, torso64, audio64: the structure of oracle/ernerf_net_ref.py (`field_forward`, `run_torso`, `encode_audio`) with every Linear, convolution, sigmoid,
  exp, softmax and norm in float64.  The grid, SH and frequency encoders stay the fp32 C restatements of oracle/ernerf_ref.c: the HIP encoders are tested
  bit for bit against those elsewhere (test_ernerf.py), so what is compared here is the arithmetic BEHIND the encoders.  test_ernerf_net_configs.py pins the
  three to the fp32 oracle on the CPU.
- magnitudes: beside each value the references carry mag = the value's first-order sensitivity to a RELATIVE perturbation of what feeds it, in the form
  nn_numerics.py uses for one layer -- sum_k |w_k| |x_k| -- pushed through the layers behind it (|W_n| ... |W_1| |x|; ReLU is 1-Lipschitz and keeps zero, a
  sigmoid is 1/4-Lipschitz).  An operand stored to u relative (REPR: 2^-16 for a (hi, lo) bf16 pair, 2^-8 for one bf16 plane) moves a result by at most u * mag to
  first order; the stress tests gate at K * u * mag + the fp32 rounding of the result, K measured on an MI355X (3 x the worst first measurement, written beside each
  gate).  On benign inputs the fixed gates of test_ernerf.py apply instead.
"""
from types import SimpleNamespace

import numpy as np
import torch

from nn_numerics import REPR
from oracle import ernerf_net_ref as NR

F32 = 2.0 ** -24
LN2_F32 = float(np.float32(np.log(2.0)))


def mlp64(sd, name, x, mag=None):
    """`MLP.forward` (bias-free Linears, ReLU between) in float64 -> (y, mag_y): mag_y = |W_n| ... |W_1| mag (mag = |x| by default)"""
    x = x.double()
    mag = x.abs() if mag is None else mag.double()
    n = sum(1 for k in sd if k.startswith(name + ".net.") and k.endswith(".weight"))
    for l in range(n):
        w = sd[f"{name}.net.{l}.weight"].double()
        x, mag = x @ w.t(), mag @ w.abs().t()
        if l != n - 1:
            x = torch.relu(x)
    return x, mag


def field64(sd, x, d, enc_a, c, e, offsets, S, bound=1.0, H=64):
    """`NeRFNetwork.forward` in test mode.  x, d [M, 3]; enc_a [1, 32]; c [1, ind] or None (individual_dim 0); e [1, 1] or None (exp_eye off).
    Returns sigma [M], log_sigma [M], color [M, 3], amb_aud [M, 1], amb_eye [M, 1], unc [M, 1] (float64) and mag_* of log_sigma, the colour net's
    pre-sigmoid output, the attention vector's norm and eye_att_net's pre-sigmoid output."""
    xn = x.numpy().astype(np.float32)
    planes = (xn[:, :2], xn[:, 1:], np.concatenate([xn[:, :1], xn[:, -1:]], -1))      # split_xyz
    feats = []
    for name, pl in zip(("xy", "yz", "xz"), planes):
        x01 = ((pl + np.float32(bound)) / np.float32(2 * bound)).astype(np.float32)   # grid.py:144, in the reference's fp32
        feats.append(NR.grid_encode(x01, sd[f"encoder_{name}.embeddings"].numpy(), offsets, S, H))
    enc_x = torch.from_numpy(np.concatenate(feats, -1)).double()
    M = enc_x.shape[0]
    att, m_att = mlp64(sd, "aud_ch_att_net", enc_x)
    ea = enc_a.double().reshape(1, -1)
    parts, mags = [enc_x, ea * att], [enc_x.abs(), ea.abs() * m_att]
    if e is not None:
        eye_pre, m_eye = mlp64(sd, "eye_att_net", enc_x)
        eye_att = torch.sigmoid(eye_pre)
        ev = e.double().reshape(1, 1)
        parts.append(ev * eye_att); mags.append(ev.abs() * (eye_att + 0.25 * m_eye))
    else:
        eye_att, m_eye = torch.zeros(M, 1, dtype=torch.float64), torch.zeros(M, 1, dtype=torch.float64)
    h, m_h = mlp64(sd, "sigma_net", torch.cat(parts, -1), torch.cat(mags, -1))
    enc_d = torch.from_numpy(NR.sh_encode(d.numpy())).double()
    cin, cmag = [enc_d, h[:, 1:]], [enc_d.abs(), m_h[:, 1:]]
    if c is not None:
        cv = c.double().reshape(1, -1).repeat(M, 1)
        cin.append(cv); cmag.append(cv.abs())
    col_pre, m_col = mlp64(sd, "color_net", torch.cat(cin, -1), torch.cat(cmag, -1))
    return SimpleNamespace(sigma=torch.exp(h[:, 0]), log_sigma=h[:, 0], color=torch.sigmoid(col_pre) * (1 + 2 * 0.001) - 0.001,
                           amb_aud=att.norm(dim=-1, keepdim=True), amb_eye=eye_att, unc=torch.full((M, 1), LN2_F32, dtype=torch.float64),
                           mag_log_sigma=m_h[:, 0], mag_color=m_col, mag_aud=m_att.norm(dim=-1, keepdim=True), mag_eye=m_eye)


def field_bounds(w, prec, K):
    """per-element |got - want| allowed on stress inputs -> dict over log_sigma, color, amb_aud, amb_eye: K[name] * REPR * mag (through the output's own
    Lipschitz constant) + the fp32 rounding of the result"""
    u = REPR[prec]
    return {"log_sigma": K["log_sigma"] * u * w.mag_log_sigma + 4 * F32 * w.log_sigma.abs() + 4 * F32,
            "color": K["color"] * u * 0.25 * 1.002 * w.mag_color + 8 * F32,
            "amb_aud": K["amb_aud"] * u * w.mag_aud + 4 * F32 * w.amb_aud,
            "amb_eye": K["amb_eye"] * u * 0.25 * w.mag_eye + 8 * F32}


def grid_sample64(grid, xy):
    """F.grid_sample(grid [G, G], xy [N, 2], bilinear, zeros padding, align_corners=True) in float64 -> [N]"""
    G = grid.shape[0]
    return torch.nn.functional.grid_sample(grid.double().view(1, 1, G, G), xy.double().view(1, -1, 1, 2), align_corners=True).view(-1)


def torso64(sd, bg_coords, poses, bg_color, offsets, S, ind_code, torso_shrink=0.8, thresh=0.0, grid_size=128, H=16, warp_with=None):
    """`run_torso` + `forward_torso` over EVERY pixel (as the HIP path runs them), the occupancy mask applied at the end.  ind_code: [1, ind] or None.
    Returns float64 bg_color [N, 3], torso_alpha [N, 1] (masked), alpha_pre [N, 1] and deform [N, 2] (both before the mask), mask [N], occ [N].
    warp_with: a [N, 2] deform to warp by in place of this function's own (the returned deform stays its own).  The tiled grid's finest level has 2048 cells
    across the image, so a deform off by 1e-8 moves a grid feature by 2e-5: comparing two implementations BEHIND the grid to better than that needs one warp."""
    xy = torch.as_tensor(bg_coords, dtype=torch.float32).reshape(-1, 2)
    N = xy.shape[0]
    bg = torch.as_tensor(bg_color, dtype=torch.float64)
    bg = bg.expand(N, 3) if bg.dim() else bg
    occ = grid_sample64(sd["density_grid_torso"].view(grid_size, grid_size), xy)
    mask = occ > float(np.float32(thresh))
    x = xy * np.float32(torso_shrink)                                            # fp32, as the frequency encoder receives it (network.py:173)
    wa = sd["anchor_points"][None, ...] @ torch.as_tensor(poses, dtype=torch.float32).reshape(1, 4, 4).permute(0, 2, 1).inverse()
    wa = (wa[:, :, :2] / wa[:, :, 3, None] / wa[:, :, 2, None]).view(1, -1)
    enc_anchor = torch.from_numpy(NR.freq_encode(wa.numpy(), 3)).double()
    enc_x = torch.from_numpy(NR.freq_encode(x.numpy(), 8)).double()
    parts = [enc_x, enc_anchor.repeat(N, 1)] + ([ind_code.double().reshape(1, -1).repeat(N, 1)] if ind_code is not None else [])
    h = torch.cat(parts, -1)
    dx, _ = mlp64(sd, "torso_deform_net", h)
    x2 = (x.double() + (dx if warp_with is None else warp_with.double())).clamp(-1, 1).float().numpy()                          # the tiled grid reads fp32 coordinates
    g = torch.from_numpy(NR.grid_encode(((x2 + np.float32(1)) / np.float32(2)).astype(np.float32), sd["torso_encoder.embeddings"].numpy(), offsets, S, H,
                                        gridtype=1)).double()
    o, _ = mlp64(sd, "torso_net", torch.cat([g, h], -1))
    pre = torch.sigmoid(o) * (1 + 2 * 0.001) - 0.001
    alpha = torch.where(mask[:, None], pre[:, :1], torch.zeros(N, 1, dtype=torch.float64))
    color = torch.where(mask[:, None], pre[:, 1:], torch.zeros(N, 3, dtype=torch.float64))
    return {"bg_color": color * alpha + bg * (1 - alpha), "torso_alpha": alpha, "alpha_pre": pre[:, :1], "deform": dx, "mask": mask, "occ": occ}


def audio64(sd, a, att=2):
    """`NeRFNetwork.encode_audio` (AudioNet on every window, AudioAttNet over the 8) in float64 for any audio_in_dim: a [n, in_dim, 16] -> [1 or n, 32]"""
    F = torch.nn.functional
    p = lambda k: sd[k].double()
    x = a.double()[:, :, 8 - 8:8 + 8]
    for i in (0, 2, 4, 6):
        x = F.leaky_relu(F.conv1d(x, p(f"audio_net.encoder_conv.{i}.weight"), p(f"audio_net.encoder_conv.{i}.bias"), stride=2, padding=1), 0.02)
    x = x.squeeze(-1)
    x = F.leaky_relu(F.linear(x, p("audio_net.encoder_fc1.0.weight"), p("audio_net.encoder_fc1.0.bias")), 0.02)
    x = F.linear(x, p("audio_net.encoder_fc1.2.weight"), p("audio_net.encoder_fc1.2.bias"))
    if att <= 0:
        return x
    x = x.unsqueeze(0)
    y = x.permute(0, 2, 1)
    for i in (0, 2, 4, 6, 8):
        y = F.leaky_relu(F.conv1d(y, p(f"audio_att_net.attentionConvNet.{i}.weight"), p(f"audio_att_net.attentionConvNet.{i}.bias"), padding=1), 0.02)
    y = torch.softmax(F.linear(y.view(1, 8), p("audio_att_net.attentionNet.0.weight"), p("audio_att_net.attentionNet.0.bias")), dim=1).view(1, 8, 1)
    return torch.sum(y * x, dim=1)


def audio_template(in_dim):
    """zero tensors with the shapes of AudioNet(in_dim, 32) / AudioAttNet(32, 8) (network.py:9-66), for weights.make_ernerf_audio_state_dict"""
    t = {}
    for i, (cin, cout) in zip((0, 2, 4, 6), ((in_dim, 32), (32, 32), (32, 64), (64, 64))):
        t[f"audio_net.encoder_conv.{i}.weight"], t[f"audio_net.encoder_conv.{i}.bias"] = torch.zeros(cout, cin, 3), torch.zeros(cout)
    for i, (cin, cout) in zip((0, 2), ((64, 64), (64, 32))):
        t[f"audio_net.encoder_fc1.{i}.weight"], t[f"audio_net.encoder_fc1.{i}.bias"] = torch.zeros(cout, cin), torch.zeros(cout)
    for i, (cin, cout) in zip((0, 2, 4, 6, 8), ((32, 16), (16, 8), (8, 4), (4, 2), (2, 1))):
        t[f"audio_att_net.attentionConvNet.{i}.weight"], t[f"audio_att_net.attentionConvNet.{i}.bias"] = torch.zeros(cout, cin, 3), torch.zeros(cout)
    t["audio_att_net.attentionNet.0.weight"], t["audio_att_net.attentionNet.0.bias"] = torch.zeros(8, 8), torch.zeros(8)
    return t
