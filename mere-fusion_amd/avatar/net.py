"""Python face of the mf_net_* builder (include/merefusion.h): buffers are ids, every op is appended in execution order."""
import ctypes as C

import numpy as np
import torch

from .. import _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pair(v):
    """torch's int-or-(h, w) convention"""
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class Net:
    def __init__(self, max_batch=1, precision="bf16x3", device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("the avatar-preparation networks need a HIP device; no CPU path exists here")
        self.device = torch.device(device)
        _lib.init_device(self.device.index if self.device.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_create(int(max_batch), _lib.PRECISIONS[precision], C.byref(h)), "net_create")
        self._h, self.max_batch, self.shape, self._keep = h.value, max_batch, {}, []

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().mf_net_destroy(self._h)
        except Exception:
            pass

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def buffer(self, Cn, H, W, halo=1):
        with torch.cuda.device(self.device):
            i = _lib.lib().mf_net_buffer(self._h, int(Cn), int(H), int(W), int(halo))
        if i < 0:
            _lib.check(i, "net_buffer")
        self.shape[i] = (Cn, H, W)
        return i

    def _f32(self, t):
        if t is None:
            return None
        t = torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous()
        self._keep.append(t)
        return t

    def conv(self, weight, in_buf, out_buf, stride=1, pad=0, act=0, bias=None, bn=None, in_coff=0, out_coff=0, res_buf=-1, res_coff=0, name="conv", res_after_act=False):
        """nn.Conv2d(cin, cout, k, stride, pad) [+ BatchNorm2d (gamma, beta, mean, var)] [+ residual] + act (0 none, 1 ReLU, 2 sigmoid, 4 SiLU); stride and pad are
        one int or an (h, w) pair as in torch; the residual is added before the activation, or after it with res_after_act (mf_conv2d_desc.residual = 2)"""
        w = self._f32(weight)
        cout, cin, kh, kw = w.shape
        (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
        d = _lib.MfConv2dDesc(cin=cin, cout=cout, kh=kh, kw=kw, stride_h=sh, stride_w=sw, pad_h=ph, pad_w=pw, act=act,
                              residual=(2 if res_after_act else 1) if res_buf >= 0 else 0)
        b = self._f32(bias)
        g, be, m, v = (self._f32(t) for t in bn) if bn is not None else (None, None, None, None)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_conv(self._h, C.byref(d), _p(w), _p(b), _p(g), _p(be), _p(m), _p(v), in_buf, in_coff, out_buf, out_coff,
                                              res_buf, res_coff, name.encode()), f"net_conv({name})")

    def dwconv(self, weight, in_buf, out_buf, stride=1, act=0, bias=None, bn=None, bn_eps=1e-5, in_coff=0, out_coff=0):
        """nn.Conv2d(C, C, k, stride, k // 2, groups=C) [+ BatchNorm2d] + act (0 none, 1 ReLU, 4 SiLU); k 3 or 5, stride 1 or 2"""
        w = self._f32(weight)
        Cn, one, kh, kw = w.shape
        if one != 1 or kh != kw:
            raise ValueError(f"dwconv: a depthwise weight is [C, 1, k, k], got {tuple(w.shape)}")
        b = self._f32(bias)
        g, be, m, v = (self._f32(t) for t in bn) if bn is not None else (None, None, None, None)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_dwconv(self._h, Cn, kh, stride, act, _p(w), _p(b), _p(g), _p(be), _p(m), _p(v), C.c_float(bn_eps), in_buf, in_coff, out_buf,
                                                out_coff), "net_dwconv")

    def chan_attn(self, x_buf, Cn, pooled_buf, fc_weight, fc_bias, out_buf, x_coff=0, out_coff=0):
        """x * hardsigmoid(fc(pooled)): mmdet's ChannelAttention after its average pool (global_avgpool into pooled_buf)"""
        w, b = self._f32(torch.as_tensor(fc_weight).reshape(Cn, Cn)), self._f32(fc_bias)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_chan_attn(self._h, x_buf, x_coff, Cn, pooled_buf, _p(w), _p(b), out_buf, out_coff), "net_chan_attn")

    def maxpool(self, in_buf, out_buf, k, stride, pad=0):
        _lib.check(_lib.lib().mf_net_maxpool(self._h, in_buf, out_buf, k, stride, pad), "net_maxpool")

    def l2norm(self, in_buf, out_buf, weight, eps=1e-10):
        w = self._f32(weight)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_l2norm(self._h, in_buf, out_buf, _p(w), w.numel(), C.c_float(eps)), "net_l2norm")

    def global_avgpool(self, in_buf, Cn, out_buf, in_coff=0):
        _lib.check(_lib.lib().mf_net_global_avgpool(self._h, in_buf, in_coff, Cn, out_buf), "net_global_avgpool")

    def scale_add(self, x_buf, Cn, out_buf, s_buf=-1, t_buf=-1, v_buf=-1, x_coff=0, t_coff=0, out_coff=0):
        _lib.check(_lib.lib().mf_net_scale_add(self._h, x_buf, x_coff, Cn, s_buf, t_buf, t_coff, v_buf, out_buf, out_coff), "net_scale_add")

    def upsample_nearest(self, in_buf, out_buf):
        _lib.check(_lib.lib().mf_net_upsample_nearest(self._h, in_buf, out_buf), "net_upsample_nearest")

    # ---- execution -------------------------------------------------------------------------------------------------------------
    def set_input(self, buf, x):
        x = x.to(self.device, torch.float32).contiguous()
        B, Cn = x.shape[0], x.shape[1]
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_set_input(self._h, buf, _p(x), Cn, B, self._stream()), "net_set_input")
        return B

    def set_input_u8(self, buf, x, mean, reverse_channels=False):
        """uint8 device frames [B, H, W, 3] -> a 3-channel input buffer: channel c = frame[..., 2 - c if reverse_channels else c] - mean[c]"""
        x = x.to(self.device).contiguous()
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or tuple(x.shape[1:3]) != self.shape[buf][1:]:
            raise ValueError(f"set_input_u8: uint8 [B, {self.shape[buf][1]}, {self.shape[buf][2]}, 3] expected, got {x.dtype} {tuple(x.shape)}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_set_input_u8(self._h, buf, _p(x), (C.c_float * 3)(*[float(m) for m in mean]), int(bool(reverse_channels)), x.shape[0],
                                                      self._stream()), "net_set_input_u8")
        return x.shape[0]

    def set_input_u8_windows(self, buf, frames, starts, T, row0, rows):
        """uint8 device frames [n, H, W, 3] -> a 3 * T-channel input buffer, one launch: batch slot w = frames[starts[w] : starts[w] + T] concatenated on the
        channel axis, rows [row0, row0 + rows), / 255 (mf_net_set_input_u8_windows).  starts is a host list; the frames are read in place."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_cuda or not frames.is_contiguous():
            raise ValueError(f"set_input_u8_windows: contiguous uint8 device frames [n, H, W, 3] expected, got {frames.dtype} {tuple(frames.shape)} on {frames.device}")
        starts = [int(v) for v in starts]
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_set_input_u8_windows(self._h, buf, _p(frames), frames.shape[0], frames.shape[1], frames.shape[2], (C.c_int * max(len(starts), 1))(*starts),
                                                              len(starts), int(T), int(row0), int(rows), self._stream()), "net_set_input_u8_windows")
        return len(starts)

    def run(self, batch):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_run(self._h, batch, self._stream()), "net_run")

    def output(self, buf, Cn, batch, coff=0):
        _, H, W = self.shape[buf]
        out = torch.empty((batch, Cn, H, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_get_output(self._h, buf, coff, Cn, _p(out), batch, self._stream()), "net_get_output")
        return out

    def output_bilinear(self, buf, Cn, batch, H, W, coff=0):
        out = torch.empty((batch, Cn, H, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_net_get_output_bilinear(self._h, buf, coff, Cn, _p(out), H, W, batch, self._stream()), "net_get_output_bilinear")
        return out

    @property
    def gflop_per_item(self):
        return _lib.lib().mf_net_flops_per_item(self._h) / 1e9
