"""`SyncNet_color`, the lip-sync expert Wav2Lip's sync loss is defined by (wav2lip/models/syncnet.py:7-66), for inference on the MI355X.

Same surface as the reference class: the constructor's module tree carries the parameters under the reference's 217 state-dict keys
(`face_encoder.{i}.conv_block.{0|1}.*`, `audio_encoder.{i}.conv_block.{0|1}.*`), `load_state_dict` / `.to` / `.eval` are nn.Module's, and
`forward(audio_sequences [B,1,80,16], face_sequences [B,15,48,96])` returns `(audio_embedding, face_embedding)`, each [B,512] and L2-normalised.
No layer has a torch forward.  Each encoder is one chain of `Conv2d + eval BatchNorm (eps 1e-5) + residual-before-ReLU + ReLU` layers (conv.py:5-19) on the
static-graph builder of avatar/net.py, the way avatar/s3fd.py is built: one `Net` per encoder at `max_batch`, captured per batch size; a larger batch runs in
chunks of `max_batch`.  DESIGN.md's kernel table says which kernel each layer lands on.

This class is not exported from the drop-in (`dropin/wav2lip/models`): training, the sync loss and the discriminators stay the reference's.  It serves
sync_score.py, which feeds the face encoder straight from served uint8 frames (`embed_faces_u8`)."""
import os

import torch
from torch import nn
from torch.nn import functional as F

from ... import weights
from .generator import _Block

FACE_T, FACE_H, FACE_W, DIM = 5, 48, 96, 512


def _seq(specs):
    return nn.Sequential(*[_Block(ci, co, k) for ci, co, k, *_ in specs])


def _out_hw(h, w, k, stride, pad):
    (sh, sw) = (stride, stride) if isinstance(stride, int) else stride
    return (h + 2 * pad - k) // sh + 1, (w + 2 * pad - k) // sw + 1


class SyncNet_color(nn.Module):
    def __init__(self, precision=None, max_batch=16):
        super().__init__()
        self.face_encoder = _seq(weights.SYNCNET_FACE)
        self.audio_encoder = _seq(weights.SYNCNET_AUDIO)
        self.precision = precision or os.environ.get("MF_PRECISION", "bf16x3")
        if self.precision not in ("bf16", "bf16x3"):
            raise ValueError(f"precision must be 'bf16' or 'bf16x3', got {self.precision!r}")
        if not 1 <= int(max_batch) <= 256:
            raise ValueError(f"max_batch must be in [1, 256], got {max_batch}")
        self.max_batch = int(max_batch)
        self._graphs, self._graphs_device = None, None

    # ---- graph lifetime: any change to the parameters invalidates the packed weights ---------------------------------------------
    def _drop_graphs(self):
        self._graphs, self._graphs_device = None, None

    def load_state_dict(self, *a, **kw):
        self._drop_graphs()
        return super().load_state_dict(*a, **kw)

    def _apply(self, fn, *a, **kw):
        self._drop_graphs()
        return super()._apply(fn, *a, **kw)

    def _chain(self, device, prefix, specs, cin, h, w):
        """one encoder: buffer i + 1 holds layer i's output; a buffer's halo is the padding of the layer that reads it"""
        from ...avatar.net import Net       # (here: importing the avatar package at module load would pull every preparation network in)
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in getattr(self, prefix).state_dict().items()}
        n = Net(self.max_batch, self.precision, device)
        pads = [s[4] for s in specs] + [0]
        bufs = [n.buffer(cin, h, w, pads[0])]
        for i, (ci, co, k, stride, pad, res) in enumerate(specs):
            h, w = _out_hw(h, w, k, stride, pad)
            bufs.append(n.buffer(co, h, w, pads[i + 1]))
            p = f"{i}.conv_block."
            n.conv(sd[p + "0.weight"], bufs[i], bufs[i + 1], stride, pad, act=1, bias=sd[p + "0.bias"],
                   bn=(sd[p + "1.weight"], sd[p + "1.bias"], sd[p + "1.running_mean"], sd[p + "1.running_var"]), res_buf=bufs[i] if res else -1, name=f"{prefix}.{i}")
        if (h, w) != (1, 1):
            raise RuntimeError(f"SyncNet_color: {prefix} ends in a {h} x {w} map, not 1 x 1")
        return dict(net=n, bufs=bufs)

    def _ensure_graphs(self, device):
        if self._graphs is None or self._graphs_device != device:
            self._drop_graphs()
            self._graphs = dict(face_encoder=self._chain(device, "face_encoder", weights.SYNCNET_FACE, 3 * FACE_T, FACE_H, FACE_W),
                                audio_encoder=self._chain(device, "audio_encoder", weights.SYNCNET_AUDIO, 1, 80, 16))
            self._graphs_device = device
        return self._graphs

    def _check(self, what, *tensors):
        if self.training:
            raise RuntimeError("the MI355X SyncNet_color is inference-only: call .eval()")
        if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
            raise RuntimeError(f"SyncNet_color.{what} needs HIP device tensors (model.to('cuda')); no CPU path exists here")

    def _run(self, g, total, fill):
        """the chain over `total` items in chunks of max_batch: fill(net, input buffer, first item, count) sets the input; -> raw embeddings [total, 512]"""
        n, out = g["net"], []
        for b0 in range(0, total, self.max_batch):
            B = min(self.max_batch, total - b0)
            fill(n, g["bufs"][0], b0, B)
            n.run(B)
            out.append(n.output(g["bufs"][-1], DIM, B).reshape(B, DIM))
        return out[0] if len(out) == 1 else torch.cat(out)

    # ---- the raw (un-normalised) embeddings: what mf_sync_score takes ---------------------------------------------------------------
    def embed_audio(self, audio_sequences):
        self._check("embed_audio", audio_sequences)
        if audio_sequences.dim() != 4 or tuple(audio_sequences.shape[1:]) != (1, 80, 16) or audio_sequences.shape[0] < 1:
            raise ValueError(f"SyncNet_color: audio_sequences must be [B, 1, 80, 16], got {tuple(audio_sequences.shape)}")
        g = self._ensure_graphs(audio_sequences.device)["audio_encoder"]
        x = audio_sequences.float().contiguous()
        return self._run(g, x.shape[0], lambda n, buf, b0, B: n.set_input(buf, x[b0:b0 + B]))

    def embed_faces(self, face_sequences):
        self._check("embed_faces", face_sequences)
        if face_sequences.dim() != 4 or tuple(face_sequences.shape[1:]) != (3 * FACE_T, FACE_H, FACE_W) or face_sequences.shape[0] < 1:
            raise ValueError(f"SyncNet_color: face_sequences must be [B, {3 * FACE_T}, {FACE_H}, {FACE_W}], got {tuple(face_sequences.shape)}")
        g = self._ensure_graphs(face_sequences.device)["face_encoder"]
        x = face_sequences.float().contiguous()
        return self._run(g, x.shape[0], lambda n, buf, b0, B: n.set_input(buf, x[b0:b0 + B]))

    def embed_faces_u8(self, frames_u8, starts):
        """The face embeddings of the windows frames_u8[s : s + 5], s in starts, straight from served frames: uint8 BGR [N, 96, 96, 3] on the device, the lower half
        of 5 frames on the channel axis, / 255 -- one launch per chunk (mf_net_set_input_u8_windows), no float copy of the windows in between."""
        self._check("embed_faces_u8", frames_u8)
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (2 * FACE_H, FACE_W, 3):
            raise ValueError(f"SyncNet_color: frames must be uint8 [N, {2 * FACE_H}, {FACE_W}, 3], got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        starts = [int(s) for s in starts]
        if not starts:
            raise ValueError("SyncNet_color: no windows")
        g = self._ensure_graphs(frames_u8.device)["face_encoder"]
        x = frames_u8.contiguous()
        return self._run(g, len(starts), lambda n, buf, b0, B: n.set_input_u8_windows(buf, x, starts[b0:b0 + B], FACE_T, FACE_H, FACE_H))

    # ---- syncnet.py:55-66 --------------------------------------------------------------------------------------------------------------
    def forward(self, audio_sequences, face_sequences):
        self._check("forward", audio_sequences, face_sequences)
        face_embedding = self.embed_faces(face_sequences)
        audio_embedding = self.embed_audio(audio_sequences)
        return F.normalize(audio_embedding, p=2, dim=1), F.normalize(face_embedding, p=2, dim=1)

    def read_tap(self, name, batch):
        """Output of layer `name` ("face_encoder.3", "audio_encoder.0", ...) in the last run as fp32 NCHW (parity tests); with a chunked batch, of the last chunk."""
        prefix, i = name.rsplit(".", 1)
        g = self._graphs[prefix]
        specs = weights.SYNCNET_FACE if prefix == "face_encoder" else weights.SYNCNET_AUDIO
        return g["net"].output(g["bufs"][int(i) + 1], specs[int(i)][1], batch)
