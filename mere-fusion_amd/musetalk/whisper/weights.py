"""The decoder half of a Whisper state dict: its key names (musetalk/whisper/whisper/model.py:174-187, 103-115) and seeded stand-ins.

No Whisper checkpoint ships with this repository; `make_decoder_state_dict` draws weights of the right shapes so that the arithmetic of
the device path can be tested.  They transcribe nothing."""
import numpy as np
import torch

# dims of the public "tiny" checkpoint (text half) and the reduced geometry the tests walk the kernels' edges with
WHISPER_TINY_TEXT = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=4)
WHISPER_SMALL_TEST = dict(n_vocab=257, n_text_ctx=80, n_text_state=128, n_text_head=2, n_text_layer=2)


def decoder_keys(n_layer):
    """{key: shape as a function of (n_vocab V, n_text_ctx T, n_state C)} under the names of `Whisper.state_dict()`"""
    keys = {"decoder.token_embedding.weight": lambda V, T, C: (V, C), "decoder.positional_embedding": lambda V, T, C: (T, C),
            "decoder.ln.weight": lambda V, T, C: (C,), "decoder.ln.bias": lambda V, T, C: (C,)}
    for i in range(n_layer):
        p = f"decoder.blocks.{i}."
        for att in ("attn", "cross_attn"):
            for lin in ("query", "key", "value", "out"):
                keys[p + f"{att}.{lin}.weight"] = lambda V, T, C: (C, C)
                if lin != "key":                                   # key = Linear(bias=False), model.py:62
                    keys[p + f"{att}.{lin}.bias"] = lambda V, T, C: (C,)
            keys[p + f"{att}_ln.weight"] = lambda V, T, C: (C,)
            keys[p + f"{att}_ln.bias"] = lambda V, T, C: (C,)
        keys[p + "mlp.0.weight"] = lambda V, T, C: (4 * C, C)
        keys[p + "mlp.0.bias"] = lambda V, T, C: (4 * C,)
        keys[p + "mlp.2.weight"] = lambda V, T, C: (C, 4 * C)
        keys[p + "mlp.2.bias"] = lambda V, T, C: (C,)
        keys[p + "mlp_ln.weight"] = lambda V, T, C: (C,)
        keys[p + "mlp_ln.bias"] = lambda V, T, C: (C,)
    return keys


def decoder_state_dict(state_dict, with_ln_post=True):
    """what `WhisperDecoder` takes out of a full checkpoint's `model_state_dict`: every "decoder.*" tensor, and the encoder's final LayerNorm
    (the encoder handle returns the last block's output without it)"""
    keep = {k: v for k, v in state_dict.items() if k.startswith("decoder.")}
    if with_ln_post:
        for k in ("encoder.ln_post.weight", "encoder.ln_post.bias"):
            if k in state_dict:
                keep[k] = state_dict[k]
    return keep


def make_decoder_state_dict(seed=0, dims=WHISPER_TINY_TEXT, emb_scale=0.1, timestamp_begin=None, timestamp_gain=1.0):
    """Seeded decoder weights under the checkpoint's key names.  The token embedding is kept small against what the blocks add to the residual
    stream: with tied weights a large embedding makes every step choose the token it was just fed, and a greedy run would test nothing.
    timestamp_gain scales the embedding rows >= timestamp_begin after they are drawn (the draws themselves do not move): with random weights
    either text or timestamps may win every step of a run under the timestamp rules, and the gain sets the balance between the two."""
    rng = np.random.default_rng(21000 + seed)
    V, T, C = dims["n_vocab"], dims["n_text_ctx"], dims["n_text_state"]
    sd = {}
    for k, shape in decoder_keys(dims["n_text_layer"]).items():
        s = shape(V, T, C)
        if k.endswith("token_embedding.weight"):
            a = rng.standard_normal(s) * emb_scale
            if timestamp_begin is not None:
                a[int(timestamp_begin):] *= timestamp_gain
        elif k.endswith("positional_embedding"):
            a = rng.standard_normal(s) * 0.3
        elif "ln.weight" in k:
            a = rng.uniform(0.8, 1.2, s)
        elif k.endswith(".bias"):
            a = rng.standard_normal(s) * 0.05
        else:
            gain = 1.5 if (".query." in k or ".key." in k or ".out." in k or "mlp.2" in k) else 1.0
            a = rng.standard_normal(s) * (gain / np.sqrt(s[1]))
        sd[k] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return sd
