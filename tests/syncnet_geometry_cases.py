"""The two conv geometries SyncNet_color's face encoder adds to the engine (wav2lip/models/syncnet.py:12,14), at the real layers' sizes, as descriptors for the
single-layer seam (test_conv_configs.Layer: seeded parameters with BatchNorm, inputs exact in the storage format, float64 reference, derived bound)."""

CASES = [
    # Conv2d(15, 32, kernel_size=(7, 7), stride=1, padding=3): 15 input channels, not a multiple of 8 (the buffer's 16th channel is zero)
    ("k7_s1_p3_cin15", dict(cin=15, cout=32, kh=7, kw=7, stride_h=1, stride_w=1, pad_h=3, pad_w=3, in_h=48, in_w=96, act=1, residual=0)),
    # Conv2d(32, 64, kernel_size=5, stride=(1, 2), padding=1): 48 x 96 -> 46 x 47
    ("k5_s12_p1", dict(cin=32, cout=64, kh=5, kw=5, stride_h=1, stride_w=2, pad_h=1, pad_w=1, in_h=48, in_w=96, act=1, residual=0)),
]
OUT_HW = {"k7_s1_p3_cin15": (48, 96), "k5_s12_p1": (46, 47)}
BATCHES = (1, 3)
