"""The (network, precision, batches) grid of the tuning table shipped beside the library (tune/gfx950.txt).

tools/make_tune_cache.py measures every implicit-GEMM layer at these batch sizes; a forward at any other batch size runs the cost model's pick.
The parity tests sweep the same grid (tests/test_musetalk_full.py, tests/test_wav2lip_gpu.py) and tests/test_tune_table.py holds the shipped
table to it, so a batch size added here is measured, shipped and tested, or the CPU suite fails."""

# MuseTalk UNet + VAE: MuseBatcher steps of 8, 16, ... 64 frames (1 ... 8 sessions) and 1, 2, 3, 5 (tests / parity legs); the single-pass bf16
# mode at 1 and 8 for the `alt` legs of bench.py.  Wav2Lip: 1, 2, 5, 16 and the cross-session batch of 128, in both precisions.
GRID = {
    ("musetalk", "bf16x3"): (1, 2, 3, 5, 8, 16, 24, 32, 40, 48, 56, 64),
    ("musetalk", "bf16"): (1, 8),
    ("wav2lip", "bf16x3"): (1, 2, 5, 16, 128),
    ("wav2lip", "bf16"): (1, 2, 5, 16, 128),
}


def batches(network, precision):
    return GRID[(network, precision)]
