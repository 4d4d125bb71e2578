"""What I420 delivery costs on the device (profiles/i420_delivery_timing.md): for an 8-frame 720 x 1280 block and an 8-frame 512 x 512 block, with hipEvents,

  1. mf_frames_to_i420 alone, on the 8-pixel strip path and on the 2 x 2 byte path (forced by a view one byte into a larger buffer), with the achieved GB/s
     over the 4.5 bytes per pixel the conversion has to move (3 in, 1.5 out);
  2. block -> FrameRing slots: the packed route (begin_batch: one D2H of 3 bytes per pixel, the code path of a default scheduler) against convert + copy as I420
     (one launch, one D2H of 1.5 bytes per pixel), alternating in the same loop.

5 warm-ups, then the median of 30 samples with min and max.  A sample of (1) is one replay of a graph of `--inner` launches between one event pair, divided by
their number: an eager call costs the host more than the kernel takes, and what is left per launch is the kernel plus the gap to the next one.  The kernel's
own duration comes from a kernel trace of a `--kernels-only` run, summarised by `--summarise`.  The host's saving (the consumer's colour conversion that no longer
runs) is not measured here: that needs libav.  Prints one JSON line.

    python tools/i420_timing.py [--frames 8] [--samples 30] [--warmup 5] [--inner 20]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o i420 -- python tools/i420_timing.py --kernels-only
    python tools/i420_timing.py --summarise DIR/.../i420_kernel_trace.csv
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT]

HBM_TBS = 6.29                  # measured float4 copy on MI355X (8.0 TB/s spec): what the achieved rate is set against


def stats(ms):
    return {"median_us": round(1e3 * float(np.median(ms)), 2), "min_us": round(1e3 * float(np.min(ms)), 2), "max_us": round(1e3 * float(np.max(ms)), 2)}


def timed(fn, inner=1):
    """device time of `inner` calls of fn between one event pair, per call, in ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def summarise(path, warmup):
    """the converter's own duration from a kernel trace (start to end of each dispatch, no launch gap in it), the first `warmup` dispatches of each row left out"""
    import csv
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "k_frames_to_i420" not in r["Kernel_Name"]:
                continue
            key = (r["Kernel_Name"], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    out = []
    for (name, grid), ms in sorted(rows.items()):
        ms = ms[warmup:] or ms
        out.append({"kernel": name, "grid_x": grid, "dispatches": len(ms), **stats(ms)})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true", help="only launch the converter (both paths, both sizes): the program to run under a kernel trace")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: median / min / max duration per (kernel, grid) of a kernel-trace CSV of a --kernels-only run")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.warmup)
    if not torch.cuda.is_available():
        raise SystemExit("i420_timing needs the GPU: a time taken anywhere else says nothing")
    from mere_fusion_amd import ops
    from mere_fusion_amd.transport import FrameRing, i420_shape
    B, out = a.frames, {"frames": a.frames, "samples": a.samples, "warmup": a.warmup, "inner": a.inner, "hbm_tb_s": HBM_TBS, "sizes": []}
    for H, W in ((720, 1280), (512, 512)):
        n = B * H * W * 3
        buf = torch.from_numpy(np.random.default_rng(H).integers(0, 256, n + 8, dtype=np.uint8)).cuda()
        aligned, shifted = buf[:n].view(B, H, W, 3), buf[1:1 + n].view(B, H, W, 3)
        planes = torch.empty((B,) + i420_shape(H, W), dtype=torch.uint8, device="cuda")
        assert aligned.data_ptr() % 4 == 0 and shifted.data_ptr() % 4 == 1
        row = {"H": H, "W": W, "bytes_moved": B * H * W * 9 // 2}
        # ---- 1. the converter alone, the two paths alternating
        t = {"vector": [], "scalar": []}
        if a.kernels_only:                                                   # for a kernel trace: nothing but the launches, each path `samples` times
            for name, src in (("vector", aligned), ("scalar", shifted)):
                for _ in range(a.warmup + a.samples):
                    ops.frames_to_i420(src, "bgr", out=planes)
            torch.cuda.synchronize()
            continue
        # `inner` launches captured into one graph per path: an eager call from Python costs the host about 10 us, more than the kernel takes
        graphs = {}
        for name, src in (("vector", aligned), ("scalar", shifted)):
            ops.frames_to_i420(src, "bgr", out=planes)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(a.inner):
                    ops.frames_to_i420(src, "bgr", out=planes)
        for i in range(a.warmup + a.samples):
            for name in ("vector", "scalar"):
                ms = timed(graphs[name].replay) / a.inner
                if i >= a.warmup:
                    t[name].append(ms)
        for name in t:
            row[name] = stats(t[name])
            row[name]["gb_s"] = round(row["bytes_moved"] / (np.median(t[name]) * 1e-3) / 1e9, 1)
            row[name]["share_of_hbm"] = round(row[name]["gb_s"] / (HBM_TBS * 1e3), 3)
        # ---- 2. block -> ring slots, packed against convert + copy, alternating; the slots go back after every sample (a rewind: nothing is published)
        rings = {"packed": FrameRing(B, (H, W, 3)), "i420": FrameRing(B, i420_shape(H, W))}
        idxs = list(range(B))

        def deliver(fmt):
            fr = aligned if fmt == "packed" else ops.frames_to_i420(aligned, "bgr")
            return rings[fmt].begin_batch(fr, idxs)

        t = {"packed": [], "i420": []}
        try:
            for i in range(a.warmup + a.samples):
                for fmt in ("packed", "i420"):
                    tok = []
                    ms = timed(lambda: tok.append(deliver(fmt)))
                    rings[fmt].abort_batch(tok[0])
                    if i >= a.warmup:
                        t[fmt].append(ms)
            want = ops.frames_to_i420(aligned, "bgr").cpu().numpy()                    # the slots hold the planes the converter gives
            tok = deliver("i420")
            torch.cuda.synchronize()
            got = np.stack([rings["i420"]._slot_view(s) for s in tok["slots"]])
            rings["i420"].abort_batch(tok)
            row["ring_i420_bytes_equal"] = bool(np.array_equal(got, want))
        finally:
            for r in rings.values():
                r.close()
        for fmt in t:
            row["ring_" + fmt] = stats(t[fmt])
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
