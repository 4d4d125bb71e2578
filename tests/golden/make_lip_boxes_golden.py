"""Generates tests/golden/lip_boxes_golden.npz from the REFERENCE's own `get_smoothened_boxes` (build container only).  wav2lip/genavatar.py cannot be imported (it
needs cv2 and parses sys.argv at import), so the one function is taken out of its source with `ast` and executed here; the pads / clamp statements of
genavatar.py:87-92 and the clip / int() of face_detection/api.py:69-78 are restated next to it.  Only inputs and outputs are stored.

Per case c: det_c fp32 [n, 5] (the detector's first box per frame, x1 y1 x2 y2 score), hw_c (H, W), pads_c (top, bottom, left, right), nosmooth_c, and the expected
coords_c int32 [n, 4] in the reference's (y1, y2, x1, x2) order (what genavatar.py:96 puts into coords.pkl).  T = 5 (genavatar.py:95).

Cases: n in {1, 2, 3, 4, 5, 6, 9, 23} with the default pads (n < T runs Python's negative-slice window); nosmooth; boxes touching all four frame edges; non-default
pads; a negative detector coordinate."""
import ast
import os

import numpy as np

REF = "/root/reference/wav2lip/genavatar.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lip_boxes_golden.npz")
T = 5
NS = (1, 2, 3, 4, 5, 6, 9, 23)


def reference_smoother():
    tree = ast.parse(open(REF).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_smoothened_boxes"]
    assert len(fn) == 1
    ns = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), REF, "exec"), ns)
    return ns["get_smoothened_boxes"]


def reference_coords(smooth, det, H, W, pads, nosmooth):
    pady1, pady2, padx1, padx2 = pads
    results = []
    for d in det:
        d = np.clip(d, 0, None)                                              # api.py:74
        rect = tuple(map(int, d[:-1]))                                       # api.py:76
        y1 = max(0, rect[1] - pady1)                                         # genavatar.py:87-90
        y2 = min(H, rect[3] + pady2)
        x1 = max(0, rect[0] - padx1)
        x2 = min(W, rect[2] + padx2)
        results.append([x1, y1, x2, y2])
    boxes = np.array(results)
    if not nosmooth:
        boxes = smooth(boxes, T=T)
    return np.array([(y1, y2, x1, x2) for (x1, y1, x2, y2) in boxes], dtype=np.int32)


def walk(rng, n, H, W):
    """a face drifting through the frame with jitter: fractional coordinates, so that clip / int() and the integer means all matter"""
    c = np.array([W * 0.45, H * 0.4]) + np.cumsum(rng.normal(0, 2.5, (n, 2)), axis=0)
    s = np.array([W * 0.22, H * 0.3]) + rng.normal(0, 1.5, (n, 2))
    det = np.concatenate([c - s / 2, c + s / 2, rng.uniform(0.6, 0.99, (n, 1))], axis=1)
    return det.astype(np.float32)


def cases():
    rng = np.random.default_rng(20)
    H, W = 72, 88
    out = [(f"n{n}", walk(rng, n, H, W), (H, W), (0, 10, 0, 0), False) for n in NS]
    out.append(("nosmooth", walk(rng, 7, H, W), (H, W), (0, 10, 0, 0), True))
    edges = walk(rng, 8, H, W)
    edges[0, :4] = (0.0, 0.0, 30.2, 40.7)                                    # top-left corner
    edges[1, :4] = (60.5, 50.5, 88.0, 72.0)                                  # bottom-right corner
    edges[2, :4] = (-3.5, 20.1, 91.2, 50.9)                                  # wider than the frame
    edges[3, :4] = (20.3, -6.0, 50.0, 80.5)                                  # taller than the frame
    out.append(("edges", edges, (H, W), (0, 10, 0, 0), False))
    out.append(("edges_nosmooth", edges.copy(), (H, W), (0, 10, 0, 0), True))
    out.append(("pads", walk(rng, 9, H, W), (H, W), (7, 3, 11, 5), False))
    out.append(("pads_large", walk(rng, 6, H, W), (H, W), (40, 40, 50, 50), False))
    neg = walk(rng, 6, H, W)
    neg[1, 0], neg[3, 1], neg[4, :2] = -12.75, -0.5, (-1.2, -7.9)
    out.append(("negative", neg, (H, W), (0, 10, 0, 0), False))
    out.append(("tall_frame", walk(rng, 11, 260, 200), (260, 200), (0, 10, 0, 0), False))
    return out


def main():
    smooth = reference_smoother()
    data = {"T": np.int32(T), "names": np.array([c[0] for c in cases()])}
    for name, det, hw, pads, nosmooth in cases():
        data[f"det_{name}"] = det
        data[f"hw_{name}"] = np.array(hw, dtype=np.int32)
        data[f"pads_{name}"] = np.array(pads, dtype=np.int32)
        data[f"nosmooth_{name}"] = np.bool_(nosmooth)
        data[f"coords_{name}"] = reference_coords(smooth, det, hw[0], hw[1], pads, nosmooth)
    # the contract the issue spells out: n = 4, T = 5 -> every box becomes the last one
    c4 = reference_coords(smooth, data["det_n4"], 72, 88, (0, 10, 0, 0), False)
    assert (c4 == reference_coords(smooth, data["det_n4"], 72, 88, (0, 10, 0, 0), True)[-1]).all()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(cases())} cases")


if __name__ == "__main__":
    main()
