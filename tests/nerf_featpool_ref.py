"""The three launches of the ER-NeRF feature pool (csrc/mf_nerf_featpool.hip), restated from include/merefusion.h on host tensors.  One model for both tiers:
the host tier (tests/test_nerf_serving_host.py, tests/test_nerf_session_lifecycle_host.py) puts these in the launches' place and holds `NerfFeaturePool` against
`NerfASRFrontend` through them; the GPU tier (tests/test_serving_moves_gpu.py) holds the launches themselves against them, bit for bit."""
import torch


def emu_scatter(feats, left, right, rings, rows, starts):
    for i, (k, st) in enumerate(zip(rows, starts)):
        assert 0 <= st and st + right - left <= rings.shape[1]
        rings[k, st:st + right - left] = feats[i, left:right]


def emu_windows(rings, hist, rows, fronts, heads, n_new, att, out=None):
    N, R, dim = rings.shape
    o = torch.full((len(rows), 8 if att else 1, dim, 16), float("nan")) if out is None else out
    n_out = 8 if att else 1
    for i, k in enumerate(rows):
        assert len(fronts[i]) == n_out
        for q, f in enumerate(fronts[i]):
            j = q - (n_out - n_new[i])
            if j >= 0 or (f >= 0 and f + 16 < R):                        # a new window, or a view of the ring
                o[i, q] = rings[k, [(f + t) % R for t in range(16)]].t()
                if att and j >= 0:
                    hist[k, (heads[i] + j) % 8] = o[i, q]
            else:                                                        # a copy (it wrapped), or a zero window
                o[i, q] = hist[k, (heads[i] + n_new[i] + q) % 8]
    return o


def emu_rows_load(rings, hist, rows, src_ring=None, src_hist=None):
    rows = list(rows)
    assert rows and len(set(rows)) == len(rows) and 0 <= min(rows) and max(rows) < rings.shape[0]
    assert hist is not None or src_hist is None
    for t, src in ((rings, src_ring), (hist, src_hist)):
        if t is None:
            continue
        if src is not None:                                              # a source may be another row of the pool, never a named one
            assert tuple(src.shape) == tuple(t.shape[1:]) and all(src.data_ptr() != t[k].data_ptr() for k in rows)
        value = torch.zeros_like(t[0]) if src is None else src.clone()
        for k in rows:
            t[k] = value
