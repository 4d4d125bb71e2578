"""GPU: the copy kernels that carry every serving step, one launch at a time and at their edges -- mf_nerf_feat_scatter and mf_nerf_feat_windows
(csrc/mf_nerf_featpool.hip) against the restatements of tests/nerf_featpool_ref.py, mf_gather_rows_f32 and mf_whisper_feature_chunks (csrc/mf_session.hip)
against indexing and the clamp `min(T - 1, max(0, left + j))`, and mf_windows_push (csrc/mf_window_push.hip) with a kept context above 64 KB -- the launch with
raised dynamic LDS -- against the torch route of tests/test_windows_push_gpu.py.

All five only move fp32 values, so every comparison is for equal bits (`torch.equal` / `np.array_equal` on the int32 view, which also tells a NaN that was
written from one that was left).  Every destination holds a sentinel before the call -- seeded noise in pools and histories, NaN in outputs -- and the WHOLE
buffers are compared afterwards: every element that had to be written was written, and every row, slot and byte that was not named kept its bits.  The
launch splits (64 sessions, 256 rows, 128 chunks) are crossed by 65 of 66 sessions, 257 and 600 rows, 129 chunks."""
import ctypes as C

import numpy as np
import pytest
import torch

from nerf_featpool_ref import emu_scatter, emu_windows
from test_windows_push_gpu import _torch_route

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want):
    """equal bits of two fp32 tensors, whole buffers"""
    return got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _noise(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# sessions of a call: (rows of the pool, pool size).  "65 of 66" is two launches (64 + 1) and leaves one row of the pool unnamed.
def _shuffled(N, n, seed):
    return [int(k) for k in torch.randperm(N, generator=torch.Generator().manual_seed(seed))][:n]


SESSIONS = {"1 session": ([2], 3), "3 sessions, not sorted": ([4, 0, 2], 5), "65 of 66, shuffled: two launches": (_shuffled(66, 65, 66), 66)}
assert sorted(SESSIONS["65 of 66, shuffled: two launches"][0]) != SESSIONS["65 of 66, shuffled: two launches"][0]


# ---- a. mf_nerf_feat_scatter ------------------------------------------------------------------------------------------------------------------------
def _scatter_ranges(R):
    """name -> (T, left, right)"""
    ranges = {"[0, T)": (7, 0, 7), "[T-1, T)": (7, 6, 7), "an inner range": (7, 2, 5)}
    if R == 16:
        ranges["16 rows: the range fills the ring"] = (18, 1, 17)
    return ranges


def _scatter_starts(name, S, R, n):
    if name == "0":
        return [0] * S
    if name == "the last legal start R - n":
        return [R - n] * S
    return [(5 * i + 1) % (R - n + 1) for i in range(S)]                  # "a different start per session"


@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("dim", [1, 29, 255, 256, 257, 1024])          # the copy loop strides by 256 threads
def test_feat_scatter_equals_the_model(lib_built, dim, R):
    from mere_fusion_amd import ops
    ran = []
    for sess, (rows, N) in SESSIONS.items():
        rings0 = _noise((N, R, dim), 1000 * R + dim + N)
        for rng, (T, left, right) in _scatter_ranges(R).items():
            feats = _noise((len(rows), T, dim), 7 * T + left + N)
            feats_dev = feats.cuda()
            for st in ("0", "the last legal start R - n", "a different start per session"):
                starts = _scatter_starts(st, len(rows), R, right - left)
                if st == "a different start per session" and len(rows) > 1 and right - left < R:
                    assert len(set(starts)) > 1
                want = rings0.clone()
                emu_scatter(feats, left, right, want, rows, starts)
                rings = rings0.cuda()
                ops.nerf_feat_scatter(feats_dev, left, right, rings, rows, starts)
                assert _same(rings, want), (sess, rng, st)
                assert not torch.equal(want, rings0)
                ran.append((sess, rng, st))
    assert len(ran) == 3 * 3 * (4 if R == 16 else 3)


# ---- b. mf_nerf_feat_windows ------------------------------------------------------------------------------------------------------------------------
def _fronts_of(R):
    """(fronts an older window takes, fronts a new window takes): R - 1 wraps by 15 rows; R - 16 fits exactly -- read from the ring as a new window, a COPY as
    an older one (first + 16 >= R); R - 17 is the last VIEW; 0; and -1, a zero window or history slot, on older windows only.  With R == 16 these fall
    together to {15, 0, -1} and every older window is a copy."""
    older = []
    for f in (R - 1, R - 16, R - 17, 0, -1):
        if f >= -1 and f not in older:
            older.append(f)
    return older, [f for f in older if f >= 0]


def _window_fronts(S, R, n_new, turn):
    """fronts [S][8] oldest first, taken in turn from _fronts_of(R) so that over the sessions and turns every front is used at new and at older positions"""
    older, new = _fronts_of(R)
    fronts = []
    for i in range(S):
        n_old = 8 - n_new[i]
        fronts.append([older[(q + i + turn) % len(older)] for q in range(n_old)] + [new[(j + i + turn) % len(new)] for j in range(n_new[i])])
    return fronts


def _windows_call(ops, rings0, hist0, rows, fronts, heads, n_new, att, what):
    """one launch from the sentinels against the model: `out`, the whole `hist`, and `rings` (unchanged)"""
    S, dim = len(rows), rings0.shape[2]
    want_hist = hist0.clone() if att else None
    want = emu_windows(rings0, want_hist, rows, fronts, heads, n_new, att, out=torch.full((S, 8 if att else 1, dim, 16), NAN))
    rings, hist = rings0.cuda(), hist0.cuda() if att else None
    out = torch.full((S, 8 if att else 1, dim, 16), NAN, device="cuda")
    assert ops.nerf_feat_windows(rings, hist, rows, fronts, heads, n_new, att, out=out) is out
    assert not torch.isnan(want).any(), what
    assert _same(out, want), what
    assert _same(rings, rings0), what
    if att:
        assert _same(hist, want_hist), what


N_NEW, HEADS = (1, 4, 8), (0, 5, 7)                                    # with 8 new windows there is no older one; heads 5 and 7 make new and older slots wrap modulo 8


@pytest.mark.parametrize("R", [16, 20, 32])
@pytest.mark.parametrize("dim", [1, 29, 63, 64, 65, 1024])             # a tile is 64 dims: part of one, one short of one, one, one and a 1-dim tile, sixteen
def test_feat_windows_equals_the_model(lib_built, dim, R):
    from mere_fusion_amd import ops
    older, new = _fronts_of(R)
    assert (older, new) == {16: ([15, 0, -1], [15, 0]), 20: ([19, 4, 3, 0, -1], [19, 4, 3, 0]), 32: ([31, 16, 15, 0, -1], [31, 16, 15, 0])}[R]
    as_new, as_older, ran = set(), set(), []
    for sess, (rows, N) in SESSIONS.items():
        S = len(rows)
        rings0, hist0 = _noise((N, R, dim), 100 * R + dim + N), _noise((N, 8, dim, 16), 200 * R + dim + N)
        if S <= 3:                                                       # every (new-window count, head), the same for all sessions of the launch
            calls = [(f"n_new {n}, head {h}", [n] * S, [h] * S, t) for t, (n, h) in enumerate((n, h) for n in N_NEW for h in HEADS)]
        else:                                                            # two launches: counts and heads differ from session to session, in three turns
            calls = [(f"n_new and heads mixed, turn {t}", [N_NEW[(i + t) % 3] for i in range(S)], [HEADS[(i // 3 + t) % 3] for i in range(S)], t) for t in range(3)]
            assert {calls[t][1][64] for t in range(3)} == set(N_NEW)     # the session of the second launch takes each count once
        for name, n_new, heads, turn in calls:
            fronts = _window_fronts(S, R, n_new, turn)
            for f, n in zip(fronts, n_new):
                as_older.update(f[:8 - n])
                as_new.update(f[8 - n:])
            _windows_call(ops, rings0, hist0, rows, fronts, heads, n_new, 2, (sess, name))
            ran.append((sess, name))
        # att = 0: one window per session, no history
        for turn in range(len(new)):
            fronts = [[new[(i + turn) % len(new)]] for i in range(S)]
            _windows_call(ops, rings0, None, rows, fronts, [0] * S, [1] * S, 0, (sess, "att = 0", turn))
    assert as_new == set(new) and as_older == set(older) and len(ran) == 9 + 9 + 3


@pytest.mark.parametrize("R", [16, 20, 32])
@pytest.mark.parametrize("dim", [29, 65])
def test_feat_windows_twice_with_a_scatter_in_between(lib_built, dim, R):
    """A session's first call (four new windows beside four zero windows) and its next (one new window), with net rows scattered into the rings in between: the
    second call reads, as older copies, history slots the first one wrote, and its views show the rewritten ring rows -- the copies do not."""
    from mere_fusion_amd import ops
    rows, N = SESSIONS["3 sessions, not sorted"]
    S = len(rows)
    rings_m, hist_m = _noise((N, R, dim), 31 * R + dim), _noise((N, 8, dim, 16), 37 * R + dim)
    rings, hist = rings_m.cuda(), hist_m.cuda()
    first4 = [R - 1, R - 16, max(R - 17, 0), 0]                           # afterwards: a copy, a copy, a view (R > 16), a view (R > 16)
    fronts1 = [[-1] * 4 + first4[i:] + first4[:i] for i in range(S)]
    feats = _noise((S, 9, dim), 41 * R + dim)
    starts = [0, R - 8, (R - 8) // 2]
    fronts2 = [f[1:] + [(3 * i + 1) % R] for i, f in enumerate(fronts1)]
    steps = (("the first call", fronts1, [0] * S, [4] * S), ("the second call", fronts2, [4] * S, [1] * S))
    for what, fronts, heads, n_new in steps:
        want = emu_windows(rings_m, hist_m, rows, fronts, heads, n_new, 2, out=torch.full((S, 8, dim, 16), NAN))
        out = torch.full((S, 8, dim, 16), NAN, device="cuda")
        ops.nerf_feat_windows(rings, hist, rows, fronts, heads, n_new, 2, out=out)
        assert _same(out, want) and _same(hist, hist_m) and _same(rings, rings_m), what
        if what == "the first call":
            first_out = want.clone()
            emu_scatter(feats, 1, 9, rings_m, rows, starts)
            ops.nerf_feat_scatter(feats.cuda(), 1, 9, rings, rows, starts)
            assert _same(rings, rings_m)
    # what the second call was to show, on the model it was held to: older windows 3..6 are the first call's new ones, out of the slots it wrote where they are
    # copies, and at least one view differs from what the first call returned (the ring rows under it were rewritten)
    copies = [(i, q) for i in range(S) for q in range(3, 7) if fronts2[i][q] + 16 >= R]
    views = [(i, q) for i in range(S) for q in range(3, 7) if fronts2[i][q] + 16 < R]
    assert copies and all(torch.equal(want[i, q], first_out[i, q + 1]) for i, q in copies)
    assert (R == 16) == (not views) and (not views or any(not torch.equal(want[i, q], first_out[i, q + 1]) for i, q in views))


# ---- c. mf_gather_rows_f32 --------------------------------------------------------------------------------------------------------------------------
POOL_ROWS = 5                                                           # fewer than any n but 1: rows repeat, as mirror indices do


def _gather(l, pool, rows, out, n=None, n_pool_rows=POOL_ROWS, row_elems=None):
    rc = l.mf_gather_rows_f32(pool.data_ptr(), n_pool_rows, pool.shape[1] if row_elems is None else row_elems, (C.c_int * max(len(rows), 1))(*rows),
                              len(rows) if n is None else n, out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n", [1, 256, 257, 600])                       # 256 rows per launch: one, a full one, a full one and 1, two full ones and 88
@pytest.mark.parametrize("row_elems", [4, 1020, 1024, 1028, 8192])      # a block moves 1024 floats: a row far shorter, 4 short, equal, 4 over, eight blocks
def test_gather_rows_equals_indexing(lib_built, row_elems, n):
    from mere_fusion_amd import _lib
    pool = _noise((POOL_ROWS, row_elems), 10 * row_elems + n)
    base = torch.randint(0, POOL_ROWS, (256,), generator=torch.Generator().manual_seed(n)).tolist()
    rows = [(base[i % 256] + i // 256) % POOL_ROWS for i in range(n)]   # entry i of every launch names another row than entry i of the launch before
    assert n == 1 or len(set(rows)) == POOL_ROWS
    want = torch.full((n + 1, row_elems), NAN)                          # one row longer than n: the last row keeps the sentinel
    want[:n] = pool[rows]
    out = torch.full((n + 1, row_elems), NAN, device="cuda")
    pool_dev = pool.cuda()
    assert _gather(_lib.lib(), pool_dev, rows, out) == 0
    assert _same(out, want) and _same(pool_dev, pool)


def test_gather_rows_refuses_without_a_launch(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    pool = _noise((POOL_ROWS, 8), 3).cuda()
    out = torch.full((4, 8), NAN, device="cuda")
    for what, kw in (("row_elems 6", dict(rows=[0, 1], row_elems=6)), ("a row equal to n_pool_rows", dict(rows=[0, POOL_ROWS])), ("a row of -1", dict(rows=[2, -1, 0])),
                     ("n = 0", dict(rows=[], n=0))):
        assert _gather(l, pool, out=out, **kw) == -1 and b"gather_rows" in l.mf_last_error(), what
        assert torch.isnan(out).all(), what


# ---- d. mf_whisper_feature_chunks -------------------------------------------------------------------------------------------------------------------
def _left_rows(T, rpc, n):
    """First rows of n chunks, of four kinds: far below 0 (every row clamps to 0), straddling 0, straddling T - 1, and T + 50 (every row clamps to T - 1);
    the kind steps with the chunk and once more at the launch split, so that chunk 128 differs from chunk 0, and each kind comes at three offsets."""
    kinds = (-100, -(rpc // 2) - 1, T - 1 - rpc // 2 - 1, T + 50)
    return [kinds[(i + i // 128) % 4] + (i // 4) % 3 for i in range(n)]


def _chunks(l, feat, T, row_elems, left, rpc, out):
    rc = l.mf_whisper_feature_chunks(feat.data_ptr(), T, row_elems, (C.c_int * len(left))(*left), rpc, len(left), out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n_chunks", [1, 128, 129])                     # 128 chunks per launch
@pytest.mark.parametrize("rpc", [1, 10, 64])                            # rows per chunk; 64 is the most the entry point takes
@pytest.mark.parametrize("T", [1, 7, 52])
def test_feature_chunks_equal_the_clamp(lib_built, T, rpc, n_chunks):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    lefts = [[v] for v in _left_rows(T, rpc, 4)] if n_chunks == 1 else [_left_rows(T, rpc, n_chunks)]     # a single chunk: once of each kind
    if n_chunks > 1:
        assert lefts[0][0] < -64 and lefts[0][3] >= T + 50 and (n_chunks <= 128 or lefts[0][128] != lefts[0][0])
        assert T == 1 or rpc == 1 or (lefts[0][1] < 0 < lefts[0][1] + rpc - 1 and lefts[0][2] < T - 1 < lefts[0][2] + rpc - 1)       # the two that straddle
    for row_elems in (4, 1028, 1920):                                    # a block moves 1024 floats: far shorter, one block and 4 floats, the (4 + 1) x 384 of a feature row
        feat = np.random.default_rng(1000 * T + row_elems).standard_normal((T, row_elems)).astype(np.float32)
        feat_dev = torch.from_numpy(feat).cuda()
        for left in lefts:
            n = len(left)
            r = np.minimum(T - 1, np.maximum(0, np.asarray(left)[:, None] + np.arange(rpc)[None, :]))       # min(T - 1, max(0, left + j))
            want = np.full((n + 1, rpc, row_elems), np.nan, np.float32)  # one chunk longer than needed: it keeps the sentinel
            want[:n] = feat[r]
            out = torch.full((n + 1, rpc, row_elems), NAN, device="cuda")
            assert _chunks(l, feat_dev, T, row_elems, left, rpc, out) == 0
            assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), (row_elems, left[:4])
        assert np.array_equal(feat_dev.cpu().numpy().view(np.int32), feat.view(np.int32))


def test_feature_chunks_refuse_without_a_launch(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    feat = _noise((7, 8), 5).cuda()
    out = torch.full((2, 65, 8), NAN, device="cuda")
    for what, rpc, row_elems in (("rows_per_chunk 65", 65, 8), ("row_elems 6", 10, 6)):
        assert _chunks(l, feat, 7, row_elems, [0, 3], rpc, out) == -1 and b"whisper_feature_chunks" in l.mf_last_error(), what
        assert torch.isnan(out).all(), what


# ---- e. mf_windows_push above 64 KB of kept context --------------------------------------------------------------------------------------------------
CONTEXTS = {"16384 floats: exactly 64 KB, the default path": 16384, "16388 floats: above 64 KB": 16388,
            "16385 floats: off the 16-byte grid, the scalar copy": 16385, "40960 floats: the 160 KiB the entry point accepts": 40960}


@pytest.mark.parametrize("n_new", [4, 10240])
@pytest.mark.parametrize("context", list(CONTEXTS))
def test_windows_push_with_a_large_context(lib_built, context, n_new):
    """A pool of 3 rows, rows 2 and 0 pushed and pushed again (the second push moves what the first wrote), against the torch route; the row between them keeps
    its bits.  Above 64 KB the entry point raises the kernel's dynamic-LDS limit before the launch; one small push at the defaults afterwards still matches."""
    from mere_fusion_amd import ops
    ctx = CONTEXTS[context]
    n, rows = ctx + n_new, [2, 0]
    assert (ctx * 4 > 64 * 1024) == (ctx > 16384) and ctx * 4 <= 160 * 1024
    buf = _noise((3, n), ctx + n_new).cuda()
    for push in (1, 2):
        new = _noise((2, n_new), ctx + push).cuda()
        want_buf, want_win = _torch_route(buf, rows, new)
        win = torch.full((2, n), NAN, device="cuda")
        assert ops.windows_push(buf, rows, new, out=win) is win
        assert _same(win, want_win) and _same(buf, want_buf), push
    small, new = _noise((3, 7040), 9).cuda(), _noise((2, 640), 10).cuda()  # the defaults: a context of 6400 floats, 640 new samples
    want_buf, want_win = _torch_route(small, rows, new)
    win = torch.full((2, 7040), NAN, device="cuda")
    ops.windows_push(small, rows, new, out=win)
    assert _same(win, want_win) and _same(small, want_buf)
