"""Plain NumPy models of S3FD's post-process (csrc/mf_s3fd_detect.hip) and seeded case builders for tests/test_s3fd_nms.py.

Written from the kernel file's comments and tests/golden/make_s3fd_detect_golden.py's docstring; tests/test_s3fd_nms.py anchors both models to the
recorded reference results of s3fd_detect_golden.npz before it uses them.

Rows.  A candidate row is (x1, y1, x2, y2, score, key) in float64, key = level << 28 | h << 14 | w as an integer value (float32 coordinates and scores
and a 31-bit key are all exact in float64).  `device_rows` turns the device's float32 rows (key = bit pattern of the sixth float) into that form.

A case is a dict: heads (12 float32 arrays [cls1, reg1, ..., cls6, reg6], cls [B, 2, h, w], reg [B, 4, h, w]), maps, and n_candidates[thresh] = the
expected candidate count per image at that candidate threshold."""
import numpy as np

LEVELS = 6
P_M = 1e-5                                   # the project's score margin (tests/golden/make_s3fd_detect_golden.py)
CAND_THRESH, NMS_THRESH, FINAL_THRESH = 0.05, 0.3, 0.5
COLD = (6.0, -6.0)                           # (bg, face) of a position that is no candidate: score 6e-6
DECODE_MAPS = [(9, 11), (5, 6), (3, 3), (2, 3), (1, 2), (1, 1)]
NMS_MAPS = [(56, 64), (16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]          # 4096 positions: the capacity of the NMS kernel's workgroup
TIE_MAPS = [(24, 32), (12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]
NMS_SIZES = [1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049, 4095, 4096]
NMS_PARTNER = {1: 129, 63: 1025, 64: 65, 65: 2049, 128: 1023, 129: 64, 1023: 4096, 1024: 63, 1025: 128, 2049: 1, 4095: 1024, 4096: 4095}
# seeds for which the float32 and the float64 NMS keep the same boxes (test_float32_and_float64_nms_agree checks every case)
NMS_SEED, TIE_SEED, DECODE_SEED, TAIL_SEED = 0, 0, 0, 0


def pack_key(level, h, w):
    return (np.asarray(level, np.int64) << 28) | (np.asarray(h, np.int64) << 14) | np.asarray(w, np.int64)


def unpack_key(key):
    key = np.asarray(key, np.int64)
    return key >> 28, (key >> 14) & 0x3fff, key & 0x3fff


def level_starts(maps):
    return np.concatenate([[0], np.cumsum([h * w for h, w in maps])])


def score64(bg, face):
    """float64 two-class softmax, face probability: exp(x - max) / sum"""
    bg, face = np.asarray(bg, np.float64), np.asarray(face, np.float64)
    with np.errstate(invalid="ignore"):
        m = np.maximum(bg, face)
        e0, e1 = np.exp(bg - m), np.exp(face - m)
        return e1 / (e0 + e1)


def candidates64(heads, cand_thresh):
    """-> (rows, mags): per image the float64 candidate rows sorted by key, and per row and coordinate the largest-magnitude intermediate of its chain
    (anchor centre, offset term, box centre, side, half side, both corners): the float32 chain's rounding errors are each at most half a spacing of one of
    these, so a few spacings of their maximum bound the coordinate's error, also where x1 cancels to something near 0."""
    B = heads[0].shape[0]
    rows, mags = [[] for _ in range(B)], [[] for _ in range(B)]
    for l in range(LEVELS):
        cls, reg = np.asarray(heads[2 * l]), np.asarray(heads[2 * l + 1])
        assert cls.dtype == np.float32 and reg.dtype == np.float32
        H, W = cls.shape[2:]
        stride = float(4 << l)
        anchor = 4.0 * stride
        score = score64(cls[:, 0], cls[:, 1])
        with np.errstate(invalid="ignore"):
            hot = score > cand_thresh                                            # a NaN score is no candidate
        for b in range(B):
            hh, ww = np.nonzero(hot[b])
            loc = reg[b][:, hh, ww].astype(np.float64)
            ac = np.stack([stride / 2 + ww * stride, stride / 2 + hh * stride])  # anchor centre (x, y)
            term = loc[0:2] * 0.1 * anchor
            c = ac + term
            side = anchor * np.exp(loc[2:4] * 0.2)
            lo = c - side / 2
            hi = side + lo
            rows[b].append(np.stack([lo[0], lo[1], hi[0], hi[1], score[b, hh, ww], pack_key(l, hh, ww).astype(np.float64)], 1))
            m = np.max(np.abs(np.stack([ac, term, c, side, lo, hi])), 0)         # [2, n]: x chain, y chain
            mags[b].append(np.stack([m[0], m[1], m[0], m[1]], 1))
    rows, mags = [np.concatenate(r) for r in rows], [np.concatenate(m) for m in mags]
    order = [np.argsort(r[:, 5], kind="stable") for r in rows]
    return [r[o] for r, o in zip(rows, order)], [m[o] for m, o in zip(mags, order)]


def device_rows(ws):
    """the device's candidate rows (float32 [n, 6], the key's bits in the sixth float) -> float64 rows with the key as a value"""
    ws = np.ascontiguousarray(ws, np.float32)
    out = ws.astype(np.float64)
    out[:, 5] = ws[:, 5].view(np.uint32)
    return out


def golden_rows(c):
    """a `*_cand*` array of s3fd_detect_golden.npz (x1, y1, x2, y2, score, level, h, w) -> float64 rows"""
    return np.concatenate([c[:, :5].astype(np.float64), pack_key(c[:, 5].astype(np.int64), c[:, 6].astype(np.int64), c[:, 7].astype(np.int64))[:, None].astype(np.float64)], 1)


def nms(rows, nms_thresh, final_thresh, dtype, info=None):
    """Greedy NMS in `dtype`: sort by (score descending, key ascending), visit in that order, a visited box that no kept box suppressed is kept and suppresses
    every later box it overlaps by more than nms_thresh; stops at the first unsuppressed score not above final_thresh.  Every operation is one NumPy operation
    of `dtype`, so float32 rounds where the kernel rounds.  -> the kept rows in keep order; `info` (a dict) receives the sorted order, the suppression flags
    by sorted position and the kept sorted positions."""
    rows = np.asarray(rows, np.float64).reshape(-1, 6)
    order = np.lexsort((rows[:, 5], -rows[:, 4]))
    s = rows[order]
    x1, y1, x2, y2, score = (s[:, i].astype(dtype) for i in range(5))
    assert all(np.array_equal(a.astype(np.float64), s[:, i]) for i, a in enumerate((x1, y1, x2, y2, score))), "the rows are not exact in dtype"
    one, zero, thr, fin = dtype(1), dtype(0), dtype(nms_thresh), dtype(final_thresh)
    area = (x2 - x1 + one) * (y2 - y1 + one)
    n = len(s)
    sup = np.zeros(n, bool)
    kept = []
    for i in range(n):
        if sup[i]:
            continue
        if not score[i] > fin:
            break
        kept.append(i)
        j = slice(i + 1, n)
        w = np.maximum(zero, np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j]) + one)
        h = np.maximum(zero, np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j]) + one)
        inter = w * h
        ovr = inter / (area[i] + area[j] - inter)
        sup[j] |= ovr > thr
    if info is not None:
        info.update(order=order, suppressed=sup, kept=np.array(kept, np.int64), sorted_rows=s)
    return s[kept]


def overlap64(a, b):
    """the NMS's overlap of two rows, float64"""
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1)
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    return w * h / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - w * h)


# ---- case builders ------------------------------------------------------------------------------------------------------------------------------------
def empty_heads(maps, B):
    heads = []
    for h, w in maps:
        cls = np.empty((B, 2, h, w), np.float32)
        cls[:, 0], cls[:, 1] = COLD
        heads += [cls, np.zeros((B, 4, h, w), np.float32)]
    return heads


def put(heads, maps, b, pos, bg, face, loc):
    """write positions `pos` (flat indices over the six levels, level-major, row-major within a level) of image b; bg, face [n], loc [n, 4]"""
    pos = np.atleast_1d(np.asarray(pos, np.int64))
    bg, face = np.broadcast_to(np.asarray(bg, np.float32), pos.shape), np.broadcast_to(np.asarray(face, np.float32), pos.shape)
    loc = np.broadcast_to(np.asarray(loc, np.float32), pos.shape + (4,))
    start = level_starts(maps)
    lv = np.searchsorted(start, pos, side="right") - 1
    for l in range(LEVELS):
        sel = lv == l
        q = pos[sel] - start[l]
        hh, ww = q // maps[l][1], q % maps[l][1]
        heads[2 * l][b, 0, hh, ww], heads[2 * l][b, 1, hh, ww] = bg[sel], face[sel]
        heads[2 * l + 1][b][:, hh, ww] = loc[sel].T


def flat(maps, level, h, w):
    return int(level_starts(maps)[level]) + h * maps[level][1] + w


def finish(heads, maps):
    """-> the case dict; asserts the score margin to both thresholds on every position (NaN logits aside) and counts the candidates"""
    B = heads[0].shape[0]
    counts = {CAND_THRESH: np.zeros(B, np.int64), FINAL_THRESH: np.zeros(B, np.int64)}
    for l in range(LEVELS):
        s = score64(heads[2 * l][:, 0], heads[2 * l][:, 1])
        ok = ~np.isnan(s)
        for t in counts:
            assert np.abs(s[ok] - t).min() > P_M, f"level {l + 1}: a score within {P_M} of {t}"
            counts[t] += (np.where(ok, s, 0.0).reshape(B, -1) > t).sum(1)
    return dict(heads=heads, maps=list(maps), n_candidates={t: [int(c) for c in v] for t, v in counts.items()})


def decode_case(seed=DECODE_SEED):
    """B = 2 on DECODE_MAPS: a candidate at the first and at the last position of every level and at about two thirds of the others, loc uniform in [-3, 3]
    with both signs on every component at the level ends, scores on both sides of 0.5, and one NaN face logit on an otherwise hot position per image."""
    rng = np.random.default_rng(seed)
    maps, B = DECODE_MAPS, 2
    heads = empty_heads(maps, B)
    start = level_starts(maps)
    ends = sorted({int(p) for l in range(LEVELS) for p in (start[l], start[l + 1] - 1)})
    nan_pos = []
    for b in range(B):
        others = np.setdiff1d(np.arange(start[-1]), ends)
        pos = np.concatenate([ends, rng.choice(others, 2 * len(others) // 3, replace=False)]).astype(np.int64)
        face = rng.uniform(-2.5, 6.0, len(pos))
        loc = rng.uniform(-3.0, 3.0, (len(pos), 4))
        loc[:len(ends)] = np.abs(loc[:len(ends)]) * np.where((np.arange(len(ends))[:, None] + np.arange(4)[None] + b) % 2, 1.0, -1.0)   # both signs, every component
        put(heads, maps, b, pos, 0.0, face, loc)
        p = int(pos[len(ends) + b])                                               # a hot position that is no level end
        nan_pos.append(p)
        put(heads, maps, b, p, 0.0, np.nan, loc[len(ends) + b])
    case = finish(heads, maps)
    case.update(ends=ends, nan_pos=nan_pos)
    return case


def nms_image(heads, maps, b, count, rng, lows):
    """`count` hot positions of image b spread over all levels (the last position of each level first, the rest drawn from all 4096), face logits in
    [0.2, 6] (score >= 0.55) except, with `lows`, every 32nd, which stays a candidate below 0.5, and loc that makes overlapping clumps: centres moved by up
    to 0.2 anchors, sides scaled by exp(+-0.3), so neighbours on the 4-px grid of level 1 overlap between nothing and 0.6"""
    start = level_starts(maps)
    forced = [int(start[l + 1] - 1) for l in range(LEVELS)][:count]
    rest = np.setdiff1d(np.arange(start[-1]), forced)
    pos = np.concatenate([forced, rng.choice(rest, count - len(forced), replace=False)]).astype(np.int64)
    face = rng.uniform(0.2, 6.0, count)
    low = (np.arange(count) % 32 == 31) & lows
    face[low] = rng.uniform(-2.5, -0.2, int(low.sum()))
    loc = np.concatenate([rng.uniform(-2.0, 2.0, (count, 2)), rng.uniform(-1.5, 1.5, (count, 2))], 1)
    put(heads, maps, b, pos, 0.0, face, loc)


def nms_case(count, seed=NMS_SEED):
    """B = 2 on NMS_MAPS: image 0 holds `count` candidates, all above 0.5, so the sorted list is walked to its last entry whatever `count` is; image 1 holds
    NMS_PARTNER[count] (a permutation: every size appears there too), one in 32 of them below 0.5, so its list is shorter when candidates are cut at 0.5"""
    rng = np.random.default_rng([seed, count])
    heads = empty_heads(NMS_MAPS, 2)
    for b, c in enumerate((count, NMS_PARTNER[count])):
        nms_image(heads, NMS_MAPS, b, c, rng, lows=b == 1)
    case = finish(heads, NMS_MAPS)
    assert case["n_candidates"][CAND_THRESH] == [count, NMS_PARTNER[count]] and case["n_candidates"][FINAL_THRESH][0] == count
    return case


def tie_case(seed=TIE_SEED):
    """B = 3 on TIE_MAPS.  Blocks of neighbouring positions share one (bg, face) pair, so their score bits are equal; neighbours one and two positions apart
    overlap by about 0.6 and 0.36 (equal squares of one anchor, shifted by a quarter and a half), three apart by 0.17, so which ones of a block survive is
    decided by the order among equal scores.  Two blocks of one image share their logits (they interleave in the output), one block's twin sits on the
    next level with the same boxes (the level bits of the key decide), and one block per image has face - bg = 40: its score is exactly 1.0f."""
    rng = np.random.default_rng(seed)
    maps, B = TIE_MAPS, 3
    heads = empty_heads(maps, B)

    def block(b, l, h0, w0, nh, nw, bg, face, grow=0.0):
        hh, ww = np.meshgrid(np.arange(h0, h0 + nh), np.arange(w0, w0 + nw), indexing="ij")
        pos = [flat(maps, l, int(h), int(w)) for h, w in zip(hh.ravel(), ww.ravel())]
        loc = np.concatenate([rng.uniform(-0.05, 0.05, (len(pos), 2)), grow + rng.uniform(-0.02, 0.02, (len(pos), 2))], 1)
        put(heads, maps, b, pos, bg, face, loc)

    for b in range(B):
        block(b, 0, 1 + b, 2, 1, 5 + b, 0.0, 2.0)                                  # a row of 5 / 6 / 7: ascending keeps 0, 3(, 6), descending keeps other ones
        block(b, 0, 8, 20 - b, 4, 5, 0.0, 2.0)                                     # same logits as the row above, elsewhere: the two interleave in key order
        block(b, 0, 16, 3, 5, 7, -20.0, 20.0)                                      # saturated: exp(-40) vanishes beside 1, the score is exactly 1.0f
        block(b, 1, 8, 2 + b, 3, 4, -20.0, 20.0)                                   # ... also on level 2, overlapping the block above
        # the same boxes from two levels: level 1 grown to level 2's anchor (exp(0.2 * ln(2) / 0.2) = 2), level 2 as it is, equal logits
        block(b, 0, 4, 24, 2, 2, 0.5, 3.5 - b, grow=float(np.log(2.0) / 0.2))
        block(b, 1, 2, 12, 1, 1, 0.5, 3.5 - b)
        block(b, 2, 3, 5, 2, 3, 1.0, 1.25)                                         # a tied block just above 0.5 (0.562), and one just below a candidate
        block(b, 3, 1, 1, 2, 2, 1.0, -0.5)
    return finish(heads, maps)


def chain_case():
    """Level 1, three equal squares of side 16 exp(1.0) = 43.5 px at shifts 0, 16 and 32 px with descending scores: A suppresses B (overlap 0.47), B overlaps C
    by the same, A overlaps C by 0.16.  Greedy NMS keeps A and C: B is gone before it can suppress anything."""
    maps = DECODE_MAPS
    heads = empty_heads(maps, 1)
    pos = [flat(maps, 0, 4, w) for w in (1, 5, 9)]
    put(heads, maps, 0, pos, 0.0, [4.0, 3.0, 2.0], [0.0, 0.0, 5.0, 5.0])
    case = finish(heads, maps)
    case["keys"] = [int(pack_key(0, 4, w)) for w in (1, 5, 9)]
    return case


TAIL_VARIANTS = {
    # name: (boxes above 0.5, sorted positions that duplicate entry 0 and are suppressed by it)
    "plain": (70, list(range(1, 11))),                                              # 64..69 live in the second mask word
    "word0_but_63": (70, list(range(1, 63))),                                       # the scan leaves entry 0 for bit 63 of its own word
    "word1_full": (140, list(range(1, 63)) + list(range(64, 128))),                 # ... and from 63 crosses a fully suppressed word to 128
}


def tail_case(variant, seed=TAIL_SEED):
    """B = 1 on NMS_MAPS, 1500 candidates of which only the first `top` in sorted order exceed 0.5 (face logit 6 - 0.03 rank).  Entry 0 is a level-2 box; the
    sorted positions in `dups` are other level-2 positions whose loc regresses onto entry 0's box (overlap ~ 1, suppressed); every other top entry is a
    level-1 anchor box on a 24-px grid that touches none of the others (kept).  The 1500 - top candidates below 0.5 lie anywhere and overlap anything."""
    rng = np.random.default_rng([seed, list(TAIL_VARIANTS).index(variant)])
    top, dups = TAIL_VARIANTS[variant]
    maps = NMS_MAPS
    heads = empty_heads(maps, 1)
    e0 = (1, 8, 12)                                                                 # entry 0: level 2, centre (100, 68), 32 x 32
    cx0, cy0 = 4 + 12 * 8.0, 4 + 8 * 8.0
    box0 = (cx0 - 16, cy0 - 16, cx0 + 16, cy0 + 16)
    l2 = [(h, w) for h in range(maps[1][0]) for w in range(maps[1][1]) if (h, w) != e0[1:]]
    l2 = [l2[i] for i in rng.permutation(len(l2))[:len(dups)]]
    iso = [(h, w) for h in range(3, maps[0][0], 6) for w in range(3, maps[0][1], 6)]
    iso = [(h, w) for h, w in iso if 2 + 4 * w + 10 < box0[0] or 2 + 4 * w - 10 > box0[2] or 2 + 4 * h + 10 < box0[1] or 2 + 4 * h - 10 > box0[3]]
    iso = [iso[i] for i in rng.permutation(len(iso))]
    used, it_iso, it_dup = [], iter(iso), iter(l2)
    for rank in range(top):
        face = 6.0 - 0.03 * rank
        if rank == 0:
            p, loc = flat(maps, *e0), np.zeros(4)
        elif rank in dups:
            h, w = next(it_dup)
            p = flat(maps, 1, h, w)
            loc = np.array([(cx0 - (4 + 8.0 * w)) / 3.2, (cy0 - (4 + 8.0 * h)) / 3.2, 0.0, 0.0]) + rng.uniform(-0.02, 0.02, 4)
        else:
            h, w = next(it_iso)
            p, loc = flat(maps, 0, h, w), np.concatenate([rng.uniform(-0.3, 0.3, 2), rng.uniform(-0.1, 0.0, 2)])
        put(heads, maps, 0, p, 0.0, face, loc)
        used.append(p)
    rest = np.setdiff1d(np.arange(level_starts(maps)[-1]), used)
    pos = rng.choice(rest, 1500 - top, replace=False)
    loc = np.concatenate([rng.uniform(-2.0, 2.0, (len(pos), 2)), rng.uniform(-1.5, 1.5, (len(pos), 2))], 1)
    put(heads, maps, 0, pos, 0.0, rng.uniform(-2.5, -0.2, len(pos)), loc)
    case = finish(heads, maps)
    assert case["n_candidates"] == {CAND_THRESH: [1500], FINAL_THRESH: [top]}
    case.update(top=top, dups=dups)
    return case
