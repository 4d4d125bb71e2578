"""S3FD's device decode and NMS (csrc/mf_s3fd_detect.hip: k_s3fd_candidates, k_s3fd_nms) where tests/test_s3fd_detect.py does not reach: every candidate row
of every level, sorts of 64 .. 4096 entries, all four per-thread slots, all 64 words of the suppression mask, equal scores, and the planes path on its own.

The references are the NumPy models of tests/s3fd_ref.py.  The CPU tier first holds them to the reference's recorded results (s3fd_detect_golden.npz):
`candidates64` to the candidate rows, the float32 `nms` to the final boxes, bit for bit.  The GPU tier then reads the device's own candidate list back from the
workspace and asks that the kept boxes are bit-identical to the float32 model's greedy NMS of exactly those rows: the arithmetic is the same sequence of
separately rounded IEEE operations and a kept row is a copy of a candidate row, so no tolerance enters.  Every case is also run through the float64 model on
the CPU (same kept keys, same order): no decision of any case hangs on a float32 rounding.

Decode bound: 8 spacings of the largest float32 intermediate of the coordinate's chain (anchor centre, offset term, centre, side, corners).  Each float32
operation of the chain errs by at most half a spacing of its result and expf by 1-2, which sums to under 6; where nothing cancels this is the "8 ulp of the
coordinate" of tests/test_s3fd_detect.py, and it stays meaningful where x1 lands near 0.

Measured on an MI355X, printed by test_decode_every_row_every_level:
  200 rows over 6 levels (B = 2): max coordinate error 1.26 spacings of the chain's largest intermediate (bound 8), max score error 8.36e-8 (bound 1e-6)
  every other GPU test here is bit-exact: test_nms_matches_float32_model_on_device_candidates keeps 1 .. 600 boxes per image (584 .. 600 of 4095 / 4096)"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import s3fd_ref as R

CAP = 4096
TAILS = list(R.TAIL_VARIANTS)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3fd_detect_golden.npz"))


@functools.lru_cache(maxsize=None)
def case(kind, arg=None):
    """every case is built once and shared; nobody writes to it"""
    c = {"decode": R.decode_case, "nms": R.nms_case, "tie": R.tie_case, "chain": R.chain_case, "tail": R.tail_case}[kind](*(() if arg is None else (arg,)))
    for t in c["heads"]:
        t.setflags(write=False)
    return c


ALL_CASES = [("decode", None), ("tie", None), ("chain", None)] + [("tail", v) for v in TAILS] + [("nms", n) for n in R.NMS_SIZES]


def f32_rows(rows):
    """float64 model rows -> the same rows with float32 coordinates and scores (what a device list holds)"""
    out = rows.copy()
    out[:, :5] = rows[:, :5].astype(np.float32)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_candidates64_reproduces_the_golden_candidate_rows(golden, k):
    heads = [golden[f"P{k}_head{i}"] for i in range(12)]
    rows, mags = R.candidates64(heads, R.CAND_THRESH)
    for b in range(3):
        want = R.golden_rows(golden[f"P{k}_cand{b}"])
        want = want[np.argsort(want[:, 5])]
        assert np.array_equal(rows[b][:, 5], want[:, 5]), f"image {b}: the set of (level, h, w) differs"
        if len(want):
            assert np.abs(rows[b][:, 4] - want[:, 4]).max() <= 1e-6
            assert np.all(np.abs(rows[b][:, :4] - want[:, :4]) <= 8 * np.spacing(mags[b].astype(np.float32)).astype(np.float64))
    assert sum(len(r) for r in rows) > 100


@pytest.mark.parametrize("tag,images", [("P0", 3), ("P1", 3), ("E", 4), ("F", 4)])
def test_float32_nms_reproduces_the_golden_boxes(golden, tag, images):
    total = 0
    for b in range(images):
        want = golden[f"{tag}_boxes{b}"]
        got = R.nms(R.golden_rows(golden[f"{tag}_cand{b}"]), R.NMS_THRESH, R.FINAL_THRESH, np.float32)[:, :5].astype(np.float32)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"{tag} image {b}"
        total += len(want)
    assert total >= 2


@pytest.mark.parametrize("kind,arg", ALL_CASES)
def test_float32_and_float64_nms_agree_on_every_case(kind, arg):
    c = case(kind, arg)
    for thresh in (R.CAND_THRESH, R.FINAL_THRESH):
        rows, _ = R.candidates64(c["heads"], thresh)
        assert [len(r) for r in rows] == c["n_candidates"][thresh]
        for b, r in enumerate(rows):
            r = f32_rows(r)
            i32, i64 = {}, {}
            k32 = R.nms(r, R.NMS_THRESH, R.FINAL_THRESH, np.float32, i32)[:, 5]
            k64 = R.nms(r, R.NMS_THRESH, R.FINAL_THRESH, np.float64, i64)[:, 5]
            assert np.array_equal(k32, k64), f"image {b} at {thresh}: float32 keeps {len(k32)}, float64 {len(k64)}"
            if kind == "nms" and thresh == R.CAND_THRESH:
                _nms_case_proves_something(len(r), i32)


def _nms_case_proves_something(n, info):
    """a large case must keep hundreds of boxes and suppress into the slots q >= 1 of the kernel's threads (sorted positions >= 1024)"""
    if n >= 2049:
        assert len(info["kept"]) >= 200, f"n = {n}: only {len(info['kept'])} boxes kept"
        assert info["suppressed"][1024:].any(), f"n = {n}: nothing suppressed at a sorted position >= 1024"
    if info["sorted_rows"][:, 4].min() > R.FINAL_THRESH:                             # image 0: the walk reaches the last entry, each one is kept or suppressed
        assert len(info["kept"]) + int(info["suppressed"].sum()) == n
    if n >= 129:
        words = np.unique(np.nonzero(info["suppressed"])[0] >> 6)
        assert len(words) >= 2, f"n = {n}: suppressions in one mask word only"


def test_chain_model_keeps_a_and_c():
    c = case("chain")
    rows = f32_rows(R.candidates64(c["heads"], R.CAND_THRESH)[0][0])
    a, b_, c_ = (rows[rows[:, 5] == k][0] for k in c["keys"])
    assert a[4] > b_[4] > c_[4] > 0.5
    assert R.overlap64(a, b_) > 0.3 and R.overlap64(b_, c_) > 0.3 and R.overlap64(a, c_) < 0.3
    for dt in (np.float32, np.float64):
        assert R.nms(rows, R.NMS_THRESH, R.FINAL_THRESH, dt)[:, 5].tolist() == [c["keys"][0], c["keys"][2]]


@pytest.mark.parametrize("variant", TAILS)
def test_tail_cases_are_what_they_claim(variant):
    c = case("tail", variant)
    rows = f32_rows(R.candidates64(c["heads"], R.CAND_THRESH)[0][0])
    info = {}
    kept = R.nms(rows, R.NMS_THRESH, R.FINAL_THRESH, np.float32, info)
    s = info["sorted_rows"][:, 4]
    assert len(rows) == 1500 and np.all(s[:c["top"]] > 0.5) and np.all(s[c["top"]:] < 0.5) and np.all(np.diff(s[:c["top"]]) < 0)
    live = sorted(set(range(c["top"])) - set(c["dups"]))
    assert info["kept"].tolist() == live and len(kept) == len(live)                  # every duplicate of entry 0 is suppressed, every other top entry kept
    assert set(range(64, 70)) <= set(live) or variant == "word1_full"
    if variant != "plain":
        assert live[:2] == [0, 63]
    if variant == "word1_full":
        assert live[2] == 128 and info["suppressed"][64:128].all()


def test_tie_case_has_ties_that_decide():
    """the tied blocks hold equal float32 scores, exactly 1.0f among them, and the descending key order among equals would keep other boxes"""
    c = case("tie")
    rows, _ = R.candidates64(c["heads"], R.CAND_THRESH)
    for r in rows:
        r = f32_rows(r)
        score = r[:, 4]
        assert (score == 1.0).sum() >= 20 and len(np.unique(score)) <= len(score) // 4
        asc = R.nms(r, R.NMS_THRESH, R.FINAL_THRESH, np.float32)
        flipped = r.copy()
        flipped[:, 5] = (1 << 31) - r[:, 5]
        desc = R.nms(flipped, R.NMS_THRESH, R.FINAL_THRESH, np.float32)
        assert not np.array_equal(asc[:, :5], desc[:, :5])
        assert len(asc) >= 10


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------------------
def detect(heads, cand_thresh, perm=None):
    """mf_s3fd_detect_tensors with a workspace of our own and max_det = max_candidates = 4096 -> (candidate rows [B, 4096, 6], boxes, counts, n_candidates), numpy"""
    from mere_fusion_amd import _lib
    _lib.init_device(torch.cuda.current_device())
    ts = [torch.from_numpy(np.array(h if perm is None else h[perm])).cuda() for h in heads]
    B = ts[0].shape[0]
    lib = _lib.lib()
    assert lib.mf_s3fd_detect_workspace_bytes(B, CAP) == B * CAP * 6 * 4
    ws = torch.zeros((B, CAP, 6), dtype=torch.float32, device="cuda")
    boxes = torch.zeros((B, CAP, 5), dtype=torch.float32, device="cuda")
    counts, ncand = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    hw = [d for l in range(6) for d in ts[2 * l].shape[2:]]
    _lib.check(lib.mf_s3fd_detect_tensors((C.c_void_p * 12)(*[t.data_ptr() for t in ts]), (C.c_int * 12)(*hw), B, cand_thresh, R.NMS_THRESH, R.FINAL_THRESH, CAP, CAP,
                                          C.c_void_p(ws.data_ptr()), C.c_void_p(boxes.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(ncand.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "s3fd_detect_tensors")
    torch.cuda.synchronize()
    return ws.cpu().numpy(), boxes.cpu().numpy(), counts.cpu().numpy(), ncand.cpu().numpy()


def assert_equals_model(out, n_expected, tag=""):
    """the kept boxes of every image are bit for bit the float32 model's NMS of the device's own candidate rows; -> the model's info per image"""
    ws, boxes, counts, ncand = out
    assert ncand.tolist() == list(n_expected), f"{tag}: n_candidates {ncand.tolist()}, the case holds {list(n_expected)}"
    infos = []
    for b, n in enumerate(ncand):
        rows = R.device_rows(ws[b, :n])
        assert len(np.unique(rows[:, 5])) == n, f"{tag} image {b}: a key appears twice in the candidate list"
        info = {}
        want = R.nms(rows, R.NMS_THRESH, R.FINAL_THRESH, np.float32, info)[:, :5].astype(np.float32)
        assert counts[b] == len(want), f"{tag} image {b} ({n} candidates): {counts[b]} boxes kept, the model keeps {len(want)}"
        same = (bits(boxes[b, :len(want)]) == bits(want)).all(1)
        assert same.all(), f"{tag} image {b} ({n} candidates): kept box {int(np.argmin(same))} of {len(want)} differs: {boxes[b, int(np.argmin(same))]} vs {want[int(np.argmin(same))]}"
        assert not boxes[b, len(want):].any(), f"{tag} image {b}: rows written past the count"
        infos.append(info)
    return infos


@pytest.mark.gpu
def test_decode_every_row_every_level(lib_built):
    c = case("decode")
    want, mags = R.candidates64(c["heads"], R.CAND_THRESH)
    ws, boxes, counts, ncand = out = detect(c["heads"], R.CAND_THRESH)
    assert ncand.tolist() == c["n_candidates"][R.CAND_THRESH]
    cerr, serr = 0.0, 0.0
    start = R.level_starts(c["maps"])
    for b in range(2):
        got = R.device_rows(ws[b, :ncand[b]])
        got = got[np.argsort(got[:, 5])]
        assert np.array_equal(got[:, 5], want[b][:, 5]), f"image {b}: the device's set of (level, h, w) differs from the model's"
        lv, hh, ww = R.unpack_key(got[:, 5])
        flat = start[lv] + hh * np.array(c["maps"])[lv, 1] + ww
        assert set(c["ends"]) <= set(flat.tolist()) and c["nan_pos"][b] not in flat       # first and last position of every level; the NaN logit is no candidate
        assert np.all(np.bincount(lv, minlength=6) >= 1)
        unit = np.spacing(mags[b].astype(np.float32)).astype(np.float64)
        cerr = max(cerr, float((np.abs(got[:, :4] - want[b][:, :4]) / unit).max()))
        serr = max(serr, float(np.abs(got[:, 4] - want[b][:, 4]).max()))
    print(f"[s3fd decode, {int(ncand.sum())} rows over 6 levels] max coordinate error {cerr:.2f} spacings of the chain's largest intermediate (bound 8), "
          f"max score error {serr:.2e} (bound 1e-6)")
    assert cerr <= 8 and serr <= 1e-6
    assert_equals_model(out, c["n_candidates"][R.CAND_THRESH], "decode case")


@pytest.mark.gpu
@pytest.mark.parametrize("count", R.NMS_SIZES)
def test_nms_matches_float32_model_on_device_candidates(lib_built, count):
    c = case("nms", count)
    answers = []
    for thresh in (R.CAND_THRESH, R.FINAL_THRESH):
        out = detect(c["heads"], thresh)
        infos = assert_equals_model(out, c["n_candidates"][thresh], f"cand_thresh {thresh}")
        if thresh == R.CAND_THRESH:
            for n, info in zip(out[3], infos):
                _nms_case_proves_something(int(n), info)
            print(f"[s3fd nms, {out[3].tolist()} candidates] kept {out[2].tolist()}, suppressed {[int(i['suppressed'].sum()) for i in infos]}")
        answers.append(out)
    assert np.array_equal(bits(answers[0][1]), bits(answers[1][1])) and np.array_equal(answers[0][2], answers[1][2])   # candidates cut at 0.05 or at 0.5: the same boxes


@pytest.mark.gpu
def test_ties_and_saturated_scores_keep_the_documented_order(lib_built):
    c = case("tie")
    first = detect(c["heads"], R.CAND_THRESH)
    assert_equals_model(first, c["n_candidates"][R.CAND_THRESH], "ties")
    for b in range(3):
        s = first[0][b, :first[3][b], 4]
        assert (s == np.float32(1.0)).sum() >= 20 and len(np.unique(s)) <= len(s) // 4                        # the device's scores tie as the model's do
    again = detect(c["heads"], R.CAND_THRESH)
    assert np.array_equal(bits(again[1]), bits(first[1])) and np.array_equal(again[2], first[2]) and np.array_equal(again[3], first[3])
    perm = [2, 0, 1]
    shuffled = detect(c["heads"], R.CAND_THRESH, perm)
    assert_equals_model(shuffled, [c["n_candidates"][R.CAND_THRESH][p] for p in perm], "ties, batch permuted")
    assert np.array_equal(bits(shuffled[1]), bits(first[1][perm])) and np.array_equal(shuffled[2], first[2][perm]) and np.array_equal(shuffled[3], first[3][perm])


@pytest.mark.gpu
def test_chain_suppressed_box_suppresses_nothing(lib_built):
    c = case("chain")
    out = detect(c["heads"], R.CAND_THRESH)
    assert_equals_model(out, [3], "chain")
    ws, boxes, counts, ncand = out
    rows = R.device_rows(ws[0, :3])
    a, cc = (rows[rows[:, 5] == k][0] for k in (c["keys"][0], c["keys"][2]))
    assert counts[0] == 2 and np.array_equal(bits(boxes[0, :2]), bits(np.stack([a[:5], cc[:5]])))             # A and C


@pytest.mark.gpu
@pytest.mark.parametrize("variant", TAILS)
def test_tail_below_final_thresh_and_mask_word_edges(lib_built, variant):
    c = case("tail", variant)
    out = detect(c["heads"], R.CAND_THRESH)
    info = assert_equals_model(out, [1500], f"tail {variant}")[0]
    assert info["kept"].tolist() == sorted(set(range(c["top"])) - set(c["dups"]))                             # the device's candidates make the case the builder meant
    short = detect(c["heads"], R.FINAL_THRESH)
    assert_equals_model(short, [c["top"]], f"tail {variant}, candidates cut at 0.5")
    assert np.array_equal(bits(short[1]), bits(out[1])) and np.array_equal(short[2], out[2])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_planes_path_bit_equal_to_tensor_path(lib_built, precision):
    """mf_s3fd_detect on six 8-channel halo-0 buffers filled through set_input against mf_s3fd_detect_tensors on the same values (bf16-exact, so both
    precisions hold them exactly), level 1's background being the max of its three channels.  The channels the kernel must not read hold 50."""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.avatar.net import Net
    c = case("decode")
    B, maps = 2, c["maps"]
    rng = np.random.default_rng(11)
    rounded = [torch.from_numpy(np.array(h)).bfloat16().float().numpy() for h in c["heads"]]
    n = Net(B, precision)
    bufs = []
    for l, (h, w) in enumerate(maps):
        cls, reg = rounded[2 * l], rounded[2 * l + 1]
        x = np.full((B, 8, h, w), 50.0, np.float32)
        if l == 0:                                                                                           # the max sits in any of the three, the others lie below it
            which = rng.integers(0, 3, (B, h, w))
            lower = torch.from_numpy(cls[:, 0:1] - rng.uniform(0.5, 4.0, (B, 3, h, w)).astype(np.float32)).bfloat16().float().numpy()
            x[:, 0:3] = np.where(np.arange(3)[None, :, None, None] == which[:, None], cls[:, 0:1], lower)
            assert np.array_equal(x[:, 0:3].max(1), cls[:, 0])
            x[:, 3] = cls[:, 1]
        else:
            x[:, 0:2] = cls
        x[:, 4:8] = reg
        bufs.append(n.buffer(8, h, w, 0))
        n.set_input(bufs[-1], torch.from_numpy(x))
        back = n.output(bufs[-1], 8, B).cpu().numpy()
        assert np.array_equal(bits(back), bits(x)), f"level {l + 1}: the buffer does not hold the values exactly"
    boxes = torch.zeros((B, CAP, 5), dtype=torch.float32, device="cuda")
    counts, ncand = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().mf_s3fd_detect(n._h, (C.c_int * 6)(*bufs), B, R.CAND_THRESH, R.NMS_THRESH, R.FINAL_THRESH, CAP, CAP, C.c_void_p(boxes.data_ptr()),
                                         C.c_void_p(counts.data_ptr()), C.c_void_p(ncand.data_ptr()), n._stream()), "s3fd_detect")
    torch.cuda.synchronize()
    ws, tboxes, tcounts, tncand = detect(rounded, R.CAND_THRESH)
    assert tcounts.min() >= 3 and tncand.min() >= 60
    assert np.array_equal(ncand.cpu().numpy(), tncand) and np.array_equal(counts.cpu().numpy(), tcounts)
    assert np.array_equal(bits(boxes.cpu().numpy()), bits(tboxes))
