"""csrc/mf_face_mask.hip and the paste's consumer of its masks where tests/test_face_mask.py's three golden jobs do not reach: calls of more than MF_FM_MAX_JOBS = 16
jobs (the chunk loop of mf_face_mask_finish and mf_face_mask_parse: source index and slot `j0 + i`, the running `packed` offset, chunk-local workspace offsets, the two
`a.out` branches), the accepted limits (151 blur taps with full LDS tiles, a blur radius above the image height, 63 resampling taps), the blur's tile edges (256-pixel
row segments, 64 x 32 column tiles), axes Pillow skips, degenerate windows, a parser graph away from 512 x 512, and refusals that fall into a later chunk.

All inputs are synthetic and seeded; every job of a call gets its own mask, so a mask read at the wrong index cannot pass.  The reference is tests/face_mask_ref.py on the
CPU.  Bars: resize, window, input planes and class masks 0 differing values; the blur the gates of test_face_mask.py::test_finish_stages_on_golden_masks, unchanged --
within 1 level of round(float64) everywhere, equal to round(float64) wherever the float64 value is farther than 1e-2 from a rounding boundary (fp32 error of two passes
of <= 151 taps: 2 x 151 x 2^-24 x 255 ~ 4.6e-3).  The exclusion may take at most 3 % of a mask and must leave >= 1000 clear pixels strictly between 0 and 255; both are
conditions on the reference alone and are also checked without a device (test_blur_gate_conditions_hold_on_the_reference).

The CPU tier also shows that each comparison can fail: the expected side is perturbed the way a plausible kernel bug would (chunk-local mask index, `packed` restarting
per chunk, a single-bounce reflection at 1504 x 40, a 64-column tile seam shifted by one) and the comparison must reject it."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import face_mask_ref as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CHUNK = 16                                   # MF_FM_MAX_JOBS
N_CHUNKED = 37                               # two full chunks and a ragged third
ALONE = (0, 15, 16, 31, 32, 36)
# (w, h) of the chunked call: mutually different, non-square, 34 .. 200; 16 % 7 != 0, so no chunk repeats the layout of the one before
CHUNK_SIZES = [(34, 190), (200, 41), (97, 131), (64, 120), (129, 200), (77, 77), (150, 66)]
# (w, h) of the sweep.  k = 151 with full tiles; k = 151 with radius 75 > h; the widest accepted crop; 53 taps down in x and up in y; odd sizes; the smallest crop (63
# taps); both tables the identity; one axis skipped; the blur's tile edges in x (256, 64) and y (32).  A 512-pixel axis cannot be resampled to fewer than 34 pixels
# (MF_FM_MAX_TAPS), so the crops with h = 31, 32, 33 are cut from the top-left 256 x 256 of the generator's mask (source_size)
GEOMETRY = [(1504, 1504), (1504, 40), (1519, 64), (40, 700), (333, 517), (34, 34), (512, 512), (512, 300), (300, 512),
            (255, 31), (256, 32), (257, 33), (64, 33), (65, 31), (63, 32), (255, 33), (256, 31), (257, 32), (64, 31), (65, 32), (63, 33)]
WINDOW_SIZES = [(97, 131), (257, 33)]
PARSE_S = 64                                 # the smallest size of 64, 96, 128 at which the BiSeNet graph builds
PARSE_JOBS = 20


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parser_mask(kind, seed):
    """a 512 x 512 parser mask.  "prod": values {0, 255}, an off-centre ellipse XOR 2 % salt noise (bicubic overshoot clips at both ends); "full": random uint8 (the C
    entry accepts any value, and only these work clip8 hard)"""
    rng = np.random.default_rng([seed, int(kind == "prod")])
    if kind == "full":
        m = rng.integers(0, 256, (512, 512), dtype=np.uint8)
    else:
        cx, cy = 256 + rng.choice([-1, 1], 2) * rng.uniform(40, 110, 2)
        ax, ay = rng.uniform(80, 190, 2)
        yy, xx = np.mgrid[:512, :512]
        inside = ((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2 <= 1.0
        m = ((inside ^ (rng.random((512, 512)) < 0.02)) * 255).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ref_pre(kind, seed, job):
    """the windowed bicubic resize of parser_mask(kind, seed) for job = (w, h, rx0, ry0, rx1, ry1, top): Pillow-exact integers"""
    w, h, rx0, ry0, rx1, ry1, top = job
    out = R.window(R.resize_u8(source(kind, seed, job), (w, h), R.BICUBIC), (rx0, ry0, rx1, ry1), (0, 0), top=top)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_blur(kind, seed, job):
    """float64, not rounded"""
    f64 = R.gaussian_blur(ref_pre(kind, seed, job), R.blur_kernel_size(job[0]))
    f64.setflags(write=False)
    return f64


def source_size(job):
    """side of the square parser mask a job is resampled from: the generator's 512, or its top-left 256 x 256 for a crop with a side below 34"""
    return 512 if min(job[:2]) >= 34 else 256


def source(kind, seed, job):
    s = source_size(job)
    return parser_mask(kind, seed)[:s, :s]


def full_window(w, h):
    return (w, h, 0, 0, w, h, 0)


def chunk_job(i):
    """job i of the chunked call: (kind, seed, job); every job its own mask and its own window"""
    w, h = CHUNK_SIZES[i % len(CHUNK_SIZES)]
    rng = np.random.default_rng(1000 + i)
    rx0, ry0 = int(rng.integers(0, w // 4)), int(rng.integers(0, h // 4))
    rx1, ry1 = int(rng.integers(w - w // 4, w + 1)), int(rng.integers(h - h // 4, h + 1))
    top = h // 2 if i % 5 == 0 else int(rng.integers(0, h // 3))           # every fifth job the production window (upper_boundary_ratio 0.5)
    return ("full" if i % 3 == 2 else "prod", 100 + i, (w, h, rx0, ry0, rx1, ry1, top))


def window_jobs(w, h):
    """(job, all zero?) -- the full crop, an empty rectangle, top = 0 with a partial rectangle, top >= h (twice), a one-pixel rectangle"""
    return [(full_window(w, h), False), ((w, h, w // 3, h // 4, w // 3, h - 2, 0), True), ((w, h, 3, 5, w - 7, h - 2, 0), False),
            ((w, h, 0, 0, w, h, h), True), ((w, h, 0, 0, w, h, h + 9), True), ((w, h, w // 2, h // 2, w // 2 + 1, h // 2 + 1, 0), False)]


# ---- the comparisons, shared by the GPU tests and the CPU checks that they can fail -------------------------------------------------------------------
def blur_conditions(f64):
    """(share of the mask within 1e-2 of a rounding boundary, clear pixels whose rounded value is strictly between 0 and 255)"""
    near = np.abs(f64 - np.floor(f64) - 0.5) <= 1e-2
    want = np.clip(np.rint(f64), 0, 255)
    return float(near.mean()), int((~near & (want > 0) & (want < 255)).sum())


def blur_gate(name, got, f64, k, edges=1000):
    got = got.astype(np.float64)
    want = np.clip(np.rint(f64), 0, 255)
    clear = np.abs(f64 - np.floor(f64) - 0.5) > 1e-2
    near, inside = blur_conditions(f64)
    print(f"[face mask blur {name}] k = {k}: max |device - float64| {np.abs(got - f64).max():.4f} (gate: within 1 level of round), "
          f"{int((got != want)[clear].sum())} of {int(clear.sum())} clear pixels differ from round(float64), {int((got != want).sum())} of all {got.size}; "
          f"{near:.2%} near a boundary, {inside} clear pixels strictly between 0 and 255")
    assert got.shape == f64.shape
    assert near <= 0.03 and inside >= edges, (name, near, inside)
    assert np.abs(got - want).max() <= 1, name
    assert np.array_equal(got[clear], want[clear]), name


def assert_exact(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} differing values of {want.size}"


def as_device_would(f64):
    """the stand-in for a correct device result in the CPU checks: one rounding of the float64 value"""
    return np.clip(np.rint(f64), 0, 255).astype(np.uint8)


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------
def test_generator_kinds_and_distinct_masks():
    prod, full = parser_mask("prod", 3), parser_mask("full", 3)
    assert prod.shape == full.shape == (512, 512) and prod.dtype == full.dtype == np.uint8
    assert set(np.unique(prod)) == {0, 255} and len(np.unique(full)) == 256
    share = (prod > 0).mean()
    assert 0.1 < share < 0.7
    yy, xx = np.nonzero(prod)
    assert abs(xx.mean() - 255.5) > 10 or abs(yy.mean() - 255.5) > 10                             # off centre
    seg = R.resize_u8(prod, (200, 200), R.BICUBIC)                                                # overshoot reaches both clips, and the values between exist
    assert (seg == 0).any() and (seg == 255).any() and ((seg > 0) & (seg < 255)).any()
    masks = [parser_mask(*chunk_job(i)[:2]) for i in range(N_CHUNKED)]
    assert len({m.tobytes() for m in masks}) == N_CHUNKED
    jobs = [chunk_job(i)[2] for i in range(N_CHUNKED)]
    assert len({j[2:] for j in jobs}) == N_CHUNKED                                                # windows differ per job
    assert len(set(CHUNK_SIZES)) == len(CHUNK_SIZES) and all(34 <= v <= 200 for s in CHUNK_SIZES for v in s) and any(w != h for w, h in CHUNK_SIZES)
    assert all(0 <= j[2] <= j[4] <= j[0] and 0 <= j[3] <= j[5] <= j[1] for j in jobs)


def test_reflect_loop_equals_numpy_reflect_padding():
    """the blur's border rule (R.reflect101 restates the kernel's loop) is numpy's "reflect" padding, the reference's: also where the radius exceeds the length and the
    index bounces more than once"""
    for n, r in [(40, 75), (2, 75), (1504, 75), (31, 12), (34, 1), (64, 75)]:
        assert np.array_equal(R.reflect101(np.arange(-r, n + r), n), np.pad(np.arange(n), r, mode="reflect")), (n, r)
    assert not R.reflect101(np.arange(-5, 6), 1).any()
    assert (75 // (40 - 1)) >= 1 and R.reflect101(np.array([-75]), 40)[0] == 3                    # -75 -> 75 -> 3: two bounces at (40, 75)
    m = parser_mask("prod", 1)[:40, :300]
    assert np.array_equal(R.gaussian_blur(m, 151), R.gaussian_blur(m, 151, index=R.reflect101))


def test_kernel_sizes_and_tap_counts_of_the_sweep():
    from mere_fusion_amd.avatar.face_parsing import blur_kernel_size
    assert [blur_kernel_size(w) for w in (1500, 1504, 1519, 1520, 34, 63, 255, 256, 257)] == [R.blur_kernel_size(w) for w in (1500, 1504, 1519, 1520, 34, 63, 255, 256, 257)] \
        == [151, 151, 151, 153, 3, 7, 25, 25, 25]
    assert R.coeffs(512, 40, R.BICUBIC)[2].shape[1] == 53 and R.coeffs(512, 34, R.BICUBIC)[2].shape[1] == 63 and R.coeffs(512, 33, R.BICUBIC)[2].shape[1] == 65
    assert int(R.coeffs(512, 34, R.BICUBIC)[1].max()) <= 63
    for size in GEOMETRY + WINDOW_SIZES + CHUNK_SIZES:                       # every case of this file is inside the limits for the source it is cut from
        s = source_size(size)
        assert all(s == v or R.coeffs(s, v, R.BICUBIC)[2].shape[1] <= 64 for v in size) and R.blur_kernel_size(size[0]) <= 151, size
    assert R.coeffs(512, 31, R.BICUBIC)[2].shape[1] == 69 and {source_size(s) for s in GEOMETRY} == {256, 512}


@pytest.mark.parametrize("size", GEOMETRY + WINDOW_SIZES, ids=lambda s: "%dx%d" % s)
def test_blur_gate_conditions_hold_on_the_reference(size):
    """what the 1e-2 exclusion leaves, from the reference alone: at most 3 % of the mask excluded, at least 1000 clear pixels strictly between 0 and 255"""
    near, inside = blur_conditions(ref_blur("prod", 7, full_window(*size)))
    print(f"[face mask blur conditions {size}] {near:.2%} near a boundary, {inside} clear pixels strictly between 0 and 255")
    assert near <= 0.03 and inside >= 1000


def test_blur_gate_conditions_hold_on_the_chunked_jobs():
    for i in range(N_CHUNKED):
        near, inside = blur_conditions(ref_blur(*chunk_job(i)))
        assert near <= 0.03 and inside >= 1000, (i, near, inside)


def _refused(l, n_jobs, bad_at, w, h):
    jobs = [(64, 64, 0, 0, 64, 64, 32)] * n_jobs
    jobs[bad_at] = (w, h, 0, 0, w, h, h // 2)
    flat = (C.c_int * (7 * n_jobs))(*[v for j in jobs for v in j])
    dummy = C.c_void_p(256)                                                   # never dereferenced: the geometry is refused before any launch
    rc = l.mf_face_mask_finish(dummy, 512, 512, flat, n_jobs, 1, dummy, 1 << 40, dummy, dummy, None)
    return rc, l.mf_last_error()


def test_refusals_at_the_limits_need_no_device(lib_built):
    """one past each accepted limit, alone and as the first job of a second chunk: the entry point names the limit and the job, and on a machine without a device this
    passes only if no launch is attempted before the refusal"""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.avatar import face_parsing as FP
    l = _lib.lib()
    for n_jobs, bad_at in ((1, 0), (17, 16), (37, 35)):
        rc, msg = _refused(l, n_jobs, bad_at, 1520, 1520)
        assert rc == -1 and b"153-tap blur" in msg and b"MF_FM_BLUR_MAX_K = 151" in msg and b"job %d:" % bad_at in msg, msg
        rc, msg = _refused(l, n_jobs, bad_at, 33, 33)
        assert rc == -1 and b"MF_FM_MAX_TAPS = 64" in msg and b"65 taps" in msg and b"job %d:" % bad_at in msg, msg
        for w in (1520, 33):
            sizes = [(64, 64)] * n_jobs
            sizes[bad_at] = (w, 64)
            assert l.mf_face_mask_workspace_bytes(1, (C.c_int * (2 * n_jobs))(*[v for s in sizes for v in s]), n_jobs, 512, 512) == 0
            assert FP.workspace_bytes(1, sizes, 512, 512) == 256              # the wrapper's "refused": the entry point then says why
    rc, msg = _refused(l, 17, 16, 64, 0)
    assert rc == -1 and b"job 16: empty crop" in msg
    # the accepted limits themselves are sized, not refused
    for w, h in ((1519, 64), (34, 34), (1504, 1504)):
        assert l.mf_face_mask_workspace_bytes(1, (C.c_int * 2)(w, h), 1, 512, 512) > w * h * 5


# ---- the comparisons can fail: the expected side perturbed the way a kernel bug would ------------------------------------------------------------------
def _split(flat, jobs):
    out, o = [], 0
    for j in jobs:
        out.append(flat[o:o + j[0] * j[1]].reshape(j[1], j[0]))
        o += j[0] * j[1]
    return out


def test_comparisons_reject_a_chunk_local_mask_index():
    """`j.src = i` instead of `j0 + i`: from the second chunk on, job i would be built from mask i - j0"""
    for i in (16, 17, 31, 32, 36):
        kind, seed, job = chunk_job(i)
        wrong_kind, wrong_seed, _ = chunk_job(i % CHUNK)
        buggy_pre = ref_pre(wrong_kind, wrong_seed, job)
        with pytest.raises(AssertionError):
            assert_exact(f"job {i}", buggy_pre, ref_pre(kind, seed, job))
        with pytest.raises(AssertionError):
            blur_gate(f"job {i}, chunk-local index", as_device_would(R.gaussian_blur(buggy_pre, R.blur_kernel_size(job[0]))), ref_blur(kind, seed, job), R.blur_kernel_size(job[0]))
        blur_gate(f"job {i}, unperturbed", as_device_would(ref_blur(kind, seed, job)), ref_blur(kind, seed, job), R.blur_kernel_size(job[0]))


def test_comparisons_reject_a_packed_offset_that_restarts_per_chunk():
    cases = [chunk_job(i) for i in range(N_CHUNKED)]
    jobs = [c[2] for c in cases]
    flat = np.zeros(sum(j[0] * j[1] for j in jobs), np.uint8)
    for j0 in range(0, N_CHUNKED, CHUNK):
        o = 0                                                                # the bug: `packed` restarts with every chunk
        for c in cases[j0:j0 + CHUNK]:
            flat[o:o + c[2][0] * c[2][1]] = ref_pre(*c).ravel()
            o += c[2][0] * c[2][1]
    rejected = []
    for i, got in enumerate(_split(flat, jobs)):
        try:
            assert_exact(f"job {i}", got, ref_pre(*cases[i]))
        except AssertionError:
            rejected.append(i)
    print(f"[face mask perturbation] packed restarting per chunk: jobs rejected {rejected}")
    assert set(range(CHUNK, N_CHUNKED)) <= set(rejected) and 0 in rejected   # every job of a later chunk, and the jobs they overwrote


def test_blur_gate_rejects_a_single_bounce_reflection():
    """(1504, 40), radius 75: an index reflected once and then clamped (what a non-looping reflect101 kept in bounds would read)"""
    job = full_window(1504, 40)
    pre, f64 = ref_pre("prod", 7, job), ref_blur("prod", 7, job)

    def single(i, n):
        return np.clip(np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i)), 0, n - 1)

    blur_gate("1504x40 loop formula", as_device_would(R.gaussian_blur(pre, 151, index=R.reflect101)), f64, 151)
    with pytest.raises(AssertionError):
        blur_gate("1504x40 single bounce", as_device_would(R.gaussian_blur(pre, 151, index=single)), f64, 151)


def test_blur_gate_rejects_a_tile_seam_shifted_by_one():
    """the first column of every 64-column tile of k_fm_blur_v computed from the column to its left"""
    for size in ((257, 64), (65, 31)):
        f64 = ref_blur("prod", 7, full_window(*size))
        good = as_device_would(f64)
        bad = good.copy()
        seam = np.arange(64, size[0], 64)
        bad[:, seam] = good[:, seam - 1]
        blur_gate(f"{size} unperturbed", good, f64, R.blur_kernel_size(size[0]))
        with pytest.raises(AssertionError):
            blur_gate(f"{size} seam shifted", bad, f64, R.blur_kernel_size(size[0]))


# ---- GPU tier: finish_masks over more than one chunk ------------------------------------------------------------------------------------------------
def _finish(cases, **kw):
    from mere_fusion_amd.avatar import finish_masks
    masks = torch.from_numpy(np.stack([source(*c) for c in cases])).cuda()
    res = finish_masks(masks, [c[2] for c in cases], **kw)
    if isinstance(res, tuple):
        return tuple([m.cpu().numpy() for m in r] for r in res)
    return [m.cpu().numpy() for m in res]


@pytest.fixture(scope="module")
def chunked(lib_built):
    cases = [chunk_job(i) for i in range(N_CHUNKED)]
    blurred, pre = _finish(cases, want_pre_blur=True)
    return dict(cases=cases, blurred=blurred, pre=pre, blurred_alone=_finish(cases), only_pre=_finish(cases, blur=False))


@pytest.mark.gpu
def test_chunked_windowed_resize_exact(chunked):
    for i, c in enumerate(chunked["cases"]):
        assert_exact(f"job {i} of {N_CHUNKED}, blur=False", chunked["only_pre"][i], ref_pre(*c))
        assert_exact(f"job {i} of {N_CHUNKED}, want_pre_blur", chunked["pre"][i], chunked["only_pre"][i])


@pytest.mark.gpu
def test_chunked_blur_same_from_given_and_workspace_pre_blur(chunked):
    """the two branches of `a.out`: the caller's pre_blur buffer at the running packed offset, the workspace's chunk-local one"""
    for i in range(N_CHUNKED):
        assert_exact(f"job {i}: blurred with and without want_pre_blur", chunked["blurred"][i], chunked["blurred_alone"][i])


@pytest.mark.gpu
def test_chunked_blur_gate(chunked):
    for i, c in enumerate(chunked["cases"]):
        blur_gate(f"job {i} of {N_CHUNKED} {c[2][:2]}", chunked["blurred"][i], ref_blur(*c), R.blur_kernel_size(c[2][0]))


@pytest.mark.gpu
def test_chunked_job_equals_the_job_alone(chunked):
    for i in ALONE:
        blurred, pre = _finish([chunked["cases"][i]], want_pre_blur=True)
        assert_exact(f"job {i} alone, windowed", pre[0], chunked["pre"][i])
        assert_exact(f"job {i} alone, blurred", blurred[0], chunked["blurred"][i])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 17])
def test_calls_of_exactly_one_chunk_and_one_more(lib_built, n):
    cases = [chunk_job(i) for i in range(N_CHUNKED - n, N_CHUNKED)]          # the last n jobs: another chunk alignment than the 37-job call
    blurred, pre = _finish(cases, want_pre_blur=True)
    only = _finish(cases)
    for i, c in enumerate(cases):
        assert_exact(f"job {i} of {n}, windowed", pre[i], ref_pre(*c))
        assert_exact(f"job {i} of {n}, blurred with and without want_pre_blur", blurred[i], only[i])
        blur_gate(f"job {i} of {n} {c[2][:2]}", blurred[i], ref_blur(*c), R.blur_kernel_size(c[2][0]))


# ---- GPU tier: geometry sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_geometry_sweep(lib_built, size):
    """both mask kinds through resize + window (0 differing values), the production-like one through the blur (the gate)"""
    job = full_window(*size)
    cases = [("full", 11, job), ("prod", 7, job)]
    blurred, pre = _finish(cases, want_pre_blur=True)
    only_pre = _finish(cases, blur=False)
    for i, c in enumerate(cases):
        assert_exact(f"{size} {c[0]}, windowed resize", only_pre[i], ref_pre(*c))
        assert_exact(f"{size} {c[0]}, want_pre_blur", pre[i], only_pre[i])
    blur_gate(f"{size}", blurred[1], ref_blur(*cases[1]), R.blur_kernel_size(size[0]))
    assert_exact(f"{size}: the production-like job alone", _finish(cases[1:])[0], blurred[1])


@pytest.mark.gpu
@pytest.mark.parametrize("size", WINDOW_SIZES, ids=lambda s: "%dx%d" % s)
def test_degenerate_windows(lib_built, size):
    wj = window_jobs(*size)
    for kind in ("prod", "full"):
        cases = [(kind, 40 + i, j) for i, (j, _) in enumerate(wj)]
        blurred, pre = _finish(cases, want_pre_blur=True)
        for i, (c, (_, zero)) in enumerate(zip(cases, wj)):
            assert_exact(f"{size} {kind} window {c[2][2:]}", pre[i], ref_pre(*c))
            if zero:
                assert not pre[i].any() and not blurred[i].any(), c[2]
            else:
                assert pre[i].any()
                blur_gate(f"{size} {kind} window {c[2][2:]}", blurred[i], ref_blur(*c), R.blur_kernel_size(size[0]),
                          edges=0 if c[2][4] - c[2][2] == 1 else 1000)             # a blurred single pixel spreads to a few dozen levels at most (97 x 131)
                                                                                   # or rounds away (257 x 33); every other window keeps the condition


@pytest.mark.gpu
def test_refusal_in_a_later_chunk_launches_nothing(lib_built):
    """17 jobs, the seventeenth one past a limit: the call is refused naming the limit, and no byte of the outputs or of the workspace is written -- the first chunk,
    which is acceptable on its own, must not have been launched"""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.avatar import finish_masks
    masks = torch.full((17, 512, 512), 255, dtype=torch.uint8, device="cuda")
    for w, h, words in ((1520, 64, "153-tap blur"), (33, 64, "MF_FM_MAX_TAPS = 64")):
        jobs = [(64, 64, 0, 0, 64, 64, 0)] * 16 + [(w, h, 0, 0, w, h, 0)]
        ws = torch.full((1 << 24,), 0xA5, dtype=torch.uint8, device="cuda")
        pre, out = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
        flat = (C.c_int * (7 * 17))(*[v for j in jobs for v in j])
        rc = _lib.lib().mf_face_mask_finish(masks.data_ptr(), 512, 512, flat, 17, 1, ws.data_ptr(), ws.numel(), pre.data_ptr(), out.data_ptr(), _lib.stream_ptr(masks.device))
        assert rc == -1 and words.encode() in _lib.lib().mf_last_error() and b"job 16:" in _lib.lib().mf_last_error()
        torch.cuda.synchronize()
        assert bool((ws == 0xA5).all()) and bool((pre == 0xA5).all()) and bool((out == 0xA5).all())
        with pytest.raises(RuntimeError, match=words):
            finish_masks(masks, jobs)
    # and the same 16 jobs without the seventeenth are served
    assert all(bool((m == 255).all()) for m in finish_masks(masks[:16], jobs[:16], blur=False))


# ---- GPU tier: parse beyond one chunk and away from 512 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_face_mask_golden", os.path.join(ROOT, "tests", "golden", "make_face_mask_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def parse_inputs(gen, S):
    """three 150 x 180 frames and 20 (frame index, box): boxes that leave the frame on each side and on all, a one-pixel-wide and a one-pixel-high box, a box of exactly
    S x S, one of width S and one of height S (an axis Pillow skips), up- and downscales; rotated so that the special boxes straddle the chunk boundary at slot 16"""
    rng = np.random.default_rng(20)
    H, W = 150, 180
    frames = np.stack([gen.two_tone(rng, H, W, 23), gen.blocks(rng, H, W, 9), gen.two_tone(rng, H, W, 11)])
    boxes = [(-10, 5, 50, 70), (80, -12, 118, 40), (140, 20, 195, 85), (20, 100, 90, 161), (-7, -9, 187, 159),
             (30, 10, 31, 80), (10, 40, 100, 41), (25, 13, 25 + S, 13 + S), (5, 5, 5 + S, 100), (40, 30, 171, 30 + S)]
    while len(boxes) < PARSE_JOBS:
        w, h = int(rng.integers(9, 170)), int(rng.integers(9, 140))
        x, y = int(rng.integers(-5, W - w + 6)), int(rng.integers(-5, H - h + 6))
        boxes.append((x, y, x + w, y + h))
    boxes = boxes[10:] + boxes[:10]
    assert len(set(boxes)) == PARSE_JOBS and boxes[15][2] - boxes[15][0] == 1 and boxes[16][3] - boxes[16][1] == 1 and boxes[17] == (25, 13, 25 + S, 13 + S)
    return frames, boxes, [(7 * i + 1) % 3 for i in range(PARSE_JOBS)]


def _normalise(crop):
    t = torch.from_numpy(np.ascontiguousarray(crop.transpose(2, 0, 1))).float().div(255)
    return (t - torch.tensor([0.485, 0.456, 0.406])[:, None, None]) / torch.tensor([0.229, 0.224, 0.225])[:, None, None]


def host_crops(gen, S):
    frames, boxes, idx = parse_inputs(gen, S)
    return torch.stack([_normalise(R.resize_u8(R.crop_u8(frames[f][:, :, ::-1], b), (S, S), R.BILINEAR)) for f, b in zip(idx, boxes)])


@pytest.fixture(scope="module")
def fp20(lib_built, gen):
    """a FaceParsing of capacity 20 whose masks follow the image at S x S.  With the seeded BiSeNet weights one background class wins on nearly every pixel of these
    crops, and 20 empty masks could not tell one slot from another.  So the head is recombined, as make_face_mask_golden.py gives its head contrast: the logits L of
    the seeded net over the 20 crops are measured once, a = their first principal direction with the mean logit projected out, and the new 1 x 1 head has row 1 (a
    mask class) = a . W, row 0 = -a . W and zeros elsewhere, so its logits are +-(a . L): zero mean over the crops, the sign following the image."""
    from mere_fusion_amd.avatar import FaceParsing
    sd = gen.state_dict()
    x = host_crops(gen, PARSE_S)
    logits = FaceParsing(state_dict=sd, max_batch=PARSE_JOBS).net(x)[0].double().cpu()
    flat = logits.permute(1, 0, 2, 3).reshape(logits.shape[1], -1)
    mu = flat.mean(1)
    a = torch.linalg.svd(flat - mu[:, None], full_matrices=False)[0][:, 0]
    a = a - (a @ mu) / (mu @ mu) * mu
    w0 = sd["conv_out.conv_out.weight"].double()[:, :, 0, 0]
    w1 = torch.zeros_like(w0)
    w1[1], w1[0] = a @ w0, -(a @ w0)
    return FaceParsing(state_dict=gen.state_dict(w1.float()[:, :, None, None]), max_batch=PARSE_JOBS)


def test_parse_inputs_are_distinct(gen):
    frames, boxes, idx = parse_inputs(gen, PARSE_S)
    crops = [R.resize_u8(R.crop_u8(frames[f][:, :, ::-1], b), (PARSE_S, PARSE_S), R.BILINEAR) for f, b in zip(idx, boxes)]
    assert len({c.tobytes() for c in crops}) == PARSE_JOBS and len(set(idx)) == 3 and idx != sorted(idx)
    assert all(c.shape == (PARSE_S, PARSE_S, 3) for c in crops)


@pytest.mark.gpu
def test_parse_twenty_jobs_at_a_small_size(fp20, gen):
    """20 jobs = one full chunk of the resampler and a ragged second, at S x S: every slot's input planes bit-equal to set_input of the host-normalised Pillow-exact
    crop, every slot's mask equal to numpy's class mask of the same handle's own logits on every pixel"""
    S = PARSE_S
    frames, boxes, idx = parse_inputs(gen, S)
    x = host_crops(gen, S)
    g = fp20._graph((S, S))
    n = g["net"]
    n.set_input(g["inp"], x)
    want = n.output(g["inp"], 8, PARSE_JOBS).cpu()
    n.set_input(g["inp"], torch.zeros_like(x))
    dev = torch.from_numpy(frames).cuda()
    got_masks = fp20.parse(dev, boxes, frame_indices=idx, size=(S, S)).cpu().numpy()
    got = n.output(g["inp"], 8, PARSE_JOBS).cpu()
    assert got.shape == (PARSE_JOBS, 8, S, S)
    for b in range(PARSE_JOBS):
        differing = int((got[b, :3].view(torch.int32) != want[b, :3].view(torch.int32)).sum())
        assert differing == 0, f"slot {b}, box {boxes[b]}, frame {idx[b]}: {differing} differing plane values of {3 * S * S}"
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not got[:, 3:].any()
    logits = fp20.net(x)[0].cpu().numpy()
    assert logits.shape == (PARSE_JOBS, 19, S, S) and got_masks.shape == (PARSE_JOBS, S, S)
    want_masks = [R.class_mask(logits[b]) for b in range(PARSE_JOBS)]
    shares = [float((m > 0).mean()) for m in want_masks]
    print(f"[face mask parse {PARSE_JOBS} jobs at {S} x {S}] foreground shares {' '.join(f'{s:.2f}' for s in shares)}")
    for b in range(PARSE_JOBS):
        assert np.array_equal(got_masks[b], want_masks[b]), f"slot {b}: {(got_masks[b] != want_masks[b]).sum()} pixels differ"
    # a mask from the wrong slot cannot pass: the expected masks differ from slot to slot, and most of them are neither empty nor full
    assert len({m.tobytes() for m in want_masks}) >= PARSE_JOBS - 2 and sum(0.02 < s < 0.98 for s in shares) >= PARSE_JOBS // 2
    # a refusal in the second chunk leaves the first chunk's planes unwritten
    n.set_input(g["inp"], torch.zeros_like(x))
    with pytest.raises(RuntimeError, match="job 17: frame index 9"):
        fp20.parse(dev, boxes, frame_indices=idx[:17] + [9] + idx[18:], size=(S, S))
    torch.cuda.synchronize()
    assert not n.output(g["inp"], 8, PARSE_JOBS).any()
